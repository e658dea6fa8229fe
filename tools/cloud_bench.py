#!/usr/bin/env python
"""Point clouds of predict_frames' results on the MI355X (gwd_point_cloud):

    python tools/cloud_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

  call            ops.point_cloud on the depth / labels / region_map / planes that predict_frames returned, with the frames' colour
                  and normals, at stride 1 and stride 2: device events over back-to-back calls, and the time of each of the three
                  launches (count, scan, emit) from the profiler's kernel records; the bytes the emit pass stores (the whole cloud,
                  points and zero tail) over its time, next to a device-to-device copy of the same number of bytes in the same run;
                  at stride 1 also without normals, colour and regions (the same stores, the least arithmetic per point);
  arms            predict_frames(intrinsics=) of a session without cloud= (the launches and keys of the parent commit) and with it,
                  alternated in one process;
  host            the route it replaces: depth, labels and the frames copied to the host, numpy unprojection in fp64, a boolean
                  mask and np.concatenate (host clock around it, the copies included; no normals, no edge rule).
Prints one JSON line and writes it to profiles/cloud_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("cloud_count_kernel", "cloud_scan_kernel", "cloud_emit_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("cloud_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from torch.profiler import ProfilerActivity, profile

    from gw_depth_amd import Config, build_model, hip, ops
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.synth import det_fill_
    assert not getattr(hip.library(), "is_fake", False)
    B, fh, fw, steps = args.frames, args.height, args.width, args.steps

    def event_ms(fn, reps=20, windows=5):
        fn()
        times = []
        for _ in range(windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) / reps)
        return statistics.median(times)

    def kernel_ms(fn, reps=10):
        """ms per launch of the three kernels from the profiler's kernel records; None where this host has no tracer."""
        fn()
        torch.cuda.synchronize()
        found = {}
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            for e in prof.key_averages():
                for k in KERNELS:
                    if k in e.key:
                        found[k] = round(e.device_time_total / max(e.count, 1) / 1e3, 5)
        except Exception:
            pass
        return {k: found.get(k) for k in KERNELS}

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    kw = dict(compute_dtype=torch.bfloat16, graph=True, line_nms=0.01, regions=True, line_profiles=True)
    plain = InferenceSession(model, **kw)
    with_cloud = InferenceSession(model, cloud=True, **kw)
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(B):
        low = torch.rand(1, 3, 9, 16, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(fh, fw), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    cam = torch.tensor([(0.9 * fw, 0.9 * fw, fw / 2.0, fh / 2.0)] * B, dtype=torch.float64)
    res = with_cloud.predict_frames(frames, intrinsics=cam)
    torch.cuda.synchronize()
    on_dev, cam_dev = [f.cuda() for f in frames], cam.cuda()
    out = {"tool": "cloud_bench", "frames": B, "frame_height": fh, "frame_width": fw, "device": torch.cuda.get_device_name(0),
           "predicted": {"points": int(res["cloud_offsets"][-1]), "capacity": int(res["cloud"].shape[0]),
                         "region_count": res["region_count"].tolist()}, "call": {}}
    for stride in (1, 2):
        fn = lambda: ops.point_cloud(res["depth_planar"], res["labels"], res["sizes"], cam_dev, frames=on_dev, region_map=res["region_map"],
                                     region_count=res["region_count"], planes=res["planes"], stride=stride, min_depth=with_cloud.min_depth,
                                     max_depth=with_cloud.max_depth)
        cloud = fn()
        torch.cuda.synchronize()
        stored = int(cloud["cloud"].numel())
        src, dst = cloud["cloud"].clone(), torch.empty_like(cloud["cloud"])
        copy_ms = event_ms(lambda: dst.copy_(src))
        call_ms, k_ms = event_ms(fn), kernel_ms(fn)
        emit = k_ms["cloud_emit_kernel"]
        out["call"][str(stride)] = {
            "points": int(cloud["cloud_offsets"][-1]), "rows": int(cloud["cloud"].shape[0]), "bytes_stored": stored,
            "call_ms": round(call_ms, 5), "kernel_ms": k_ms, "emit_gb_per_s_stored": None if not emit else round(stored / emit / 1e6, 1),
            "copy_ms": round(copy_ms, 5), "copy_gb_per_s_stored": round(stored / copy_ms / 1e6, 1),
            "emit_over_copy_rate": None if not emit else round(copy_ms / emit, 3)}
    # the same stores with the least work per point: no normals, no colour, no regions - what of the emit time is the record's arithmetic
    bare = lambda: ops.point_cloud(res["depth_planar"], res["labels"], res["sizes"], cam_dev, normals=False, min_depth=with_cloud.min_depth,
                                   max_depth=with_cloud.max_depth)
    k_ms = kernel_ms(bare)
    emit = k_ms["cloud_emit_kernel"]
    out["call"]["1_bare"] = {"kernel_ms": k_ms, "emit_gb_per_s_stored": None if not emit else round(out["call"]["1"]["bytes_stored"] / emit / 1e6, 1),
                             "emit_over_copy_rate": None if not emit else round(out["call"]["1"]["copy_ms"] / emit, 3)}
    out["call"]["note"] = ("call_ms: device events over 20 back-to-back ops.point_cloud calls, allocation and launch gaps included; kernel_ms: "
                           "per launch, from the profiler; emit_gb_per_s_stored: the cloud's bytes over the emit launch (its reads - depth five "
                           "times, labels, region_map, the frames - come on top); copy: torch copy_ of the same bytes, device to device")

    calls = {"predict_frames": lambda: plain.predict_frames(frames, intrinsics=cam),
             "predict_frames_cloud": lambda: with_cloud.predict_frames(frames, intrinsics=cam)}
    for a in calls:
        for _ in range(max(args.warmup, 1)):
            calls[a]()
        torch.cuda.synchronize()
    windows = {a: [] for a in calls}
    arms, rounds = list(calls), 0
    while any(len(windows[a]) < 3 or sum(windows[a]) * steps / 1e3 < args.min_seconds for a in arms):
        k = rounds % len(arms)
        rounds += 1
        for a in arms[k:] + arms[:k]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(steps):
                calls[a]()
            t1.record()
            t1.synchronize()
            windows[a].append(t0.elapsed_time(t1) / steps)
    out["arms"] = {a: {"ms_per_call": round(statistics.median(w), 4), "ms_min": round(min(w), 4), "ms_max": round(max(w), 4), "windows": len(w)}
                   for a, w in windows.items()}
    out["arms"]["note"] = ("predict_frames: a session without cloud= issues the parent commit's launches; both with line_nms=0.01, regions=True, "
                           "line_profiles=True and intrinsics; the cloud arm at stride 1 with colour and normals")

    def host_route():
        """What the cloud costs without the kernels: the planes and frames to the host, fp64 unprojection, a mask, a concatenate."""
        depth, labels = res["depth_planar"].cpu().numpy().astype(np.float64), res["labels"].cpu().numpy()
        y, x = np.meshgrid(np.arange(fh, dtype=np.float64), np.arange(fw, dtype=np.float64), indexing="ij")
        parts = []
        for b in range(B):
            fx, fy, cx, cy = cam[b].tolist()
            z = depth[b]
            keep = np.isfinite(z) & (z >= with_cloud.min_depth) & (z <= with_cloud.max_depth) & (labels[b] != 255)
            xyz = np.stack([(x - cx) * z / fx, (y - cy) * z / fy, z], axis=-1)[keep].astype(np.float32)
            parts.append((xyz, frames[b].numpy()[keep], labels[b][keep]))
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])

    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    out["host"] = {"ms_per_call": round(statistics.median(host), 3), "ms_min": round(min(host), 3), "ms_max": round(max(host), 3),
                   "windows": len(host), "note": "depth / labels .cpu(), numpy unprojection in fp64, boolean mask, np.concatenate; stride 1, "
                                                  "no normals, no edge rule"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

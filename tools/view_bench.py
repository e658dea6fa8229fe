#!/usr/bin/env python
"""The scene view on the MI355X (gwd_cloud_view):

    python tools/view_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

  view            the map section 29's bench builds - the cloud predict_frames(intrinsics=, poses=) returned at stride 1, merged at voxel
                  0.05 and 0.02 - extracted and seen from the frames' own poses at frame size: the time of each of the three launches
                  from the profiler's kernel records, at footprint 0 (one pixel per voxel) and at footprint = voxel; device events over
                  back-to-back cloud_view calls; device-to-device copies of the four planes' bytes and of the z-buffer's bytes in the
                  same run, the floors of resolve and clear; the splat launch's covered pixels per second;
  near            the same extraction at a footprint of 100 m: every splat at the cap of max_splat = 32 pixels, the wave-cooperative
                  path, same-pixel atomics - the counterpart of section 29's contended row;
  arms            predict_frames(intrinsics=, poses=) of a session with cloud= and scene= (the launches of the parent commit) and with
                  scene_view= as well, alternated in one process;
  host            the route it replaces: extract().cpu(), a numpy projection, np.minimum.at over 64-bit keys (host clock around it, the
                  copy included; voxel 0.05, footprint 0).
Prints one JSON line and writes it to profiles/view_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("view_clear_kernel", "view_splat_kernel", "view_resolve_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("view_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from torch.profiler import ProfilerActivity, profile

    from gw_depth_amd import Config, build_model, hip, ops
    from gw_depth_amd.cloud import SceneMap
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.synth import det_fill_
    assert not getattr(hip.library(), "is_fake", False)
    B, fh, fw, steps = args.frames, args.height, args.width, args.steps

    def event_ms(fn, reps=10, windows=5):
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
        return {"ms": round(statistics.median(times), 5), "ms_min": round(min(times), 5), "ms_max": round(max(times), 5), "windows": windows}

    def kernel_ms(fn, names, reps=5):
        """ms per launch of the named kernels from the profiler's kernel records; None where this host has no tracer."""
        fn()
        torch.cuda.synchronize()
        found = {}
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            for e in prof.key_averages():
                for k in names:
                    if k in e.key:
                        found[k] = round(e.device_time_total / max(e.count, 1) / 1e3, 5)
        except Exception:
            pass
        return {k: found.get(k) for k in names}

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    kw = dict(compute_dtype=torch.bfloat16, graph=True, line_nms=0.01, regions=True, line_profiles=True)
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(B):
        low = torch.rand(1, 3, 9, 16, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(fh, fw), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    cam = torch.tensor([(0.9 * fw, 0.9 * fw, fw / 2.0, fh / 2.0)] * B, dtype=torch.float64)
    # section 29's camera: walking sideways, 5 cm and one degree per frame
    poses = []
    for b in range(B):
        a = np.deg2rad(1.0 * b)
        poses.append([[np.cos(a), 0.0, np.sin(a), 0.05 * b], [0.0, 1.0, 0.0, 0.0], [-np.sin(a), 0.0, np.cos(a), 0.0]])
    poses = torch.tensor(poses, dtype=torch.float64)

    out = {"tool": "view_bench", "frames": B, "frame_height": fh, "frame_width": fw, "device": torch.cuda.get_device_name(0), "view": {}}
    sess = InferenceSession(model, cloud=True, **kw)
    res = sess.predict_frames(frames, intrinsics=cam, poses=poses)
    cloud, offsets = res["cloud"].clone(), res["cloud_offsets"].clone()
    del sess, res
    torch.cuda.synchronize()
    d_cam, d_poses = cam.cuda(), poses.cuda()
    d_sizes = torch.tensor([(fh, fw)] * B, dtype=torch.int32).cuda()
    pixels = B * fh * fw

    def measure(ext, **options):
        view = lambda: ops.cloud_view(ext["cloud"], ext["cloud_offsets"], d_cam, d_sizes, poses=d_poses, plane=(fh, fw), **options)
        ks = kernel_ms(view, KERNELS)
        got = view()
        covered = int((got["view_index"] >= 0).sum())
        call = event_ms(view)
        del got
        return {"options": options, "kernel_ms": ks, "view_ms": None if any(v is None for v in ks.values()) else round(sum(ks.values()), 5),
                "cloud_view_call": call, "covered_pixels": covered, "covered_share": round(covered / pixels, 4)}

    planes = [torch.empty(pixels * n, dtype=torch.uint8, device="cuda") for n in (4, 4, 1, 3)]
    planes_dst = [torch.empty_like(p) for p in planes]
    zbuf, zbuf_dst = torch.empty(pixels, dtype=torch.int64, device="cuda"), torch.empty(pixels, dtype=torch.int64, device="cuda")

    def copy_planes():
        for d, s in zip(planes_dst, planes):
            d.copy_(s)

    out["floors"] = {"planes_bytes": 12 * pixels, "zbuffer_bytes": 8 * pixels, "copy_planes": event_ms(copy_planes),
                     "copy_zbuffer": event_ms(lambda: zbuf_dst.copy_(zbuf)),
                     "note": "torch copy_ device to device, read + write: resolve reads the z-buffer and writes the planes (20 bytes per pixel "
                             "+ one 16-byte record load per covered pixel), clear only writes the z-buffer"}
    del planes, planes_dst, zbuf, zbuf_dst
    extractions = {}
    for voxel in (0.05, 0.02):
        m = SceneMap(voxel, int(cloud.shape[0])).integrate(cloud, offsets)
        ext = m.extract()
        st = m.check()
        extractions[voxel] = ext
        entry = {"voxels": st["count"], "rows": int(ext["cloud"].shape[0]), "extract_call": event_ms(m.extract),
                 "footprint_0": measure(ext, footprint=0.0), "footprint_voxel": measure(ext, footprint=voxel)}
        for k in ("footprint_0", "footprint_voxel"):
            ks, n = entry[k]["kernel_ms"]["view_splat_kernel"], st["count"] * B
            entry[k]["splat_rows_per_us"] = None if not ks else round(n / ks / 1e3, 1)
        out["view"]["v%s" % voxel] = entry
        del m
    out["near"] = measure(extractions[0.05], footprint=100.0, max_splat=32)
    out["near"]["voxels"] = out["view"]["v0.05"]["voxels"]
    out["view"]["note"] = ("kernel_ms: per launch, from the profiler; the extraction has as many rows as the cloud (capacity), the splat grid is "
                           "sized by it and the tiles behind the total return at once; cloud_view_call: device events over 10 back-to-back "
                           "calls, allocation of the planes and the z-buffer and launch gaps included; splat_rows_per_us: voxels x views over "
                           "the splat launch; near: footprint 100 m, every splat 32 x 32 pixels")

    max_voxels = int(cloud.shape[0])
    mapped = InferenceSession(model, cloud=True, scene=dict(voxel=0.05, max_voxels=max_voxels), **kw)
    viewed = InferenceSession(model, cloud=True, scene=dict(voxel=0.05, max_voxels=max_voxels), scene_view=True, **kw)
    calls = {"predict_frames_cloud_scene": lambda: mapped.predict_frames(frames, intrinsics=cam, poses=poses),
             "predict_frames_cloud_scene_view": lambda: viewed.predict_frames(frames, intrinsics=cam, poses=poses)}
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
    seen = calls["predict_frames_cloud_scene_view"]()
    out["arms"]["scene_view_covered_share"] = round(int((seen["scene_index"] >= 0).sum()) / pixels, 4)
    out["arms"]["note"] = ("both with line_nms=0.01, regions=True, line_profiles=True, cloud=True (stride 1), scene at voxel 0.05, intrinsics and "
                           "poses; the scene_view arm also extracts the map and views it from the call's cameras (footprint = voxel, max_splat "
                           "32) before integrating")
    del mapped, viewed, seen

    def host_route(ext):
        """What a view costs without the kernels: the extraction to the host, a numpy projection, np.minimum.at over the keys."""
        n = int(ext["cloud_offsets"][-1])
        rec = ext["cloud"][:n].cpu().numpy()
        xyz = rec[:, :12].copy().view(np.float32).astype(np.float64)
        zb = np.full((B, fh * fw), np.iinfo(np.uint64).max, dtype=np.uint64)
        rows = np.arange(n, dtype=np.uint64)
        for b in range(B):
            M = poses[b].numpy()
            p = (xyz - M[:, 3]) @ M[:, :3]
            Z = p[:, 2]
            with np.errstate(all="ignore"):
                x = np.ceil(cam[b, 0].item() * p[:, 0] / Z + cam[b, 2].item() - 0.5)
                y = np.ceil(cam[b, 1].item() * p[:, 1] / Z + cam[b, 3].item() - 0.5)
            ok = (Z >= 1e-3) & (Z <= 10.0) & (x >= 0) & (x < fw) & (y >= 0) & (y < fh)
            key = Z[ok].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32) | rows[ok]
            np.minimum.at(zb[b], (y[ok] * fw + x[ok]).astype(np.int64), key)
        return zb

    host = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(extractions[0.05])
        host.append((time.perf_counter() - t0) * 1e3)
    dev = out["view"]["v0.05"]["footprint_0"]["view_ms"]
    out["host"] = {"ms_per_call": round(statistics.median(host), 1), "ms_min": round(min(host), 1), "ms_max": round(max(host), 1), "windows": len(host),
                   "over_device_view": None if not dev else round(statistics.median(host) / dev, 1),
                   "note": "voxel 0.05, footprint 0: the kept rows of the extraction .cpu(), R^T (p - t) and the projection in numpy, np.minimum.at "
                           "over 64-bit keys per view; the keys only, no planes"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

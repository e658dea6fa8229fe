#!/usr/bin/env python
"""The scene map on the MI355X (gwd_scene_*):

    python tools/scene_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

  map             the cloud predict_frames(intrinsics=, poses=) returned, at stride 1 and stride 2, merged at voxel 0.02 and 0.05 into
                  a map of as many voxels as the cloud has rows: the time of every launch from the profiler's kernel records, for the
                  FIRST sight of the cloud (reset + integrate: every voxel is claimed and ranked) and for a REVISIT (the same cloud
                  again: no births), and of extract; device events over back-to-back integrate / extract calls; a device-to-device
                  copy of the cloud's bytes in the same run as the stream yardstick, and the add launch's nominal atomics per second
                  (eleven per point, before the runs of one voxel inside a wave are merged);
  contended       the same stride-1 cloud at voxel 100 m: every point in a handful of voxels, same-address atomics;
  arms            predict_frames(intrinsics=, poses=) of a session with cloud= (the launches of the parent commit) and with cloud= and
                  scene=, alternated in one process;
  host            the route it replaces: cloud.cpu(), keys from quantised positions, np.unique, np.add.at for the sums (host clock
                  around it, the copy included; voxel 0.05).
Prints one JSON line and writes it to profiles/scene_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("scene_reset_kernel", "scene_claim_kernel", "scene_count_kernel", "scene_scan_kernel", "scene_rank_kernel", "scene_add_kernel",
           "scene_keep_kernel", "scene_keep_scan_kernel", "scene_emit_kernel")
INTEGRATE = KERNELS[1:6]
EXTRACT = KERNELS[6:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("scene_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from torch.profiler import ProfilerActivity, profile

    from gw_depth_amd import Config, build_model, hip
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

    total_of = lambda ks: None if any(v is None for v in ks.values()) else round(sum(ks.values()), 5)

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
    # a camera walking sideways, 5 cm and one degree per frame: successive frames see mostly the same surfaces
    poses = []
    for b in range(B):
        a = np.deg2rad(1.0 * b)
        poses.append([[np.cos(a), 0.0, np.sin(a), 0.05 * b], [0.0, 1.0, 0.0, 0.0], [-np.sin(a), 0.0, np.cos(a), 0.0]])
    poses = torch.tensor(poses, dtype=torch.float64)

    out = {"tool": "scene_bench", "frames": B, "frame_height": fh, "frame_width": fw, "device": torch.cuda.get_device_name(0), "map": {}}
    clouds = {}
    for stride in (1, 2):
        sess = InferenceSession(model, cloud=dict(stride=stride), **kw)
        res = sess.predict_frames(frames, intrinsics=cam, poses=poses)
        clouds[stride] = (res["cloud"].clone(), res["cloud_offsets"].clone())
        del sess, res
    torch.cuda.synchronize()

    def measure(cloud, offsets, voxel):
        rows = int(cloud.shape[0])
        m = SceneMap(voxel, rows)
        first = lambda: m.reset().integrate(cloud, offsets)
        again = lambda: m.integrate(cloud, offsets)
        k_first = kernel_ms(first, KERNELS[:6])
        st = m.check()
        k_again = kernel_ms(again, INTEGRATE)
        k_extract = kernel_ms(m.extract, EXTRACT)
        src, dst = cloud.clone(), torch.empty_like(cloud)
        copy = event_ms(lambda: dst.copy_(src))
        call_again, call_extract = event_ms(again), event_ms(m.extract)
        add = k_again["scene_add_kernel"]
        # a point with normal and colour: 2 packed counts + 3 offsets + 3 normal + 3 colour sums = 11 integer adds of 8 bytes - nominal:
        # the rows of one voxel that lie next to each other in a wave are merged into one set of adds
        return {"rows": rows, "points": st["points"], "voxels": st["count"], "bytes_read": int(cloud.numel()),
                "first_kernel_ms": k_first, "first_integrate_ms": total_of({k: k_first[k] for k in INTEGRATE}),
                "revisit_kernel_ms": k_again, "revisit_integrate_ms": total_of(k_again), "extract_kernel_ms": k_extract,
                "extract_ms": total_of(k_extract), "integrate_call": call_again, "extract_call": call_extract, "copy": copy,
                "integrate_over_copy": None if total_of(k_again) is None else round(total_of(k_again) / copy["ms"], 2),
                "add_nominal_atomics_per_us": None if not add else round(11 * st["points"] / max(st["serial"], 1) / add / 1e3, 1),
                "add_nominal_atomic_gb_per_s": None if not add else round(88 * st["points"] / max(st["serial"], 1) / add / 1e6, 1)}

    for stride in (1, 2):
        for voxel in (0.02, 0.05):
            out["map"]["s%d-v%s" % (stride, voxel)] = measure(*clouds[stride], voxel)
    out["contended"] = measure(*clouds[1], 100.0)
    out["map"]["note"] = ("kernel_ms: per launch, from the profiler; first: reset + integrate of an empty map (every voxel claimed and ranked); "
                          "revisit: the same cloud again (no births); *_call: device events over 10 back-to-back calls, allocation and launch "
                          "gaps included; copy: torch copy_ of the cloud's bytes, device to device; add_nominal_atomics: 11 integer adds of 8 bytes "
                          "per point over the add launch, before the runs of one voxel inside a wave are merged into one set of adds; contended: voxel 100 m, all points in a handful of voxels")

    plain = InferenceSession(model, cloud=True, **kw)
    mapped = InferenceSession(model, cloud=True, scene=dict(voxel=0.05, max_voxels=int(clouds[1][0].shape[0])), **kw)
    calls = {"predict_frames_cloud": lambda: plain.predict_frames(frames, intrinsics=cam, poses=poses),
             "predict_frames_cloud_scene": lambda: mapped.predict_frames(frames, intrinsics=cam, poses=poses)}
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
    out["arms"]["scene_state"] = mapped.scene.check()
    out["arms"]["note"] = ("both with line_nms=0.01, regions=True, line_profiles=True, cloud=True (stride 1), intrinsics and poses; the scene arm "
                           "integrates every call's cloud into one map at voxel 0.05 (after the first call: revisits)")

    def host_route(cloud, offsets, voxel):
        """What merging costs without the kernels: the cloud to the host, quantised keys, np.unique, np.add.at."""
        rec = cloud.cpu().numpy()[:int(offsets[-1])]
        xyz = rec[:, :12].copy().view(np.float32).astype(np.float64)
        t = xyz / voxel
        i = np.floor(t)
        q = np.floor((t - i) * 65536.0).astype(np.int64)
        idx = i.astype(np.int64) + (1 << 20)
        key = idx[:, 0] | idx[:, 1] << 21 | idx[:, 2] << 42
        uniq, inverse = np.unique(key, return_inverse=True)
        n = np.bincount(inverse, minlength=len(uniq))
        sums = np.zeros((len(uniq), 9), dtype=np.int64)
        nrm = np.rint(rec[:, 12:24].copy().view(np.float32).astype(np.float64) * 32767.0).astype(np.int64)
        np.add.at(sums, inverse, np.concatenate([q, nrm, rec[:, 24:27].astype(np.int64)], axis=1))
        return n, sums

    out["host"] = {}
    for stride in (1, 2):
        host = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route(*clouds[stride], 0.05)
            host.append((time.perf_counter() - t0) * 1e3)
        dev = out["map"]["s%d-v0.05" % stride]
        both = None if dev["first_integrate_ms"] is None or dev["extract_ms"] is None else dev["first_integrate_ms"] + dev["extract_ms"]
        out["host"]["s%d-v0.05" % stride] = {"ms_per_call": round(statistics.median(host), 1), "ms_min": round(min(host), 1), "ms_max": round(max(host), 1),
                                             "windows": len(host), "over_device_first_integrate_plus_extract": None if not both else round(statistics.median(host) / both, 1)}
    out["host"]["note"] = "cloud.cpu(), keys from quantised positions, np.unique, np.bincount and one np.add.at over nine sums; no birth order, no records"
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

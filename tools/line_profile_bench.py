"""Line profiles on the device (csrc/lineprofile.hip) on 8 frames of 720 x 1280, in ONE process.

    python tools/line_profile_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

bf16 graph sessions (line_nms=0.01, regions=True) over the det_fill_ seed 0 weights, frames of smooth seeded colour noise.  Measured:
  call            ops.line_profiles on the labels / depth_mm / region_map that predict_frames returned, at 100 and at 1024 seeded
                  random lines per frame (both ends uniform in the frame): device events over back-to-back calls (allocation and
                  launch gaps included) and the kernel's own device time from torch.profiler's kernel records, with the samples
                  walked and the gathers issued at most (label, millimetres and rank in pass 1, the millimetres again in passes 2 and 3: 14
                  one- or two-byte reads, 23 bytes, per sample whose probes all lie in the frame);
  arms            predict_frames of a session without line_profiles= (the launches and keys of the parent commit) and with it,
                  alternated round-robin (a window = --steps calls between two device events, ending in a synchronise);
  host            the route before it on the same results: labels.cpu(), depth_mm.cpu(), region_map.cpu() and the numpy statement
                  (tests/line_profile_ref.py), at 100 lines per frame (host clock around it, the copies included).
Prints one JSON line and writes it to profiles/line_profile_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_profile_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("line_profile_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from torch.profiler import ProfilerActivity, profile

    from gw_depth_amd import Config, build_model, hip, ops
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.synth import det_fill_
    from tests import line_profile_ref as P
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
        """ms per launch of line_profile_kernel from the profiler's kernel records; None where this host has no tracer."""
        fn()
        torch.cuda.synchronize()
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            for e in prof.key_averages():
                if "line_profile_kernel" in e.key:
                    return round(e.device_time_total / max(e.count, 1) / 1e3, 5)
        except Exception:
            pass
        return None

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    kw = dict(compute_dtype=torch.bfloat16, graph=True, line_nms=0.01, regions=True)
    plain = InferenceSession(model, **kw)
    with_profiles = InferenceSession(model, line_profiles=True, **kw)
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(B):
        low = torch.rand(1, 3, 9, 16, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(fh, fw), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    res = with_profiles.predict_frames(frames)
    torch.cuda.synchronize()
    labels, mm, sizes, rmap = res["labels"], res["depth_mm"], res["sizes"], res["region_map"]
    out = {"tool": "line_profile_bench", "frames": B, "frame_height": fh, "frame_width": fw, "device": torch.cuda.get_device_name(0),
           "predicted": {"nms_count": res["nms_count"].tolist(), "rows": int(res["nms_lines"].shape[1]),
                         "samples": int(res["profile_counts"][..., 0].sum()), "region_count": res["region_count"].tolist()},
           "call": {}}

    rng = np.random.default_rng(2)
    operands = {}
    for C in (100, 1024):
        lines = torch.from_numpy(rng.uniform(0.0, 1.0, (B, C, 4)) * np.array([fw, fh, fw, fh])).cuda()
        count = torch.full((B,), C, dtype=torch.int32, device="cuda")
        operands[C] = (lines, count)
        fn = lambda: ops.line_profiles(lines, count, labels, mm, sizes, region_map=rmap)
        samples = int(fn()["profile_counts"][..., 0].sum())
        out["call"][str(C)] = {"lines": B * C, "samples": samples, "gathers": 14 * samples, "gather_bytes": 23 * samples, "call_ms": round(event_ms(fn), 5),
                               "kernel_ms": kernel_ms(fn)}
    out["call"]["note"] = "call_ms: device events over 20 back-to-back ops.line_profiles calls, allocation and launch gaps included"

    calls = {"predict_frames": lambda: plain.predict_frames(frames), "predict_frames_profiles": lambda: with_profiles.predict_frames(frames)}
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
    out["arms"]["note"] = "predict_frames: a session without line_profiles= issues the parent commit's launches; both with line_nms=0.01, regions=True"

    lines, count = operands[100]

    def host_route():
        return P.line_profiles(lines.cpu().numpy(), count.cpu().numpy(), labels.cpu().numpy(), mm.cpu().numpy(), sizes.cpu().numpy(),
                               region_map=rmap.cpu().numpy())

    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    out["host"] = {"lines": B * 100, "ms_per_call": round(statistics.median(host), 3), "ms_min": round(min(host), 3), "ms_max": round(max(host), 3),
                   "windows": len(host), "note": "labels.cpu() + depth_mm.cpu() + region_map.cpu() + the numpy statement, 100 lines per frame"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

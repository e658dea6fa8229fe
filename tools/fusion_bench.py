"""Sensor depth fusion on the device (csrc/fusion.hip) on 8 frames of 720 x 1280, in ONE process.

    python tools/fusion_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

bf16 graph sessions over the det_fill_ seed 0 weights, frames of smooth seeded colour noise.  The sensor plane is synthetic, made from
the session's own output: the network's millimetres where there is no glass, 1.5 times as far behind the panes, 5 % of the pixels
within 6 of the glass at twice the depth, 3 % holes.  What is measured:
  stream          a device-to-device copy of 256 MiB, read + written bytes over its device time: the box's stream rate in this run;
  kernels         device time of every launch of ops.sensor_fusion on what predict_frames returned (torch.profiler's kernel records,
                  mean over the calls), the bytes the algorithm has to move (`traffic` below) and that as a fraction of the stream
                  rate; the whole operation also by device events;
  arms            predict_frames of a session with regions= and of one with regions= and fusion= (the sensor plane already on the
                  device), alternated round-robin (a window = --steps calls between two device events, ending in a synchronise),
                  and the route before it on the same results: four .cpu() copies, scipy.ndimage minimum / maximum filters,
                  numpy.linalg.lstsq per region (two fits) and the fused plane in numpy (host clock around it, the copies included).
Prints one JSON line and writes it to profiles/fusion_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("fusion_row_kernel", "fusion_col_kernel", "fusion_scale_kernel") + \
    tuple("fusion_%s_kernel<%d>" % (k, m) for m in range(4) for k in ("moments", "solve")) + ("fusion_depth_kernel<4>", "fusion_depth_kernel<1>")


def traffic(npix):
    """Bytes each streaming launch has to move, from the shapes alone (the halo rows the column pass re-reads are not counted).
    row: labels 1 + region_map 1 in, the row byte out; col: the row byte, labels 1, sensor 2, depth_mm 2 in, the ring out;
    moments: ring 1 + sensor 2; depth: labels 1, region_map 1, sensor 2, depth 4 in, fp32 4 + uint16 2 + source 1 out."""
    need = {"fusion_row_kernel": 3 * npix, "fusion_col_kernel": 7 * npix, "fusion_depth_kernel<4>": 15 * npix, "fusion_depth_kernel<1>": 15 * npix}
    need.update({"fusion_moments_kernel<%d>" % m: 3 * npix for m in range(4)})
    return need


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from scipy import ndimage
    if not torch.cuda.is_available():
        sys.exit("fusion_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from torch.profiler import ProfilerActivity, profile

    from gw_depth_amd import Config, build_model, hip, ops
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.synth import det_fill_
    assert not getattr(hip.library(), "is_fake", False)
    B, fh, fw, steps = args.frames, args.height, args.width, args.steps
    npix = B * fh * fw

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
        """{kernel: ms per launch} from the profiler's kernel records; {} where this host has no tracer."""
        fn()
        torch.cuda.synchronize()
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            out = {}
            for e in prof.key_averages():
                for k in KERNELS:
                    base, _, variant = k.partition("<")
                    if base in e.key and (not variant or "<" + variant in e.key):
                        out[k] = round(e.device_time_total / max(e.count, 1) / 1e3, 5)
            return out
        except Exception as exc:                                # no tracer: say so, keep the event timings
            return {"error": str(exc)}

    # ---- the box's stream rate in this run
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    copy_ms = event_ms(lambda: dst.copy_(src))
    stream = 2 * src.numel() / (copy_ms * 1e-3)
    del src, dst

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    with_regions = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, regions=True)
    with_fusion = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, regions=True, fusion=True)
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(B):
        low = torch.rand(1, 3, 9, 16, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(fh, fw), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    res = with_regions.predict_frames(frames)
    torch.cuda.synchronize()

    # ---- the synthetic sensor plane, from the session's own output
    rng = np.random.default_rng(2)
    lab_np, mm_np = res["labels"].cpu().numpy(), res["depth_mm"].cpu().numpy().astype(np.float64)
    glass = lab_np == 1
    near = np.stack([ndimage.maximum_filter(m.astype(np.uint8), size=13, mode="constant") > 0 for m in glass]) & ~glass
    sensor_np = np.where(glass, 1.5 * mm_np, mm_np)
    sensor_np = np.where(near & (rng.random(glass.shape) < 0.05), 2.0 * sensor_np, sensor_np)
    sensor_np = np.where(rng.random(glass.shape) < 0.03, 0.0, sensor_np)
    sensor = torch.from_numpy(np.clip(np.rint(sensor_np), 0, 65535).astype(np.uint16)).cuda()
    operands = (sensor, res["labels"], res["depth"], res["depth_mm"], res["sizes"], res["region_map"], res["region_count"], res["regions"])
    full = lambda: ops.sensor_fusion(*operands)
    fused = full()
    torch.cuda.synchronize()
    source = fused["fused_source"]
    status = fused["fusion_planes"][:, :, 10]
    kept = [max(int(k), 0) for k in res["region_count"].tolist()]

    def report(times):
        need = traffic(npix)
        out = {}
        for k, ms in times.items():
            out[k] = {"ms": ms}
            if k in need and isinstance(ms, float) and ms > 0:
                out[k].update(bytes=need[k], bytes_per_s=round(need[k] / (ms * 1e-3), 1), of_stream=round(need[k] / (ms * 1e-3) / stream, 4))
        return out

    out = {"tool": "fusion_bench", "frames": B, "frame_height": fh, "frame_width": fw, "device": torch.cuda.get_device_name(0),
           "stream": {"copy_ms": round(copy_ms, 5), "bytes_per_s": round(stream, 1), "note": "256 MiB device-to-device copy, read + written"},
           "scene": {"glass_pixels": int(glass.sum()), "ring_pixels": int((fused["fusion_ring"] > 0).sum()), "region_count": res["region_count"].tolist(),
                     "planes_usable": int(sum(int((status[b, :k] == 0).sum()) for b, k in enumerate(kept))),
                     "planes_rejected": int(sum(int((status[b, :k] == 2).sum()) for b, k in enumerate(kept))),
                     "planes_unfitted": int(sum(int((status[b, :k] == 1).sum()) for b, k in enumerate(kept))),
                     "pixels_sensor": int((source == 1).sum()), "pixels_plane": int((source == 2).sum()), "pixels_network": int((source == 3).sum()),
                     "scale": [round(v, 6) for v in fused["fusion_scale"][:, 0].tolist()]},
           "kernels": report(kernel_ms(full))}
    out["sensor_fusion_ms"] = {"ms": round(event_ms(full), 5),
                               "note": "device events over 20 back-to-back ops.sensor_fusion calls, allocation and launch gaps included"}

    # ---- predict_frames without / with fusion, and the route before it
    def host_route():
        lab, rmap, sen, dep = res["labels"].cpu().numpy(), res["region_map"].cpu().numpy(), sensor.cpu().numpy(), res["depth"].cpu().numpy()
        counts = res["region_count"].cpu().numpy()
        outs = []
        ys, xs = np.mgrid[0:fh, 0:fw].astype(np.float64)
        for b in range(B):
            is_glass = lab[b] == 1
            valid = (sen[b] >= 1) & (sen[b] <= 10000)
            rank = np.where(rmap[b] > 0, rmap[b], 255).astype(np.uint8)
            best = ndimage.minimum_filter(rank, size=13, mode="constant", cval=255)
            gap = ndimage.maximum_filter(is_glass.astype(np.uint8), size=3, mode="constant") > 0
            ring = np.where(~is_glass & valid & ~gap & (best != 255), best, 0)
            fusedb = np.where(~is_glass & valid, sen[b] / 1000.0, dep[b].astype(np.float64))
            for r in range(max(int(counts[b]), 0)):
                yy, xx = np.nonzero(ring == r + 1)
                if len(xx) < 50:
                    continue
                w = 1000.0 / sen[b][yy, xx]
                A = np.stack([xx, yy, np.ones(len(xx))], 1).astype(np.float64)
                c, *_ = np.linalg.lstsq(A, w, rcond=None)
                e = w - A @ c
                keep = e * e <= (2.5 * np.sqrt(np.mean(e * e))) ** 2
                c, *_ = np.linalg.lstsq(A[keep], w[keep], rcond=None)
                sel = rmap[b] == r + 1
                den = c[0] * xs[sel] + c[1] * ys[sel] + c[2]
                fusedb[sel] = np.where(den > 0, np.clip(1.0 / np.where(den > 0, den, 1.0), 1e-3, 10.0), fusedb[sel])
            outs.append(fusedb.astype(np.float32))
        return outs

    calls = {"predict_frames_regions": lambda: with_regions.predict_frames(frames),
             "predict_frames_regions_fusion": lambda: with_fusion.predict_frames(frames, sensor_depth=sensor)}
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
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    out["arms"]["host_scipy_filters_lstsq"] = {"ms_per_call": round(statistics.median(host), 3), "ms_min": round(min(host), 3),
                                               "ms_max": round(max(host), 3), "windows": len(host),
                                               "note": "labels / region_map / sensor / depth .cpu() + scipy.ndimage filters + numpy.linalg.lstsq twice per region + the fused plane"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Glass regions on the device (csrc/regions.hip) on 8 frames of 720 x 1280, in ONE process.

    python tools/regions_bench.py [--frames 8] [--height 720] [--width 1280] [--steps N] [--warmup K] [--min-seconds 2]

bf16 graph sessions over the det_fill_ seed 0 weights, frames of smooth seeded colour noise.  What is measured:
  stream          a device-to-device copy of 256 MiB, read + written bytes over its device time: the box's stream rate in this run;
  kernels         device time of every launch of ops.glass_regions on the labels / depth_mm / depth that predict_frames returned
                  (torch.profiler's kernel records, median over the calls), the bytes the algorithm has to move (labels 1, parent
                  and area words 4, map 1, millimetres 2, depth 4 bytes per pixel: `traffic` below) and that as a fraction of the
                  stream rate; the three entry points also by device events;
  masks           the same kernels of gwd_glass_regions on masks that stress the merge (all glass, vertical comb joined in the last
                  row, one-pixel spiral, 4-connected checkerboard, thresholded smooth noise), 8 copies of 720 x 1280 each;
  arms            predict_frames of a session without and with regions=, alternated round-robin (a window = --steps calls between
                  two device events, ending in a synchronise), and the route before it on the same results: labels.cpu(),
                  scipy.ndimage.label and the numpy records per frame (host clock around it, the copy included).
Prints one JSON line and writes it to profiles/regions_bench.json; fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("cc_init_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_candidates_kernel", "cc_select_kernel", "cc_records_kernel",
           "cc_finish_kernel", "plane_moments_kernel<0>", "plane_solve_kernel<0>", "plane_moments_kernel<1>", "plane_solve_kernel<1>",
           "depth_planar_kernel")


def traffic(npix, nglass, nkept):
    """Bytes each launch has to move, from the shapes alone (neighbour re-reads and the parent words a union walks are not counted)."""
    return {"cc_init_kernel": 9 * npix, "cc_merge_kernel": npix + 4 * nglass, "cc_flatten_kernel": npix + 8 * nglass,
            "cc_candidates_kernel": 4 * npix, "cc_records_kernel": 5 * npix + 4 * nglass + 2 * nkept,
            "plane_moments_kernel<0>": 3 * npix, "plane_moments_kernel<1>": 3 * npix, "depth_planar_kernel": 13 * npix}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from scipy import ndimage
    if not torch.cuda.is_available():
        sys.exit("regions_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
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
    plain = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True)
    with_regions = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, regions=True)
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(B):
        low = torch.rand(1, 3, 9, 16, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(fh, fw), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    res = with_regions.predict_frames(frames)
    torch.cuda.synchronize()
    labels, mm, depth, sizes = res["labels"], res["depth_mm"], res["depth"], res["sizes"]
    nglass, nkept = int((labels == 1).sum()), int((res["region_map"] > 0).sum())

    def report(times, nglass, nkept):
        need = traffic(npix, nglass, nkept)
        out = {}
        for k, ms in times.items():
            out[k] = {"ms": ms}
            if k in need and isinstance(ms, float) and ms > 0:
                out[k].update(bytes=need[k], bytes_per_s=round(need[k] / (ms * 1e-3), 1), of_stream=round(need[k] / (ms * 1e-3) / stream, 4))
        return out

    full = lambda: ops.glass_regions(labels, mm, sizes, depth=depth)
    out = {"tool": "regions_bench", "frames": B, "frame_height": fh, "frame_width": fw, "device": torch.cuda.get_device_name(0),
           "stream": {"copy_ms": round(copy_ms, 5), "bytes_per_s": round(stream, 1), "note": "256 MiB device-to-device copy, read + written"},
           "predicted": {"glass_pixels": nglass, "kept_pixels": nkept, "region_total": res["region_total"].tolist(),
                         "region_count": res["region_count"].tolist()},
           "kernels": report(kernel_ms(full), nglass, nkept)}
    entry = {"regions_only": lambda: ops.glass_regions(labels, mm, sizes, planes=False, planar=False),
               "regions_planes": lambda: ops.glass_regions(labels, mm, sizes, planar=False), "regions_planes_planar": full}
    out["entry_points_ms"] = {k: round(event_ms(f), 5) for k, f in entry.items()}
    out["entry_points_ms"]["note"] = "device events over 20 back-to-back ops.glass_regions calls, allocation and launch gaps included"

    # ---- masks that stress the merge
    yy, xx = np.mgrid[0:fh, 0:fw]
    comb = (xx % 2 == 0) | (yy == fh - 1)
    spiral = np.zeros((fh, fw), bool)
    t, l, b_, r = 0, 0, fh - 1, fw - 1
    while r - l >= 4 and b_ - t >= 4:                            # rectangular windings two pixels apart, each joined to the next
        spiral[t, l:r + 1] = spiral[b_, l:r + 1] = True
        spiral[t:b_ + 1, l] = spiral[t:b_ + 1, r] = True
        spiral[t + 1, l] = False
        spiral[t + 2, l:l + 3] = True
        t, l, b_, r = t + 2, l + 2, b_ - 2, r - 2
    from scipy.ndimage import gaussian_filter
    noise = gaussian_filter(np.random.default_rng(0).random((fh, fw)), sigma=3.0)
    noise = (noise - noise.min()) / (noise.max() - noise.min()) > 0.55
    masks = {"full": (np.ones((fh, fw), bool), 8), "comb": (comb, 8), "spiral": (spiral, 8), "checkerboard4": ((yy + xx) % 2 == 0, 4),
             "noise": (noise, 8)}
    out["masks"] = {}
    for name, (m, conn) in masks.items():
        lab = torch.from_numpy(np.broadcast_to(m.astype(np.uint8), (B, fh, fw)).copy()).cuda()
        fn = lambda: ops.glass_regions(lab, mm, sizes, connectivity=conn, planes=False, planar=False, max_candidates=1 << 20)
        r_ = fn()
        ng, nk = int(m.sum()) * B, int((r_["region_map"] > 0).sum())
        out["masks"][name] = {"connectivity": conn, "glass_pixels": ng, "region_total": int(r_["region_total"][0]),
                              "call_ms": round(event_ms(fn, reps=10, windows=3), 5), "kernels": report(kernel_ms(fn, reps=5), ng, nk)}

    # ---- predict_frames without / with regions, and the route before it
    def host_route():
        lab_np = labels.cpu().numpy()
        mm_np = mm.cpu().numpy()
        recs = []
        for b in range(B):
            comp, n = ndimage.label(lab_np[b] == 1, structure=np.ones((3, 3), bool))
            flat = comp.ravel()
            area = np.bincount(flat, minlength=n + 1)
            keep = np.argsort(-area[1:], kind="stable")[:32] + 1
            keep = keep[area[keep] >= 100]
            boxes = ndimage.find_objects(comp)
            ys, xs = np.divmod(np.arange(flat.size), fw)
            sx, sy = np.bincount(flat, xs, n + 1), np.bincount(flat, ys, n + 1)
            smm = np.bincount(flat, mm_np[b].ravel(), n + 1)
            recs.append([(area[k], boxes[k - 1], sx[k], sy[k], smm[k]) for k in keep])
        return recs

    calls = {"predict_frames": lambda: plain.predict_frames(frames), "predict_frames_regions": lambda: with_regions.predict_frames(frames)}
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
    out["arms"]["host_scipy_label_records"] = {"ms_per_call": round(statistics.median(host), 3), "ms_min": round(min(host), 3),
                                               "ms_max": round(max(host), 3), "windows": len(host),
                                               "note": "labels.cpu() + depth_mm.cpu() + scipy.ndimage.label + numpy records, no planes"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

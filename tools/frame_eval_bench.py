"""Scoring predict_frames results at frame size: one FrameMetrics.update (gwd_eval_frames, one launch) against the route a user had
before it, and evaluate_frames end to end.  Prints ONE JSON line and writes it to profiles/frame_eval_bench.json.

    python tools/frame_eval_bench.py [--frames 8] [--height 720] [--width 1280] [--calls 50] [--windows 7] [--samples 16]

8 frames of 720 x 1280 (predictions and ground truth drawn from a seed; the ground truth as a record holds it: 16-bit millimetres,
raw label bytes).  Arms, alternated round-robin in ONE process, every arm warmed up first; a window is `calls` back-to-back calls
between two device events; median and spread (max - min) over `windows` windows:
  update_bins0 / update_bins8   FrameMetrics.update with no depth bins and with eight (one / five grid slices: the bins re-read the
                                8 bytes per pixel, two bins per slice);
  update_bins0_int32            the same with the int32 planes FrameStore.frames() returns (10 bytes per pixel);
  dense_route                   the same eight frames through what existed before: GT to fp32 metres and int64 classes, one-hot
                                logits fabricated from the labels, DenseMetrics.update (no regions, no per-image sums).
Bytes per call are computed from the shapes (what the launch has to read); the implied rate stands beside the box's own stream rate,
taken by running tools/ubench/streamcopy (build: hipcc -O3 --offload-arch=gfx950 tools/ubench/streamcopy.hip -o
tools/ubench/streamcopy) when the binary is there, "not measured" otherwise.
End to end: a synthetic data set of --samples frames of the same size (tools/make_synth_dataset.py) in a device-resident FrameStore,
bf16 graph session with det_fill_ weights: frames per second of predict_frames alone and of evaluate_frames, ensemble off and on,
wall clock around a pass that ends in a synchronise, best and median of three passes after a warm-up pass.
Fails without a GPU."""
import argparse
import importlib.util
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EDGES8 = (0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0)


def stream_rate():
    exe = os.path.join(ROOT, "tools", "ubench", "streamcopy")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120).stdout
    rates = [float(m) for m in re.findall(r"= ([0-9.]+) TB/s", out)]
    return max(rates) if rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=16, help="frames of the end-to-end data set (0: skip that part)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_eval_bench.json"))
    args = ap.parse_args()
    B, H, W = args.frames, args.height, args.width

    from gw_depth_amd import decode
    tmp = pool = index = None
    if args.samples:                                        # the decode pool has to be up before the GPU is initialised
        spec = importlib.util.spec_from_file_location("make_synth_dataset", os.path.join(ROOT, "tools", "make_synth_dataset.py"))
        synth = importlib.util.module_from_spec(spec)
        sys.modules["make_synth_dataset"] = synth            # its worker processes pickle functions by this name
        spec.loader.exec_module(synth)
        tmp = tempfile.TemporaryDirectory(prefix="gwd_frame_eval_bench_")
        synth.write_dataset(tmp.name, args.samples, [(H, W)], seed=0, jobs=min(16, len(os.sched_getaffinity(0))))
        index = decode.GlassRGBDIndex(**synth.index_args(tmp.name))
        pool = decode.DecodePool(index)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        if pool is not None:
            pool.close()
        raise SystemExit("frame_eval_bench needs the GPU: a CPU run gives no device time")
    from gw_depth_amd.evaluate import DenseMetrics, FrameMetrics, evaluate_frames
    dev = torch.device("cuda")
    res = {"tool": "frame_eval_bench", "device": torch.cuda.get_device_name(0), "frames": B, "size": [H, W],
           "calls_per_window": args.calls, "windows": args.windows}
    rate = stream_rate()
    res["box_stream_TBps_read_plus_write"] = rate if rate is not None else "not measured"

    rng = np.random.default_rng(0)
    mm = rng.integers(0, 11000, size=(B, H, W)).astype(np.uint16)
    depth = torch.from_numpy((mm / 1000.0 * rng.uniform(0.7, 1.4, size=(B, H, W))).astype(np.float32)).to(dev)
    labels = torch.from_numpy((rng.random((B, H, W)) < 0.3).astype(np.uint8)).to(dev)
    raw = torch.from_numpy(((rng.random((B, H, W)) < 0.3) * 255).astype(np.uint8)).to(dev)
    mm16 = torch.from_numpy(mm.view(np.int16)).to(dev).view(torch.uint16)
    mm32 = torch.from_numpy(mm.astype(np.int32)).to(dev)
    result = {"depth": depth, "labels": labels}
    gt16 = [(mm16[b], raw[b]) for b in range(B)]
    gt32 = [(mm32[b], raw[b]) for b in range(B)]
    cap = B * args.calls
    fm0, fm8, fm0w = (FrameMetrics(dev, depth_bins=e, capacity_images=cap) for e in (None, EDGES8, None))
    dm = DenseMetrics(dev)

    def dense_route(into=dm):
        gt = mm32.to(torch.float32) / 1000.0
        seg_gt = (raw > 0).to(torch.int64)
        logits = torch.nn.functional.one_hot(labels.to(torch.int64), 2).permute(0, 3, 1, 2).to(torch.float32)
        into.update(depth.unsqueeze(1), gt.unsqueeze(1), logits, seg_gt.unsqueeze(1))

    def upd(fm, gt):
        def f():
            if fm.images_seen + B > fm.capacity:
                fm.reset()
            fm.update(result, gt)
        return f

    npix = B * H * W
    arms = {"update_bins0": (upd(fm0, gt16), npix * 8 * 1), "update_bins8": (upd(fm8, gt16), npix * 8 * 5),
            "update_bins0_int32": (upd(fm0w, gt32), npix * 10 * 1), "dense_route": (dense_route, None)}
    for f, _ in arms.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.windows):
        for k, (f, _) in arms.items():
            for fm in (fm0, fm8, fm0w):
                fm.reset()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                f()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / args.calls)
    res["arms"] = {}
    for k, (_, nbytes) in arms.items():
        med = statistics.median(times[k])
        a = {"ms_median": round(med, 5), "ms_min": round(min(times[k]), 5), "ms_max": round(max(times[k]), 5),
             "spread_ms": round(max(times[k]) - min(times[k]), 5)}
        if nbytes:
            a["bytes_read_per_call"] = nbytes
            a["implied_TBps_read"] = round(nbytes / (med * 1e-3) / 1e12, 4)
        res["arms"][k] = a
    res["dense_route_over_update_bins0"] = round(res["arms"]["dense_route"]["ms_median"] / res["arms"]["update_bins0"]["ms_median"], 3)
    # the two routes count the same pixels
    fm0.reset()
    fm0.update(result, gt16)
    check, dm2 = fm0.compute(), DenseMetrics(dev)
    dense_route(dm2)
    dense = dm2.compute()
    res["rms_update_vs_dense_route"] = [check["rms"], dense["rms"]]
    res["mean_iu_update_vs_dense_route"] = [check["Mean IU"], dense["Mean IU"]]

    if args.samples:
        from gw_depth_amd import Config, build_model, dataset
        from gw_depth_amd.infer import InferenceSession
        from gw_depth_amd.synth import det_fill_
        cfg = Config(device="cuda", dropout=0.0)
        model, _, _ = build_model(cfg)
        model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
        model.cuda().eval()
        sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True)
        store = dataset.FrameStore.build(index, pool, device="cuda", where="device")
        n = len(store)

        def predict_only(ensemble, batch):
            for at in range(0, n, batch):
                sess.predict_frames(store.record_rgb(range(at, min(at + batch, n))), ensemble=ensemble)

        def evaluate(ensemble, batch):
            evaluate_frames(sess, store, batch=batch, ensemble=ensemble, depth_bins=EDGES8)

        e2e = {}
        for name, f, ens in (("predict_frames", predict_only, False), ("evaluate_frames", evaluate, False),
                             ("predict_frames_ensemble", predict_only, True), ("evaluate_frames_ensemble", evaluate, True)):
            f(ens, 8)
            torch.cuda.synchronize()
            fps = []
            for _ in range(3):
                t = time.perf_counter()
                f(ens, 8)
                torch.cuda.synchronize()
                fps.append(n / (time.perf_counter() - t))
            e2e[name] = {"frames_per_s_best": round(max(fps), 2), "frames_per_s_median": round(statistics.median(fps), 2)}
        res["end_to_end"] = dict(e2e, samples=n, batch=8, session="bf16, graph, det_fill_ seed 0, size 1024 / max_size 1024")
        pool.close()
        tmp.cleanup()

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Inference throughput: the plain model.eval() forward against infer.InferenceSession, in ONE process.

    python tools/infer_bench.py --config c1|c5 [--steps N] [--warmup K] [--arms a,b,c] [--min-seconds 2] [--no-launch-count]

c1 = 1 x 480 x 640 (the reference evaluates at batch 1), c5 = 32 x 960 x 1280 (BASELINE's HBM-bound stress); bf16, synth_batch
inputs, weights det_fill_ seed 0.  Arms:
  a        the plain `model.eval(); model(NestedTensor(...))` forward under no_grad - the path without a session, the baseline;
  b, b_predict   session, graph=False, as __call__ and as predict();
  c, c_predict   session, graph=True, likewise.
The arms are ALTERNATED round-robin (each round starts one arm further on), one window of --steps calls each, until every arm has at least --min-seconds of timed
work and at least three windows, so that they share the machine's state.  A window is timed by device events and ends in a
synchronise; the host clock around the enqueue loop of the same window gives the host-side cost per call.  Per arm: median,
minimum and maximum of the windows' ms per call (the spread), images/s from the median.  Launches per call of arms a and b are
counted with torch.profiler AFTER all timing (a count, not a time).  Prints one JSON line; fails without a GPU.

Kernel tables: run under `rocprofv3 --kernel-trace --stats -- python tools/infer_bench.py --config c5 --arms b_predict
--min-seconds 0 --no-launch-count` in a run of its own (arm b's launches are plain ones).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {"c1": (1, 480, 640, 50), "c5": (32, 960, 1280, 2)}       # B, H, W, default calls per window
ALL_ARMS = ["a", "b", "b_predict", "c", "c_predict"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c1")
    ap.add_argument("--steps", type=int, default=0, help="calls per timed window (0: the config's default)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per arm before the first window")
    ap.add_argument("--arms", default="a,b,c", help="comma list of a, b, c (b and c include their _predict form) or full arm names")
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("infer_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from gw_depth_amd import Config, build_model, hip
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.model import NestedTensor
    from gw_depth_amd.synth import det_fill_, synth_batch

    assert not getattr(hip.library(), "is_fake", False)
    B, H, W, steps = CONFIGS[args.config]
    steps = args.steps or steps
    arms = []
    for a in args.arms.split(","):
        arms += [a, a + "_predict"] if a in ("b", "c") else [a]
    assert all(a in ALL_ARMS for a in arms), arms

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    model.compute_dtype = torch.bfloat16
    b = synth_batch(min(B, 4), H, W, seed=1)
    rep = B // min(B, 4)
    x = NestedTensor(b["images"].cuda().repeat(rep, 1, 1, 1), b["pad_mask"].cuda().repeat(rep, 1, 1))
    eager = InferenceSession(model, compute_dtype=torch.bfloat16, graph=False)
    graph = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True)

    def plain():
        with torch.no_grad():
            return model(x)
    calls = {"a": plain, "b": lambda: eager(x), "b_predict": lambda: eager.predict(x),
             "c": lambda: graph(x), "c_predict": lambda: graph.predict(x)}

    for a in arms:
        for _ in range(max(args.warmup, 1)):
            out = calls[a]()
        torch.cuda.synchronize()
    if any(a.startswith("c") for a in arms):
        assert all(v["captured"] for v in graph.graphs.values()), "capture was refused: %r" % dict(graph.graphs)

    windows = {a: [] for a in arms}
    host = {a: [] for a in arms}
    rounds = 0
    while any(len(windows[a]) < 3 or sum(windows[a]) * steps / 1e3 < args.min_seconds for a in arms):
        k = rounds % len(arms)                       # the round starts one arm further on each time: no arm always follows the same one
        rounds += 1
        for a in arms[k:] + arms[:k]:
            fn = calls[a]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            h0 = time.perf_counter()
            for _ in range(steps):
                fn()
            h1 = time.perf_counter()
            t1.record()
            t1.synchronize()
            windows[a].append(t0.elapsed_time(t1) / steps)
            host[a].append((h1 - h0) * 1e3 / steps)

    res = {"tool": "infer_bench", "config": args.config, "batch": B, "height": H, "width": W, "dtype": "bf16",
           "calls_per_window": steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "arms": {}}
    for a in arms:
        w = windows[a]
        med = statistics.median(w)
        res["arms"][a] = {"ms_per_call": round(med, 4), "ms_min": round(min(w), 4), "ms_max": round(max(w), 4),
                          "spread_ms": round(max(w) - min(w), 4), "windows": len(w), "images_per_s": round(B * 1e3 / med, 2),
                          "host_enqueue_ms_per_call": round(statistics.median(host[a]), 4)}
    if "a" in arms:
        for a in arms:
            if a != "a":
                res["arms"][a]["speedup_vs_a"] = round(res["arms"]["a"]["ms_per_call"] / res["arms"][a]["ms_per_call"], 4)
    out = plain()
    d, s = out["pred_depth"][-1], out["pred_seg"]
    res["dense_postprocess_bytes"] = B * H * W * (d.element_size() + 2 * s.element_size() + 4 + 2 + 1)    # read depth + 2 logits, write fp32 + uint16 + uint8

    if not args.no_launch_count:
        from torch.profiler import ProfilerActivity, profile
        for a in [k for k in ("a", "b", "b_predict") if k in arms]:
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                calls[a]()
                torch.cuda.synchronize()
            ev = list(prof.events())
            res["arms"][a]["launches_per_call"] = sum(1 for e in ev if "LaunchKernel" in e.name)
            res["arms"][a]["weight_prep_kernels_per_call"] = sum(1 for e in ev if "weight_prep" in e.name)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

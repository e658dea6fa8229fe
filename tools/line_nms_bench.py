"""Line NMS on the device: the kernel alone, and what it adds to a replayed predict(), in ONE process.

    python tools/line_nms_bench.py [--steps 50] [--warmup 3] [--min-seconds 2] [--out profiles/line_nms_bench.json]

kernel   device time of ops.line_nms alone (gwd_line_nms and its four output allocations) at B = 1 and B = 32, Q = 100, on the
         lines of tests/line_score_ref.random_case, in score order at 0.010 of the diagonal: windows of 200 back-to-back calls
         between device events, median of 7 windows and their spread.
predict  the replayed c1 predict (1 x 480 x 640, bf16, tools/infer_bench.py's model and input) of a session without line_nms - the
         yardstick, tools/infer_bench.py's arm c_predict - and of a session with line_nms=0.010, ALTERNATED round-robin as
         tools/infer_bench.py alternates its arms, one window of --steps calls each, until both have --min-seconds of timed work
         and three windows.  Median, minimum and maximum of the windows' ms per call.
Writes one JSON line to --out and prints it; fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def window(fn, calls):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls


def summary(w):
    return {"ms_per_call": round(statistics.median(w), 5), "ms_min": round(min(w), 5), "ms_max": round(max(w), 5),
            "spread_ms": round(max(w) - min(w), 5), "windows": len(w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="predict calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_nms_bench.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("line_nms_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from gw_depth_amd import Config, build_model, hip, ops
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.model import NestedTensor
    from gw_depth_amd.synth import det_fill_, synth_batch
    from tests.line_score_ref import random_case

    assert not getattr(hip.library(), "is_fake", False)
    res = {"tool": "line_nms_bench", "device": torch.cuda.get_device_name(0), "threshold": 0.010, "order": "score", "kernel": {}}
    for B in (1, 32):
        logits, lines, sizes, _, _ = random_case(B, 100, 0, seed=900 + B)
        logits, lines, sizes = (torch.from_numpy(a).cuda() for a in (logits, lines, sizes))
        order = ops.line_postprocess(logits, lines, sizes, 0.6)[2]
        fn = lambda: ops.line_nms(logits, lines, sizes, 0.010, order=order)
        for _ in range(10):
            kept = fn()[3]
        w = [window(fn, 200) for _ in range(7)]
        res["kernel"]["B%d_Q100" % B] = dict(summary(w), calls_per_window=200, kept_mean=round(float(kept.float().mean()), 2))

    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True)
    model, _, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda().eval()
    model.compute_dtype = torch.bfloat16
    b = synth_batch(1, 480, 640, seed=1)
    x = NestedTensor(b["images"].cuda(), b["pad_mask"].cuda())
    sessions = {"c_predict": InferenceSession(model, compute_dtype=torch.bfloat16, graph=True),
                "c_predict_line_nms": InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, line_nms=0.010)}
    arms = list(sessions)
    for a in arms:
        for _ in range(max(args.warmup, 1)):
            out = sessions[a].predict(x)
        torch.cuda.synchronize()
        assert all(v["captured"] for v in sessions[a].graphs.values()), "capture was refused: %r" % dict(sessions[a].graphs)
    res["kept_in_predict"] = int(out["nms_count"][0])
    windows = {a: [] for a in arms}
    rounds = 0
    while any(len(windows[a]) < 3 or sum(windows[a]) * args.steps / 1e3 < args.min_seconds for a in arms):
        k = rounds % len(arms)
        rounds += 1
        for a in arms[k:] + arms[:k]:
            windows[a].append(window(lambda: sessions[a].predict(x), args.steps))
    res["predict"] = {a: dict(summary(windows[a]), calls_per_window=args.steps) for a in arms}
    res["predict"]["added_ms"] = round(res["predict"]["c_predict_line_nms"]["ms_per_call"] - res["predict"]["c_predict"]["ms_per_call"], 5)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Device time of one LineMetrics.update (gwd_line_score, one launch) at B = 1 and B = 32, Q = 100, G = 16, beside the host time of the
NumPy restatement (tests/line_score_ref.py) on the same inputs.  Prints ONE JSON line (kept as profiles/linescore_bench.json).

Method: every shape is warmed up; a window is `calls` back-to-back updates into consecutive image slots between two device events,
so a window is device time of the launches including their gaps; 7 windows, median and spread (max - min) per update.  The host
figure is a wall clock around image_chain per image (it has no device work).  Needs the GPU: there is no fallback.

Usage: python tools/linescore_bench.py [--calls 500] [--windows 7] [--out profiles/linescore_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gw_depth_amd.evaluate import LineMetrics  # noqa: E402
from tests import line_score_ref as R  # noqa: E402

REFERENCE_BASELINE = {"ms_per_image_per_nms_threshold": [83, 130],
                      "provenance": "the reference's own postprocess() (evaluation/eval_post_online.py:44-91), pure Python, 100 queries of "
                                    "which 97-99 kept, 480 x 640, float32 and float64, on a development machine's CPU; quoted, not re-measured here"}
FORWARD_C1_MS = 6.25          # profiles/infer_bench.json: the replayed batch-1 480 x 640 bf16 forward


def device_arm(B, Q, G, calls, windows, warmup=20):
    logits, lines, sizes, gts, counts = R.random_case(B, Q, G, seed=900 + B)
    dev = torch.device("cuda")
    ops = [torch.from_numpy(a).to(dev) for a in (logits, lines, sizes, gts, counts)]
    lm = LineMetrics(dev, capacity_images=B * max(calls, warmup))
    for _ in range(warmup):
        lm.update(*ops)
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        lm.reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            lm.update(*ops)
        t1.record()
        torch.cuda.synchronize()
        per_call.append(t0.elapsed_time(t1) / calls)
    t = time.perf_counter()
    stats = lm.compute()
    close_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for b in range(min(B, 4)):
        R.image_chain(lines[b], sizes[b], gts[b, :counts[b]])
    host_ms = (time.perf_counter() - t) * 1e3 / min(B, 4)
    med = statistics.median(per_call)
    return {"B": B, "Q": Q, "G": G, "calls_per_window": calls, "windows": windows, "update_ms_median": round(med, 5),
            "update_ms_min": round(min(per_call), 5), "update_ms_max": round(max(per_call), 5),
            "spread_ms": round(max(per_call) - min(per_call), 5), "update_us_per_image": round(med * 1e3 / B, 3),
            "share_of_c1_forward": round(med / FORWARD_C1_MS, 5), "compute_ms_over_%d_images" % (B * calls): round(close_ms, 3),
            "host_restatement_ms_per_image_both_thresholds": round(host_ms, 3), "sAP10_nms0_010": stats["sAP10_nms0_010"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linescore_bench needs the GPU: a CPU run gives no device time")
    res = {"tool": "linescore_bench", "device": torch.cuda.get_device_name(0), "forward_c1_ms": FORWARD_C1_MS,
           "reference_baseline": REFERENCE_BASELINE,
           "arms": [device_arm(1, 100, 16, args.calls, args.windows), device_arm(32, 100, 16, args.calls, args.windows)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

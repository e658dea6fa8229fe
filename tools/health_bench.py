"""The guarded optimizer step: what it costs, in ONE process, against the unguarded step of the same TrainStep.

    python tools/health_bench.py [--steps 20] [--warmup 3] [--min-seconds 2] [--out profiles/health_bench.json]

optimizer  device time of optimizer_step() alone on the flat buffers of the full model (66 M elements, bf16 shadow), between device
           events: "sqnorm_adamw" (the zeroing of sq, gwd_sqnorm, two gwd_adamw_step), "stats_decide_guarded" (gwd_segment_stats of
           flat_g, gwd_health_decide, two gwd_adamw_step_guarded), and each with stats_every=1 (the extra passes); windows of 20
           back-to-back calls, alternated round-robin, median of 7 windows and their spread.  The gradient is the last step's.
step       ms per replayed step, 8 x 480 x 640 bf16, bench.py's model, weights and batch: guard="off" twice ("off_a", "off_b": the
           run-to-run spread of the yardstick is the difference of these two legs), guard="skip", guard="skip" with stats_every=1 and
           guard="off" with stats_every=1, ALTERNATED round-robin, one window of --steps steps each (flush() inside the window), until
           every leg has --min-seconds of timed work and three windows.  Median, minimum and maximum of the windows.
The legs are settings of ONE TrainStep (the guard and stats_every are read at every optimizer_step), so all of them replay the same
captured graph on the same buffers.  Writes one JSON line to --out and prints it; fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEGS = {"off_a": ("off", 0), "skip": ("skip", 0), "skip_stats1": ("skip", 1), "off_stats1": ("off", 1), "off_b": ("off", 0)}
OPT_LEGS = {"sqnorm_adamw": ("off", 0), "stats_decide_guarded": ("skip", 0), "sqnorm_adamw_stats1": ("off", 1),
            "stats_decide_guarded_stats1": ("skip", 1)}


def window(fn, calls, end=None):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        fn()
    if end is not None:
        end()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls


def summary(w):
    return {"ms": round(statistics.median(w), 5), "ms_min": round(min(w), 5), "ms_max": round(max(w), 5),
            "spread_ms": round(max(w) - min(w), 5), "windows": len(w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "health_bench.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("health_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from gw_depth_amd import Config, build_model, hip
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import det_fill_, synth_batch

    assert not getattr(hip.library(), "is_fake", False)
    cfg = Config(device="cuda", dropout=0.1, log_depth_error=True)
    model, crits, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda()
    crits[0].cuda()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=True, guard="skip", stats_every=1)
    b = synth_batch(args.batch, args.height, args.width, seed=1)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    batch["targets"] = [{k: v.cuda() for k, v in t.items()} for t in b["targets"]]
    torch.manual_seed(100)

    def setting(leg, table=LEGS):
        step.guard, step.stats_every = table[leg]

    for leg in LEGS:
        setting(leg)
        for _ in range(max(args.warmup, 1)):
            step(batch)
        step.flush()
    torch.cuda.synchronize()
    assert step._graphs and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
    setting("skip")
    h = step.health()
    assert h["skipped"] == 0, "a warm-up step was skipped: %r" % (h,)

    res = {"tool": "health_bench", "device": torch.cuda.get_device_name(0), "elements": step.total, "tensors": len(step.names),
           "chunks": int(step._health.chunks.shape[0]), "flat_buffer_mb": round(step.total * 4 / 1e6, 1),
           "shape": "%dx%dx%d bf16, replayed" % (args.batch, args.height, args.width)}

    # ---- the replayed step
    legs = list(LEGS)
    w = {n: [] for n in legs}
    rounds = 0
    while any(len(w[n]) < 3 or sum(w[n]) * args.steps / 1e3 < args.min_seconds for n in legs):
        k = rounds % len(legs)
        rounds += 1
        for n in legs[k:] + legs[:k]:
            setting(n)
            w[n].append(window(lambda: step(batch), args.steps, end=step.flush))
    st = res["step"] = {n: dict(summary(w[n]), steps_per_window=args.steps) for n in legs}
    off = 0.5 * (st["off_a"]["ms"] + st["off_b"]["ms"])
    st["off_ms"] = round(off, 5)
    st["off_leg_to_leg_ms"] = round(abs(st["off_a"]["ms"] - st["off_b"]["ms"]), 5)
    st["skip_added_ms"] = round(st["skip"]["ms"] - off, 5)
    st["skip_stats1_added_over_skip_ms"] = round(st["skip_stats1"]["ms"] - st["skip"]["ms"], 5)
    st["off_stats1_added_ms"] = round(st["off_stats1"]["ms"] - off, 5)
    setting("skip")
    h = step.health()
    res["health"] = {"applied": h["applied"], "skipped": h["skipped"], "attempts": step.step_count}
    st["one_pass_at_4p7_TBps_ms"] = round(step.total * 4 / 4.7e12 * 1e3, 5)       # profiles/r03_stream_copy.txt: 4.7 TB/s, read + write

    # ---- the optimizer part alone (last: 560 updates from one gradient leave the weights nowhere useful)
    names = list(OPT_LEGS)
    w = {n: [] for n in names}
    for r in range(7):
        k = r % len(names)
        for n in names[k:] + names[:k]:
            setting(n, OPT_LEGS)
            w[n].append(window(step.optimizer_step, 20, end=step.flush))
    res["optimizer"] = {n: dict(summary(w[n]), calls_per_window=20) for n in names}
    res["optimizer"]["guard_added_ms"] = round(res["optimizer"]["stats_decide_guarded"]["ms"] - res["optimizer"]["sqnorm_adamw"]["ms"], 5)

    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""The weight average fused into the AdamW pass: what it costs against the step without it and against the separate pass a user
would write, in ONE process, on the flat buffers of the full model.

    python tools/ema_bench.py [--rounds 60] [--calls 4] [--steps 10] [--no-step] [--out profiles/ema_bench.json]

optimizer  device time between device events of the optimizer part alone on a TrainStep's own buffers (66 M elements in two LR groups,
           bf16 shadow; the gradient is noise of size 1e-3):
             A  the zeroing of sq, gwd_sqnorm, gwd_adamw_step per group                         today's path (run as two legs, A_a and A_b)
             B  A, then flat_e.lerp_(flat_p, omd)                                               what a user does without the feature
             C  the zeroing of sq, gwd_sqnorm, gwd_adamw_step_ema per group                     the fused pass
           A_a, B, C and A_b ALTERNATE round-robin (the starting leg rotates), one window of --calls back-to-back calls per leg and
           round, --rounds rounds after a warm-up round; median, minimum, maximum and inter-quartile range of the windows of each leg.
           "A against itself" is |median A_a - median A_b|: the fusion counts as bought when B - C exceeds it ("done").
           C's rate is 38 bytes per element (p, g, m, v, ema read; p, m, v, ema and the shadow written) over its time, next to the
           box's own stream rate (tools/ubench/streamcopy when the binary is there, "not measured" otherwise).
step       ms per replayed step, 8 x 480 x 640 bf16, bench.py's model, weights and batch, with and without the average: legs off_a,
           ema, off_b of ONE TrainStep (optimizer_step reads flat_e at every call, the captured graph is the same), alternated, windows
           of --steps steps, at least three per leg.
Writes one JSON line to --out and prints it; fails without a GPU."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES_PER_ELEMENT = {"A": 30, "B": 42, "C": 38}


def stream_rate():
    exe = os.path.join(ROOT, "tools", "ubench", "streamcopy")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120).stdout
    rates = [float(m) for m in re.findall(r"= ([0-9.]+) TB/s", out)]
    return max(rates) if rates else None


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
    q = statistics.quantiles(w, n=4) if len(w) >= 4 else [min(w), statistics.median(w), max(w)]
    return {"ms": round(statistics.median(w), 5), "ms_min": round(min(w), 5), "ms_max": round(max(w), 5), "iqr_ms": round(q[2] - q[0], 5),
            "windows": len(w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--calls", type=int, default=4, help="back-to-back optimizer calls per window")
    ap.add_argument("--steps", type=int, default=10, help="train steps per timed window of the replayed step")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the replayed 8 x 480 x 640 step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    args = ap.parse_args()
    if args.rounds < 50:
        sys.exit("ema_bench: at least 50 rounds")

    import torch
    if not torch.cuda.is_available():
        sys.exit("ema_bench: needs the MI355X (no GPU found); a timing from anything else says nothing")
    from gw_depth_amd import Config, build_model, hip
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import det_fill_, synth_batch

    lib = hip.library()
    assert not getattr(lib, "is_fake", False)
    rate = stream_rate()
    cfg = Config(device="cuda", dropout=0.1, log_depth_error=True)
    model, crits, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda()
    crits[0].cuda()
    decay = 0.9998
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=True, ema_decay=decay)
    flat_e = step.flat_e
    res = {"tool": "ema_bench", "device": torch.cuda.get_device_name(0), "elements": step.total, "groups": [step.split, step.total - step.split],
           "flat_buffer_mb": round(step.total * 4 / 1e6, 1), "ema_decay": decay,
           "box_stream_TBps_read_plus_write": rate if rate is not None else "not measured"}

    # ---- the replayed step first: its weights are still the seeded ones
    if not args.no_step:
        b = synth_batch(8, 480, 640, seed=1)
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        batch["targets"] = [{k: v.cuda() for k, v in t.items()} for t in b["targets"]]
        torch.manual_seed(100)
        legs = {"off_a": None, "ema": flat_e, "off_b": None}

        def setting(leg):
            step.flat_e = legs[leg]

        for leg in legs:
            setting(leg)
            for _ in range(max(args.warmup, 1)):
                step(batch)
            step.flush()
        torch.cuda.synchronize()
        assert step._graphs and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
        names = list(legs)
        w = {n: [] for n in names}
        for r in range(3):
            k = r % len(names)
            for n in names[k:] + names[:k]:
                setting(n)
                w[n].append(window(lambda: step(batch), args.steps, end=step.flush))
        st = res["step"] = {n: dict(summary(w[n]), steps_per_window=args.steps) for n in names}
        st["shape"] = "8x480x640 bf16, replayed"
        off = 0.5 * (st["off_a"]["ms"] + st["off_b"]["ms"])
        st["off_ms"], st["off_leg_to_leg_ms"] = round(off, 5), round(abs(st["off_a"]["ms"] - st["off_b"]["ms"]), 5)
        st["ema_added_ms"] = round(st["ema"]["ms"] - off, 5)
        step.flat_e = flat_e

    # ---- the optimizer part alone
    gen = torch.Generator(device="cuda").manual_seed(7)
    step.flat_g.copy_(torch.randn(step.total, device="cuda", generator=gen) * 1e-3)
    groups = [(lo, hi, lr) for lo, hi, lr in ((0, step.split, cfg.lr), (step.split, step.total, cfg.lr_backbone)) if hi > lo]
    P, G, M, V, S, E = step.flat_p, step.flat_g, step.flat_m, step.flat_v, step.flat_p16, flat_e
    omd = float(torch.tensor(1.0 - decay, dtype=torch.float32))
    count = [0]

    def adamw(ema):
        count[0] += 1
        t = count[0]
        bc1, bc2 = 1 - 0.9 ** t, 1 - 0.999 ** t
        step.sq.zero_()
        lib.sqnorm(G, step.sq, step.total)
        for lo, hi, lr in groups:
            if ema:
                lib.adamw_step_ema(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], S[lo:hi], E[lo:hi], step.sq, None, hi - lo, lr, 0.9, 0.999, 1e-8,
                                   cfg.weight_decay, bc1, bc2, cfg.clip_max_norm, 1.0, decay, False, t)
            else:
                lib.adamw_step(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], S[lo:hi], step.sq, hi - lo, lr, 0.9, 0.999, 1e-8, cfg.weight_decay,
                               bc1, bc2, cfg.clip_max_norm, 1.0)

    def leg_b():
        adamw(False)
        E.lerp_(P, omd)

    variants = {"A_a": lambda: adamw(False), "B": leg_b, "C": lambda: adamw(True), "A_b": lambda: adamw(False)}
    names = list(variants)
    for n in names:                                              # warm-up round
        window(variants[n], args.calls)
    w = {n: [] for n in names}
    for r in range(args.rounds):
        k = r % len(names)
        for n in names[k:] + names[:k]:
            w[n].append(window(variants[n], args.calls))
    opt = res["optimizer"] = {n: dict(summary(w[n]), calls_per_window=args.calls) for n in names}
    a = 0.5 * (opt["A_a"]["ms"] + opt["A_b"]["ms"])
    opt["rounds"] = args.rounds
    opt["A_ms"] = round(a, 5)
    opt["A_against_itself_ms"] = round(abs(opt["A_a"]["ms"] - opt["A_b"]["ms"]), 5)
    opt["B_minus_C_ms"] = round(opt["B"]["ms"] - opt["C"]["ms"], 5)
    opt["C_minus_A_ms"] = round(opt["C"]["ms"] - a, 5)
    opt["B_minus_A_ms"] = round(opt["B"]["ms"] - a, 5)
    opt["done"] = bool(opt["B_minus_C_ms"] > opt["A_against_itself_ms"])
    # the sqnorm pass reads 4 more bytes per element in every variant; the rates below are the AdamW pass's own bytes over the whole leg
    opt["bytes_per_element"] = dict(BYTES_PER_ELEMENT, sqnorm=4)
    opt["C_TBps_at_38_bytes_per_element"] = round(step.total * 38 / (opt["C"]["ms"] * 1e-3) / 1e12, 4)
    opt["A_TBps_at_30_bytes_per_element"] = round(step.total * 30 / (a * 1e-3) / 1e12, 4)
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(E).all())

    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

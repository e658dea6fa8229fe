"""Census of the bias gradients of one train step of bench.py's workload: which ride with their layer's weight-gradient job
(gwd_conv_desc.dbias) and which still run as column sums, grouped by the reason (DESIGN.md "Bias gradients inside the weight gradient").

    python tools/bias_census.py [--batch 8 --height 480 --width 640]

One eager step (the captured step issues the same calls).  Counts the calls of ops.COLSUMS.add by call site and, for the ones from
_ConvFn.backward, why the bias did not go with the weight gradient."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    from gw_depth_amd import Config, build_model, hip, ops
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import det_fill_, synth_batch
    lib = hip.library()
    cfg = Config(device="cuda", dropout=0.1, log_depth_error=True)
    model, crits, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda()
    crits[0].cuda()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=False)
    b = synth_batch(a.batch, a.height, a.width, seed=1)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    batch["targets"] = [{k: v.cuda() for k, v in t.items()} for t in b["targets"]]
    step(batch)                                            # warm: caches, scratch pools

    rides, colsums, asked = collections.Counter(), collections.Counter(), {}
    q_add, w_add, takes = ops.COLSUMS.add, ops.WGRADS.add, lib.conv_wgrad_takes_bias

    def takes_logged(x, gy, dims, batched, **kw):
        r = takes(x, gy, dims, batched, **kw)
        asked[gy.data_ptr()] = (r, dims, kw, str(x.dtype))
        return r

    def wgrad_add(x, dv, dw, dims, kw, hook=None, unpad=None):
        if kw.get("dbias") is not None:
            rides["%d x %d -> %d k%d s%d" % (dims[0] * dims[4] * dims[5], dims[3], dims[6], dims[7], kw.get("stride", 1))] += 1
        return w_add(x, dv, dw, dims, kw, hook, unpad)

    def colsum_add(g, out, rows, C, hook=None):
        f = sys._getframe(1)
        site = "%s:%s" % (f.f_code.co_name, os.path.basename(f.f_code.co_filename))
        why = "not a conv / Linear bias"
        if f.f_code.co_name == "backward" and "dims" in f.f_locals and "w_sink" in f.f_locals:
            q = asked.get(g.data_ptr())
            loc = f.f_locals
            if not loc["ctx"].needs_input_grad[1] or loc["w_sink"] is None:
                why = "no weight-gradient job into the flat buffer"
            elif q is None:
                why = "weight gradient in another form (upsampled taps)"
            else:
                _, dims, kw, dt = q
                why = "query 0: %s, %d x %d -> %d k%d s%d%s" % (dt, dims[0] * dims[4] * dims[5], dims[3], dims[6], dims[7], kw.get("stride", 1),
                                                             ", scale" if kw.get("scale") is not None else "")
        colsums[(site, why, "rows %d C %d" % (rows, C))] += 1
        return q_add(g, out, rows, C, hook)

    lib.conv_wgrad_takes_bias, ops.WGRADS.add, ops.COLSUMS.add = takes_logged, wgrad_add, colsum_add
    try:
        step(batch)
        torch.cuda.synchronize()
    finally:
        lib.conv_wgrad_takes_bias, ops.WGRADS.add, ops.COLSUMS.add = takes, w_add, q_add
    print("bias gradients that ride with the weight gradient: %d" % sum(rides.values()))
    for k, n in sorted(rides.items(), key=lambda kv: -kv[1]):
        print("  %3d  %s" % (n, k))
    print("column-sum jobs that remain: %d" % sum(colsums.values()))
    for (site, why, shape), n in sorted(colsums.items(), key=lambda kv: (kv[0][0], kv[0][1], -kv[1])):
        print("  %3d  %-28s %-22s %s" % (n, site, shape, why))


if __name__ == "__main__":
    main()

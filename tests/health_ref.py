"""fp64 references of csrc/health.hip (CPU only, plain module): gwd_segment_stats and gwd_health_decide restated from
include/gwdepth.h.  Nothing here goes through the product's kernels or through tests/fake_device.py.

segment_stats: the squares of fp32 values are exact in fp64 and math.fsum adds them without error, so `sumsq` is the correctly
rounded sum; a device sum of the n_s non-negative terms of a segment, in ANY order, is within (n_s - 1) 2^-53 sumsq of it
(``sumsq_bound``: the recursive-summation bound).  absmax and nonfinite are exact.
decide: the counters, bias corrections and clip coefficient of one step; the fp32 statements are made in numpy float32.
"""
import math

import numpy as np
import torch

F32 = np.float32


def segment_stats(x, seg_begin, seg_end, exact=True):
    """x: flat fp32 CPU tensor -> [(sumsq, absmax, nonfinite)] per segment (Python float, float, int).  exact=False adds the exact
    squares with torch's fp64 sum instead of math.fsum: for the CPU stand-in over a whole model, never for a kernel's reference."""
    out = []
    for b, e in zip(seg_begin, seg_end):
        v = x[int(b):int(e)].double()
        fin = torch.isfinite(v)
        f = v[fin]
        out.append((math.fsum((f * f).tolist()) if exact else float((f * f).sum()), float(f.abs().max()) if f.numel() else 0.0, int((~fin).sum())))
    return out


def sumsq_bound(n, sumsq):
    return n * 2.0 ** -53 * sumsq


def bias_corrections(beta1, beta2, t):
    return float(F32(1.0 - beta1 ** t)), float(F32(1.0 - beta2 ** t))


def new_ctl():
    return {"sq": 0.0, "applied": 0, "skipped": 0, "streak": 0, "nonfinite_total": 0, "apply": 0, "loss_finite": 0, "bc1": 0.0, "bc2": 0.0,
            "clip_coef": 0.0, "loss": 0.0}


def decide(stats, ctl, loss, beta1, beta2, max_norm, grad_scale, bad=None):
    """One gwd_health_decide: stats as segment_stats returns them, ctl a dict as new_ctl(); -> (ctl', ring record, bad')."""
    c = dict(ctl)
    sq = 0.0
    for s in stats:                                     # the fold, in segment order
        sq += s[0]
    nf = sum(s[2] for s in stats)
    apply = int(nf == 0)
    c.update(sq=sq, nonfinite_total=nf, apply=apply, applied=c["applied"] + apply, skipped=c["skipped"] + 1 - apply,
             streak=0 if apply else c["streak"] + 1)
    if apply:
        c["bc1"], c["bc2"] = bias_corrections(beta1, beta2, c["applied"])
    clip = F32(1.0)
    if F32(max_norm) > 0:
        total = F32(math.sqrt(sq)) * F32(grad_scale)
        clip = min(F32(max_norm) / (total + F32(1e-6)), F32(1.0))
    c["clip_coef"] = float(clip)
    c["loss"] = 0.0 if loss is None else float(F32(loss))
    c["loss_finite"] = int(loss is not None and math.isfinite(c["loss"]))
    rec = {"step": c["applied"] + c["skipped"], "apply": bool(apply), "grad_norm": math.sqrt(sq) * float(F32(grad_scale)),
           "clip_coef": c["clip_coef"], "loss": c["loss"], "nonfinite_total": nf}
    return c, rec, (bad if apply else [s[2] for s in stats])

"""fp64 reference and error bound of the weight average of csrc/ema.hip (CPU only, plain module).

    d    = min(decay, (1 + t) / (10 + t)) with the warm-up on, decay without it      (fp64, t the 1-based update number)
    omd  = float32(1 - d)                                                            (rounded once)
    ema' = ema + omd (p' - ema)

The kernel forms ema' = fmaf(omd, fl32(p' - ema), ema): two roundings, the difference's and the fmaf's.  An element is charged
against the p' THE KERNEL RETURNED (as p16 is in tests/loss_ref.py), so AdamW's own error is not counted twice:

    |ema'_got - ema'_ref| <= 0.5 ulp32(p' - ema) omd + 0.5 ulp32(|ema'_ref| + first term) + 4 * 2^-53 (|p'| + |ema|)

first term: the rounding of the difference, scaled by omd; second: the rounding of the fmaf (its exact argument lies within the first
term of the reference, so the ulp is taken at that distance); third: the reference's own three fp64 roundings.  No fitted constant.
A zero difference has no rounding: p' == ema gives ema' == ema exactly."""
import numpy as np
import torch

F32_MIN_ULP = 2.0 ** -149


def decay_at(t, decay, warmup):
    """The decay of update t, in fp64 (Python floats)."""
    return min(float(decay), (1.0 + float(t)) / (10.0 + float(t))) if warmup else float(decay)


def omd_at(t, decay, warmup):
    """float32(1 - d), as the double the kernel's fp32 value widens to."""
    return float(np.float32(1.0 - decay_at(t, decay, warmup)))


def ema_update(e, p_new, omd):
    """fp64 ema' from the fp32 operands e, p_new and the fp32 value omd."""
    e64, p64 = e.double(), p_new.double()
    return e64 + float(omd) * (p64 - e64)


def ulp32(x):
    """The fp32 unit in the last place at the magnitude of the fp64 tensor x: 2^(floor(log2 |x|) - 23), 2^-149 in the denormals,
    0 at x == 0 (an exact zero is not rounded)."""
    x = x.double().abs()
    _, ex = torch.frexp(x)                                       # |x| = m 2^ex, m in [0.5, 1)
    u = torch.pow(torch.tensor(2.0, dtype=torch.float64), (ex - 24).double()).clamp_min(F32_MIN_ULP)
    return torch.where(x == 0, torch.zeros_like(u), u)


def ema_bound(e, p_new, omd, ref=None):
    ref = ema_update(e, p_new, omd) if ref is None else ref
    first = 0.5 * ulp32(p_new.double() - e.double()) * float(omd)
    return first + 0.5 * ulp32(ref.abs() + first) + 4.0 * 2.0 ** -53 * (p_new.double().abs() + e.double().abs())


def check(got_e, e, p_new, omd, what=""):
    """Every element of the average the kernel returned against the reference under the bound -> the worst |error| / bound."""
    ref = ema_update(e, p_new, omd)
    bound = ema_bound(e, p_new, omd, ref)
    err = (got_e.double() - ref).abs()
    bad = ~(err <= bound)                                        # a NaN is outside
    assert not bool(bad.any()), "%s: %d of %d elements outside the bound; first at %d: got %r ref %r err %.3g bound %.3g" % (
        what, int(bad.sum()), bad.numel(), int(bad.nonzero()[0]), float(got_e[bad][0]), float(ref[bad][0]), float(err[bad][0]),
        float(bound[bad][0]))
    r = err / bound.clamp_min(1e-300)
    return float(r.max()) if r.numel() else 0.0


def ema_values(n, seed):
    """Averages of both signs with magnitudes from 1e-8 to 1e4, log-uniform."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(torch.tensor(10.0, dtype=torch.float64), torch.rand(n, generator=g, dtype=torch.float64) * 12.0 - 8.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()

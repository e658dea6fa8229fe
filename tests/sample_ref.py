"""fp64 reference, conditions and fp32 model of CertainSample on the device (csrc/sample.hip, gwd_certain_sample; CPU only, plain
module, plain numpy).  The output is a list of pixel coordinates, so there is no rounding bound: the comparison is EXACT, and the
inputs are built so that an exact comparison is legitimate.

* ``reference(c, inp)`` -> (coords, cond).  Per image, all in fp64 on the fp32 operands:
      up    = align-corners bilinear up-sampling of small (hs, ws) -> (H, W): fy = y (hs - 1) / (H - 1) (0 when H = 1), y0 = floor(fy),
              y1 = min(y0 + 1, hs - 1), the four-tap blend; the same along x
      var   = (up - large)^2
      n_i   = #{pixels: edges[i] <= large < edges[i + 1]}
      k_i   = min(floor(fl32(fl32(n_i / HW) S)), n_i), evaluated in numpy.float32 (the reference evaluates it in fp32 tensors; where
              fp64 disagrees, fp32 is the contract)
      order = stable descending order of var: ties go to the lowest pixel index
      every interval with k_i > 0 contributes the k_i best pixels in ascending pixel index; no such interval: the S best pixels
      (the global branch); remain = S - sum k_i: remain >= sum k_i repeats the whole list remain // sum + 1 times, a remainder is
      complemented with the list's tail, a negative one is trimmed from the largest group (the first on ties; no case reaches
      the trim: k_i exceeds n_i S / HW by less than an fp32 unit of S, so sum k_i < S + 1)
      coords = (fl32(fl32(col / W) 2 - 1), fl32(fl32(row / H) 2 - 1)), evaluated in numpy.float32
  cond holds what the CPU file asserts about the case for the reference ALONE: ``var`` (fp64), ``ks``, ``n``, ``kmax``, the branch of
  every image and, in the margin regime, ``gap`` (the smallest distance of two consecutive variances among the kmax + 1 largest)
  and ``err`` (twice the largest |model variance - reference variance| of the image: the same factor 2 as the constants of the
  other witnesses).
* Two input regimes make the exact comparison legitimate.
      exact   every fp32 operation of the kernel's variance is exact, so the fp32 variance map equals the fp64 one bit for bit
              (asserted on the CPU).  Either H - 1 = 2 (hs - 1) and W - 1 = 2 (ws - 1) (all blend weights in {0, 1/2, 1}) with small
              and large multiples of 1/64 in [0, 1] - var = (k / 256)^2 -, or small constant 0.5 (the blend of equal taps is exact
              at any ratio: hx 0.5 + lx 0.5 = 0.5 fl(fl(1 - lx) + lx) = 0.5) with large in multiples of 1/64.  Ties abound here.
      margin  a general ratio (15 x 20 -> 30 x 40, 50 x 70 -> 192 x 192).  large = up + offsets: S + 4 marked pixels get |offset| =
              0.30 + 0.004 j (variances 2.4e-3 apart), all others |offset| <= 0.2.  The CPU file asserts gap > 2 err, i.e. the
              reference's selection is unchanged when every variance moves by +- err.  ``inputs`` re-draws until that holds.
* ``model(c, inp, defect=None)``: the kernel's arithmetic in numpy.float32 (sh = fl(hs - 1) / fl(H - 1), fy = fl(sh y), y0 = int(fy),
  the clamps, the blend as written in sample.hip without fused multiply-adds), the selection as a lexicographic sort of (value
  descending, index ascending) and the kernel's list surgery on an index array.  Defects: ``tie_high`` (ties to the highest
  index), ``k_fp64``, ``x1_noclamp`` (reads the next element of the flat buffer: the next row, the next image, or the NaN guard
  behind the last image), ``edge_inclusive`` (large <= edges[i + 1]), ``repeat_off`` (a repeat count one short).

MEASURED (CPU, 2026-10): the bound is zero, C = 0: every coordinate is compared for equality.  Largest err of a margin case:
@ERR@ against a smallest gap of @GAP@.
"""
import types
import zlib

import numpy as np

DEFECTS = ("tie_high", "k_fp64", "x1_noclamp", "edge_inclusive", "repeat_off")
MAX_PIX, MAX_S, MAX_INT, THREADS = 36864, 256, 8, 256           # csrc/sample.hip
GUARD = 8
f32 = np.float32


def _case(kind, B, hs, ws, H, W, S, n_int, regime):
    c = types.SimpleNamespace(kind=kind, B=B, hs=hs, ws=ws, H=H, W=W, S=S, n_int=n_int, regime=regime)
    c.text = "sample %s B=%d %dx%d->%dx%d S=%d n_int=%d %s" % (kind, B, hs, ws, H, W, S, n_int, regime)
    c.id = c.text.replace(" ", "-")
    return c


def k_of(n, HW, S):
    """k_i as the reference evaluates it: IEEE fp32."""
    return int(min(np.floor(f32(f32(n) / f32(HW)) * f32(S)), f32(n)))


def k_of_fp64(n, HW, S):
    return int(min(np.floor(float(n) / float(HW) * float(S)), float(n)))


def find_k_split(HW):
    """The first (S, n) in a fixed scan at which the fp64 evaluation of k_i differs from the fp32 one."""
    for S in range(2, min(HW, MAX_S) + 1):
        for n in range(1, HW + 1):
            if k_of(n, HW, S) != k_of_fp64(n, HW, S):
                return S, n
    raise AssertionError("no split for HW = %d" % HW)


KSPLIT_SHAPE = (7, 9, 13, 17)                                  # hs, ws, H, W of the k-split case
KSPLIT_S, KSPLIT_N = find_k_split(13 * 17)


def cases():
    return [
        _case("limits", 2, 50, 70, 192, 192, 256, 8, "margin"),
        _case("general", 3, 15, 20, 30, 40, 80, 5, "margin"),
        _case("allequal", 2, 96, 96, 192, 192, 80, 5, "exact"),
        _case("thr33000", 2, 96, 96, 192, 192, 256, 1, "exact"),
        _case("h1", 2, 3, 9, 1, 17, 8, 3, "exact"),
        _case("w1", 2, 9, 3, 17, 1, 8, 3, "exact"),
        _case("hsws1", 2, 1, 1, 9, 13, 40, 4, "exact"),
        _case("mid", 2, 33, 41, 65, 81, 256, 8, "exact"),           # the four-tap blend with ties, 21 pixels per thread
        _case("small", 2, 7, 9, 13, 17, 64, 5, "exact"),           # HW = 221 < 256 threads
        _case("s_eq_hw", 2, 3, 3, 5, 5, 25, 3, "exact"),
        _case("s1", 2, 3, 3, 5, 5, 1, 3, "exact"),
        _case("oneint", 2, 7, 9, 13, 17, 64, 1, "exact"),          # remain = 0 in image 0
        _case("onedges", 2, 7, 9, 13, 17, 64, 4, "exact"),
        _case("global", 2, 7, 9, 13, 17, 64, 5, "exact"),
        _case("repeat", 3, 7, 9, 13, 17, 64, 5, "exact"),
        _case("ksplit", 2, KSPLIT_SHAPE[0], KSPLIT_SHAPE[1], KSPLIT_SHAPE[2], KSPLIT_SHAPE[3], KSPLIT_S, 2, "exact"),
    ]


def rejected():
    """(B, hs, ws, H, W, S, n_int) that gwd_certain_sample answers with -4."""
    return [(1, 4, 4, 193, 192, 16, 2), (1, 4, 4, 16, 16, 257, 2), (1, 2, 2, 3, 3, 10, 2), (1, 4, 4, 16, 16, 16, 9)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(c, attempt=0):
    return np.random.default_rng(zlib.crc32(("%s #%d" % (c.text, attempt)).encode()))


def _axis64(n_src, n_dst):
    f = np.arange(n_dst, dtype=np.float64) * ((n_src - 1) / (n_dst - 1)) if n_dst > 1 else np.zeros(n_dst)
    i0 = np.floor(f).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, f - i0


def upsample64(sm, H, W):
    """(hs, ws) -> (H, W), align-corners bilinear in fp64."""
    sm = sm.astype(np.float64)
    y0, y1, ly = _axis64(sm.shape[0], H)
    x0, x1, lx = _axis64(sm.shape[1], W)
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * sm[y0][:, x0] + lx * sm[y0][:, x1]
    bot = (1 - lx) * sm[y1][:, x0] + lx * sm[y1][:, x1]
    return (1 - ly) * top + ly * bot


def _q64(g, shape, lo=0, hi=64):
    return (g.integers(lo, hi + 1, size=shape) / 64.0).astype(f32)


def _exact_edges(n_int, lo=16, hi=48):
    """n_int + 1 increasing multiples of 1/64 from lo/64 to hi/64."""
    e = np.round(np.linspace(lo, hi, n_int + 1)).astype(np.int64)
    assert len(set(e.tolist())) == n_int + 1
    return (e / 64.0).astype(f32)


def _exact_inputs(c, g):
    B, hs, ws, H, W, HW = c.B, c.hs, c.ws, c.H, c.W, c.H * c.W
    small = _q64(g, (B, 1, hs, ws))
    large = _q64(g, (B, 1, H, W))
    edges = _exact_edges(c.n_int)
    k = c.kind
    if k == "allequal":                                      # every variance 1/16; image 1 spreads the depths over the intervals
        small[:] = 0.5
        large[0] = 0.75
        large[1] = np.where(g.random((1, H, W)) < 0.5, 0.25, 0.75)
        edges = np.array([0.125, 0.25, 0.5, 0.625, 0.75, 1.0], dtype=f32)
    elif k == "thr33000":                                    # the pixels equal to the threshold value lie at indices >= 33000 only
        small[:] = 0.5
        flat = np.full((B, HW), 0.5, dtype=f32)              # variance 0
        for b in range(B):
            low = g.choice(33000, size=100 + 17 * b, replace=False)
            flat[b, low] = 1.0                               # variance 1/4: above the threshold, fewer than kmax of them
            tied = 33000 + g.choice(HW - 33000, size=3000, replace=False) if b else np.arange(33000, HW)
            flat[b, tied] = 0.75                             # variance 1/16: the threshold value
        large = flat.reshape(B, 1, H, W)
        edges = np.array([0.0, 2.0], dtype=f32)
    elif k == "oneint":
        edges = np.array([0.0, 2.0], dtype=f32)              # image 0: every pixel inside, k = S, remain = 0
        large[1].flat[:HW // 2] = 2.0                        # image 1: half of them outside
    elif k == "onedges":                                     # every depth equals an edge, edges[0] and edges[n_int] included
        large = edges[g.integers(0, c.n_int + 1, size=(B, 1, H, W))]
    elif k == "global":                                      # image 0 below edges[0], image 1 at and above edges[n_int]; no interval has a pixel
        large[0] = _q64(g, (1, H, W), 0, 15)
        large[1] = _q64(g, (1, H, W), 48, 64)
    elif k == "repeat":                                      # image 0: remain >= already; image 1: 0 < remain < already; image 2: few
        inside = (0.3, 0.8, 0.1)
        for b in range(B):
            out = g.random((1, H, W)) >= inside[b]
            large[b] = np.where(out, _q64(g, (1, H, W), 50, 64), _q64(g, (1, H, W), 16, 47))
    elif k == "ksplit":                                      # image 0: interval 0 holds exactly the n at which fp32 and fp64 disagree
        flat = np.full((B, HW), 60 / 64.0, dtype=f32)
        for b in range(B):
            n0 = KSPLIT_N if b == 0 else KSPLIT_N // 2
            flat[b, g.choice(HW, size=n0, replace=False)] = 20 / 64.0
        rest = flat == f32(60 / 64.0)
        flat[rest] = np.where(g.random(int(rest.sum())) < 0.5, 40 / 64.0, 60 / 64.0).astype(f32)
        large = flat.reshape(B, 1, H, W)
        edges = np.array([16 / 64.0, 32 / 64.0, 48 / 64.0], dtype=f32)
    return small, large, edges


def _margin_inputs(c, g):
    B, hs, ws, H, W, HW = c.B, c.hs, c.ws, c.H, c.W, c.H * c.W
    small = (0.3 + 0.4 * g.random((B, 1, hs, ws))).astype(f32)
    large = np.empty((B, 1, H, W), dtype=f32)
    marked = min(HW, c.S + 4)
    for b in range(B):
        up = upsample64(small[b, 0], H, W).reshape(-1)
        mag = 0.2 * g.random(HW)
        mag[g.choice(HW, size=marked, replace=False)] = 0.30 + 0.004 * g.permutation(marked)
        sign = np.where(up + mag > 1.6, -1.0, np.where(g.random(HW) < 0.5, 1.0, -1.0))
        if b == B - 1:
            sign[:] = 1.0                                    # the last image keeps more of its depths above the intervals
        large[b, 0] = (up + sign * mag).reshape(H, W).astype(f32)
    edges = np.linspace(0.1, 1.0, c.n_int + 1).astype(f32)
    return small, large, edges


def margin_of(c, inp, ref_cond):
    """Smallest (gap - 2 err) over the images of a margin case."""
    return min(float(gp - 2 * e) for gp, e in zip(ref_cond["gap"], ref_cond["err"]))


def inputs(c):
    for attempt in range(8):
        g = _gen(c, attempt)
        small, large, edges = (_exact_inputs if c.regime == "exact" else _margin_inputs)(c, g)
        inp = {"small": np.ascontiguousarray(small, dtype=f32), "large": np.ascontiguousarray(large, dtype=f32), "edges": edges.astype(f32)}
        if c.regime == "exact" or margin_of(c, inp, reference(c, inp)[1]) > 0:
            return inp
    raise AssertionError("%s: no draw with the margin" % c.text)


# ------------------------------------------------------------------------------------------------------------- reference
def _coords(idx, H, W):
    idx = np.asarray(idx, dtype=np.int64)
    col, row = (idx % W).astype(f32), (idx // W).astype(f32)
    return np.stack([(col / f32(W)) * f32(2) - f32(1), (row / f32(H)) * f32(2) - f32(1)], axis=-1).astype(f32)


def reference(c, inp):
    B, H, W, HW, S = c.B, c.H, c.W, c.H * c.W, c.S
    edges = inp["edges"].astype(np.float64)
    out = np.empty((B, S, 1, 2), dtype=f32)
    cond = {"var": [], "ks": [], "n": [], "kmax": [], "branch": [], "gap": [], "err": []}
    mvar = None if c.regime == "exact" else model_var(c, inp)
    for b in range(B):
        lg = inp["large"][b, 0].astype(np.float64)
        var = ((upsample64(inp["small"][b, 0], H, W) - lg) ** 2).reshape(-1)
        lgf = lg.reshape(-1)
        n = [int(((lgf >= edges[i]) & (lgf < edges[i + 1])).sum()) for i in range(c.n_int)]
        ks = [k_of(ni, HW, S) for ni in n]
        order = np.argsort(-var, kind="stable")
        groups = [np.sort(order[:k]) for k in ks if k > 0]
        already = sum(ks)
        if groups:
            lst, remain, branch = np.concatenate(groups), S - already, "exact"
        else:
            lst, remain, branch = np.sort(order[:S]), 0, "global"
        if remain > 0 and remain >= already:
            times = remain // already + 1
            lst, remain, branch = np.tile(lst, times), S - already * times, "repeat"
        if remain > 0:
            lst = np.concatenate([lst, lst[-remain:]])
            branch = "complement" if branch == "exact" else branch
        if remain < 0:
            mid = int(np.argmax([len(x) for x in groups]))
            groups[mid] = groups[mid][:remain]
            lst, branch = np.concatenate(groups), "trim"
        assert len(lst) == S
        out[b, :, 0] = _coords(lst, H, W)
        kmax = S if not groups else max(ks)
        top = var[order[:min(kmax + 1, HW)]]
        cond["var"].append(var)
        cond["ks"].append(ks)
        cond["n"].append(n)
        cond["kmax"].append(kmax)
        cond["branch"].append(branch)
        cond["gap"].append(float(np.min(top[:-1] - top[1:])) if len(top) > 1 else float("inf"))
        cond["err"].append(0.0 if mvar is None else 2.0 * float(np.max(np.abs(mvar[b].astype(np.float64) - var))))
    return out, cond


# ----------------------------------------------------------------------------------------------------------------- model
def _axis32(n_src, n_dst, clamp=True):
    s = f32(n_src - 1) / f32(n_dst - 1) if n_dst > 1 else f32(0)
    f = (s * np.arange(n_dst, dtype=f32)).astype(f32)
    i0 = f.astype(np.int32)
    i1 = i0 + ((i0 < n_src - 1) if clamp else 1)
    l = (f - i0.astype(f32)).astype(f32)
    return i0.astype(np.int64), i1.astype(np.int64), l, (f32(1) - l).astype(f32)


def model_var(c, inp, defect=None):
    """(B, HW) fp32: the variance map as sample.hip computes it."""
    B, hs, ws, H, W = c.B, c.hs, c.ws, c.H, c.W
    flat = np.concatenate([inp["small"].reshape(-1), np.full(GUARD + ws, np.nan, dtype=f32)])
    y0, y1, ly, hy = _axis32(hs, H)
    x0, x1, lx, hx = _axis32(ws, W, clamp=defect != "x1_noclamp")
    ly, hy, lx, hx = ly[:, None], hy[:, None], lx[None, :], hx[None, :]
    out = np.empty((B, H * W), dtype=f32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            base = b * hs * ws
            at = lambda yy, xx: flat[base + yy[:, None] * ws + xx[None, :]]
            up = hy * (hx * at(y0, x0) + lx * at(y0, x1)) + ly * (hx * at(y1, x0) + lx * at(y1, x1))
            d = (up - inp["large"][b, 0]).astype(f32)
            out[b] = (d * d).astype(f32).reshape(-1)
    return out


def model(c, inp, defect=None):
    assert defect is None or defect in DEFECTS
    B, H, W, HW, S = c.B, c.H, c.W, c.H * c.W, c.S
    var = model_var(c, inp, defect)
    edges = inp["edges"]
    out = np.empty((B, S, 1, 2), dtype=f32)
    for b in range(B):
        l = inp["large"][b, 0].reshape(-1)
        kk = []
        for i in range(c.n_int):
            hi = (l <= edges[i + 1]) if defect == "edge_inclusive" else (l < edges[i + 1])
            n = int(((l >= edges[i]) & hi).sum())
            kk.append(k_of_fp64(n, HW, S) if defect == "k_fp64" else k_of(n, HW, S))
        total = sum(kk)
        kmax = max(kk) if total > 0 else S
        bits = np.where(np.isnan(var[b]), f32(np.inf), var[b]).astype(f32).view(np.uint32).astype(np.int64)   # NaN patterns sort above all
        idx = np.arange(HW)
        order = np.lexsort((idx if defect != "tie_high" else -idx, -bits))[:kmax]
        outidx = np.zeros(4 * MAX_S + S, dtype=np.int64)
        n_out, gstart, gcount = 0, [], []
        if total > 0:
            for k in kk:
                if k > 0:
                    gstart.append(n_out)
                    gcount.append(k)
                    outidx[n_out:n_out + k] = np.sort(order[:k])
                    n_out += k
        else:
            outidx[:S] = np.sort(order[:S])
            n_out = S
        remain = S - total if total > 0 else 0
        if remain > 0 and remain >= total:
            times = remain // total + (0 if defect == "repeat_off" else 1)
            for t in range(1, times):
                outidx[t * total:(t + 1) * total] = outidx[:total]
            n_out = total * times
            remain = S - n_out
        if remain > 0:
            for a in range(remain):
                outidx[n_out + a] = outidx[max(n_out - remain + a, 0)]
            n_out += remain
        if remain < 0:
            mid = int(np.argmax(gcount))
            cut, frm = -remain, gstart[mid] + gcount[mid]
            outidx[frm - cut:n_out - cut] = outidx[frm:n_out].copy()
        out[b, :, 0] = _coords(outidx[:S], H, W)
    return out


def threshold_search(var32, kmax):
    """sample.hip's selection, restated: -> (T bits, n_gt, need_eq, I) of one image's fp32 variance map."""
    bits = var32.view(np.uint32).astype(np.int64)
    T = 0
    for bit in range(30, -1, -1):
        cand = T | (1 << bit)
        if int((bits >= cand).sum()) >= kmax:
            T = cand
    n_gt = int((bits > T).sum())
    need = kmax - n_gt
    idx = np.arange(len(bits))
    I = 0
    for bit in range(15, -1, -1):
        cand = I | (1 << bit)
        if int(((bits == T) & (idx < cand)).sum()) < need:
            I = cand
    return T, n_gt, need, I


def measure_c():
    """-> (largest err, smallest gap) over the margin cases; the constant itself is 0 (exact comparison)."""
    err, gap = 0.0, float("inf")
    for c in cases():
        if c.regime == "margin":
            cond = reference(c, inputs(c))[1]
            err, gap = max(err, max(cond["err"])), min(gap, min(cond["gap"]))
    return err, gap


MEASURED = {"err": 4.1e-6, "gap": 3.6e-3}
C = 0.0
__doc__ = __doc__.replace("@ERR@", "%.1e" % MEASURED["err"]).replace("@GAP@", "%.1e" % MEASURED["gap"])

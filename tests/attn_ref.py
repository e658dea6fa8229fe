"""fp64 references, rounding models and the element-wise comparator of the attention kernels (CPU only, plain module).

Every reference works on operands that are ALREADY rounded to the storage type (bf16 or fp32) and widened; the only error left
between a kernel and its reference is the kernel's own arithmetic.

Three things per operation:

* ``*_ref64``   - the operation written from its formula in fp64, gradients through fp64 autograd
                  (window attention: multiscale_transformerr.py:311-328, 937-955; class-token attention: :560-578;
                  reference points: :296-309; DETR attention core: multi_head_attention.py:329-375).
* ``*_cond``    - for every output element the fp64 sum of the absolute values of the terms it is a sum of (expressions next
                  to each operation below).  Each is a pair (A, B): A carries the terms that are rounded to the STORAGE
                  type on their way (P, dS, A crossing registers / LDS as bf16, the stored O re-read by the MHA backward),
                  B the fp32 error of the scores seen through the softmax (|score terms| x the same sum).  The bound of an
                  element is  c * u * (|ref| + A + (2^-24 / u) * B),  u = 2^-9 for a bf16 output and 2^-24 for an fp32 one.
* ``*_model``   - the kernel's arithmetic on the CPU in fp32 with a bf16 rounding exactly where the kernel's header comment
                  has one (operands; P / dS / A where an accumulator tile becomes an MFMA operand or crosses LDS; the stored
                  output) and nowhere else.  With ``rounding=False`` it is the fp32 kernels' model: the same arithmetic in
                  fp32 with every reduction run over the reversed axis (another summation order).
                  It exists to size ``c`` without looking at a kernel's output.

The constants.  ``attn_cases.measure_c()`` (tests/test_attn_ref.py runs it) evaluates the models over the case matrix of
tests/attn_cases.py and takes the largest |model - ref64| / (u (|ref| + cond)); C is twice that, rounded up to one decimal
(the factor 2 covers the summation order of the device and its exp / log).  Measured on the CPU, 2026-10:

    operation            output   bf16 model max   C[bf16]    fp32 model max   C[fp32]
    ------------------   ------   --------------   -------    --------------   -------
    mha                  dk       1.071            2.2        0.347            0.7
    mha                  dq       0.621            1.3        0.395            0.8
    mha                  dv       1.842            3.7        0.976            2.0
    mha                  lse      2.044            4.1        2.191            4.4
    mha                  o        1.555            3.2        1.208            2.5
    ref_mix              att      1.991            4.0        1.012            2.1
    ref_mix              d_ra     1.991            4.0        2.288            4.6
    ref_mix              dv       3.406            6.9        4.556            9.2
    ref_mix              q_new    1.990            4.0        0.753            1.6
    ref_scores           dk       1.378            2.8        3.180            6.4
    ref_scores           dq       1.992            4.0        2.855            5.8
    ref_scores           ra       1.992            4.0        2.711            5.5
    softmax              gx       0.962            2.0        1.850            3.7
    softmax              y        1.992            4.0        1.567            3.2
    token                dk       1.920            3.9        0.684            1.4
    token                dq       1.789            3.6        0.484            1.0
    token                dv       1.955            4.0        2.641            5.3
    token                o        1.751            3.6        1.488            3.0
    token_pair           dk       1.924            3.9        -                -
    token_pair           dq       1.789            3.6        -                -
    token_pair           dq2      1.795            3.6        -                -
    token_pair           dv       1.893            3.8        -                -
    token_pair           o        1.751            3.6        -                -
    token_pair           o2       1.770            3.6        -                -
    window               dbias    0.716            1.5        0.660            1.4
    window               dk       1.810            3.7        0.365            0.8
    window               dq       1.828            3.7        0.518            1.1
    window               dv       1.918            3.9        1.151            2.4
    window               o        1.742            3.5        1.368            2.8

(ref_scores dk, ref_mix dv and window dbias are fp32 results of bf16 operands: their u is 2^-24 in both columns; they are sums over all
T = nwin x 49 tokens, whose rounding error grows with the length of the sum - hence the larger figures.  A single rounding to bf16
gives up to 2.0 in this measure, u = 2^-9 being half of bf16's rounding unit.)

A kernel that needs more than its C has a defect or the cond lacks a term: neither is repaired by raising C.
"""
import torch

U_BF16 = 2.0 ** -9
U_F32 = 2.0 ** -24
# Both storage types share fp32's exponent range and the device flushes subnormals: a probability below 2^-126 is a zero there and
# not in fp64.  An error of up to FLOOR (64 smallest normals: a sum of that many flushed terms) is therefore not counted - except
# where the bound is zero, which still demands an exact zero.
FLOOR = 2.0 ** -120
NT = 49


def unit_roundoff(dtype):
    return {torch.bfloat16: U_BF16, torch.float32: U_F32}[dtype]


def rb(x):
    """Round to bf16 and back (round to nearest even), keeping the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def as_storage(x, dtype):
    """fp64 image of x after rounding to the storage type of a kernel operand."""
    return x.to(dtype).double()


# ------------------------------------------------------------------------------------------------------------ comparator
def combine_cond(cond, u):
    a, b = cond
    return a if b is None else a + (U_F32 / u) * b


def ratio(got, ref64, cond, u):
    """|got - ref| / (u (|ref| + cond)) per element; elements whose bound is zero give 0 when exact and inf otherwise."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double()
    bound = u * (ref64.abs() + combine_cond(cond, u))
    err = ((got - ref64).abs() - torch.where(bound > 0, FLOOR, 0.0)).clamp_min(0.0)
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    exact = (got == ref64) | ((got == 0) & (ref64.abs() < FLOOR))        # (an fp64 subnormal reference is a zero of the device's types)
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(exact, torch.zeros_like(err), torch.full_like(err, float("inf"))))


def assert_elementwise(got, ref64, cond, c, names, u=None, what=""):
    """Every element: |got - ref| <= c u (|ref| + cond); a zero bound demands an exact zero.  names: one label per axis of `got`
    (e.g. ("window", "token", "head", "channel")): the worst violator is reported decoded into them."""
    u = unit_roundoff(got.dtype) if u is None else u
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    r = ratio(got, ref64, cond, u)
    bad = r > c
    worst = float(r.max()) if r.numel() else 0.0
    if bool(bad.any()):
        flat = int(torch.argmax(r))
        idx = []
        for n in reversed(r.shape):
            idx.append(flat % n)
            flat //= n
        idx = idx[::-1]
        where = ", ".join("%s %d" % (n, i) for n, i in zip(names, idx))
        t = tuple(idx)
        raise AssertionError("%s: %d of %d elements outside c = %.2f; worst ratio %.3g at (%s): got %.9g, reference %.9g, cond %.3g"
                             % (what, int(bad.sum()), r.numel(), c, worst, where, float(got.detach().double().cpu()[t]), float(ref64[t]),
                                float(combine_cond(cond, u)[t])))
    return worst


# ---------------------------------------------------------------------------------------------------- window attention
def dense_bias(table, rel):
    """(n_rel, H) table -> (H, 49, 49) through relative_position_index (multiscale_transformerr.py:313-315)."""
    return table[rel.reshape(-1).long()].view(NT, NT, -1).permute(2, 0, 1)


def table_grad(dense, rel, n_rel):
    """(H, 49, 49) -> (n_rel, H): the transpose of dense_bias."""
    out = dense.new_zeros(n_rel, dense.shape[0])
    out.index_add_(0, rel.reshape(-1).long(), dense.reshape(dense.shape[0], -1).t())
    return out


def region_fill(region, wpi, nwin, dtype):
    """(nwin, 1, 49, 49): -100 where the labels of query and key differ (window w reads region[w % wpi])."""
    reg = region.long()
    m = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).to(dtype)
    return m.repeat(nwin // wpi, 1, 1)[:, None]


def window_scores(q, k, bias, region, wpi, scale):
    s = scale * torch.einsum("wihd,wjhd->whij", q, k) + bias[None]
    if region is not None:
        s = s + region_fill(region, wpi, q.shape[0], s.dtype)
    return s


def window_ref64(q, k, v, bias, region, wpi, scale, go):
    """q, k, v, go (W, 49, H, D) fp64, bias (H, 49, 49) fp64 -> dict o, dq, dk, dv, dbias (dense), fp64 autograd."""
    q, k, v, bias = (t.detach().clone().requires_grad_(True) for t in (q, k, v, bias))
    o = torch.einsum("whij,wjhd->wihd", torch.softmax(window_scores(q, k, bias, region, wpi, scale), -1), v)
    g = torch.autograd.grad(o, [q, k, v, bias], go)
    return dict(o=o.detach(), dq=g[0], dk=g[1], dv=g[2], dbias=g[3])


def _flip(t, dim, on):
    return torch.flip(t, (dim,)) if on else t


def _window_explicit(q, k, v, bias, region, wpi, scale, go, r, alt):
    """The kernels' formulas; r rounds where mfattn.hip's window kernels round, alt reverses every reduction axis."""
    s = scale * torch.einsum("wihd,wjhd->whij", _flip(q, 3, alt), _flip(k, 3, alt)) + bias[None]
    if region is not None:
        s = s + region_fill(region, wpi, q.shape[0], s.dtype)
    m = s.max(-1, keepdim=True).values
    pu = torch.exp(s - m)                                    # P relative to the row maximum, in (0, 1]
    l = _flip(pu, 3, alt).sum(-1, keepdim=True)
    # forward: the UNNORMALISED P is the bf16 operand of O^T = V^T P^T, 1 / l rides on the store
    o = r(torch.einsum("whij,wjhd->wihd", _flip(r(pu), 3, alt), _flip(v, 1, alt)) / l.permute(0, 2, 1, 3))
    p = pu / l
    dp = torch.einsum("wihd,wjhd->whij", _flip(go, 3, alt), _flip(v, 3, alt))
    delta = _flip(p * dp, 3, alt).sum(-1, keepdim=True)      # in fp32 from the fp32 P and dP (no stored O is re-read)
    ds = p * (dp - delta)
    dq = r(scale * torch.einsum("whij,wjhd->wihd", _flip(r(ds), 3, alt), _flip(k, 1, alt)))
    dk = r(scale * torch.einsum("whij,wihd->wjhd", _flip(r(ds), 2, alt), _flip(q, 1, alt)))
    dv = r(torch.einsum("whij,wihd->wjhd", _flip(r(p), 2, alt), _flip(go, 1, alt)))
    dbias = _flip(ds, 0, alt).sum(0)                         # fp32 registers + fp32 atomics: never rounded to bf16
    return dict(o=o, dq=dq, dk=dk, dv=dv, dbias=dbias), dict(p=p, dp=dp, ds=ds, delta=delta)


def window_model(q, k, v, bias, region, wpi, scale, go, rounding=True):
    f = lambda t: t.float()
    return _window_explicit(f(q), f(k), f(v), f(bias), region, wpi, scale, f(go), rb if rounding else (lambda t: t), not rounding)[0]


def window_cond(q, k, v, bias, region, wpi, scale, go):
    """cond (A, B) of every output of window attention, fp64.
         sc_i     = max_j ( scale sum_d |q_id| |k_jd| + |bias_ij| + 100 [masked] )        the size of the terms of a score
         o_id     : A = sum_j P_ij |v_jd|                                   B = 2 sc_i A
         dP_ij    = sum_d dO_id v_jd,  adP_ij = sum_d |dO_id| |v_jd|
         dS_ij    = P_ij (dP_ij - delta_i);   aS_ij = |P_ij| |dP_ij - delta_i|
         eS_ij    = 2 sc_i aS_ij + P_ij (adP_ij + (1 + 2 sc_i) sum_j' P_ij' adP_ij')        fp32 error of dS, in units of 2^-24: of P_ij,
                                                                of dP_ij, and of delta_i (whose P carry the score error too)
         dq_id    : A = scale sum_j aS_ij |k_jd|                            B = scale sum_j eS_ij |k_jd|
         dk_jd    : A = scale sum_i aS_ij |q_id|                            B = scale sum_i eS_ij |q_id|
         dv_jd    : A = sum_i P_ij |dO_id|                                  B = 2 sum_i sc_i P_ij |dO_id|
         dbias_ij : (fp32 accumulator, fp32 output) A = sum_w aS_wij + eS_wij            B = None"""
    _, z = _window_explicit(q, k, v, bias, region, wpi, scale, go, lambda t: t, False)
    p, dp, delta = z["p"], z["dp"], z["delta"]
    sc = scale * torch.einsum("wihd,wjhd->whij", q.abs(), k.abs()) + bias.abs()[None] + (100.0 if region is not None else 0.0)
    sc = sc.max(-1, keepdim=True).values                     # (W, H, 49, 1)
    a_s = p * (dp - delta).abs()
    adp = torch.einsum("wihd,wjhd->whij", go.abs(), v.abs())
    e_s = 2 * sc * a_s + p * (adp + (1 + 2 * sc) * (p * adp).sum(-1, keepdim=True))
    ao = torch.einsum("whij,wjhd->wihd", p, v.abs())
    sct = sc.permute(0, 2, 1, 3)                             # (W, 49, H, 1)
    return dict(
        o=(ao, 2 * sct * ao),
        dq=(scale * torch.einsum("whij,wjhd->wihd", a_s, k.abs()), scale * torch.einsum("whij,wjhd->wihd", e_s, k.abs())),
        dk=(scale * torch.einsum("whij,wihd->wjhd", a_s, q.abs()), scale * torch.einsum("whij,wihd->wjhd", e_s, q.abs())),
        dv=(torch.einsum("whij,wihd->wjhd", p, go.abs()), 2 * torch.einsum("whij,wihd->wjhd", p * sc, go.abs())),
        dbias=((a_s + e_s).sum(0), None))


# ------------------------------------------------------------------------------------------------- class-token attention
def token_ref64(q, k, v, scale, go):
    """q, go (W, 49, H, 4), k, v (W, 49, H, e): A = softmax_c(scale sum_n q[n][r] k[n][c]), o[n][r] = sum_c A[r][c] v[n][c]."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    a = torch.softmax(scale * torch.einsum("wnhr,wnhc->whrc", q, k), -1)
    o = torch.einsum("whrc,wnhc->wnhr", a, v)
    g = torch.autograd.grad(o, [q, k, v], go)
    return dict(o=o.detach(), dq=g[0], dk=g[1], dv=g[2])


def token_pair_ref64(q, q2, k, v, scale, go, go2):
    a, b = token_ref64(q, k, v, scale, go), token_ref64(q2, k, v, scale, go2)
    return dict(o=a["o"], o2=b["o"], dq=a["dq"], dq2=b["dq"], dk=a["dk"] + b["dk"], dv=a["dv"] + b["dv"])


def _token_explicit(q, k, v, scale, go, r, alt):
    s = scale * torch.einsum("wnhr,wnhc->whrc", _flip(q, 1, alt), _flip(k, 1, alt))
    pu = torch.exp(s - s.max(-1, keepdim=True).values)
    a = pu / _flip(pu, 3, alt).sum(-1, keepdim=True)         # normalised in fp32, THEN the bf16 operand
    o = r(torch.einsum("whrc,wnhc->wnhr", _flip(r(a), 3, alt), _flip(v, 3, alt)))
    da = torch.einsum("wnhc,wnhr->whrc", _flip(v, 1, alt), _flip(go, 1, alt))
    dot = _flip(a * da, 3, alt).sum(-1, keepdim=True)
    ds = a * (da - dot)
    dq = r(scale * torch.einsum("whrc,wnhc->wnhr", _flip(r(ds), 3, alt), _flip(k, 3, alt)))
    dk_acc = torch.einsum("whrc,wnhr->wnhc", _flip(r(ds), 2, alt), _flip(q, 3, alt))     # fp32 accumulators: the pair kernel sums both
    dv_acc = torch.einsum("whrc,wnhr->wnhc", _flip(r(a), 2, alt), _flip(go, 3, alt))     # tokens' rows here, before the one rounding
    return dict(o=o, dq=dq, dk_acc=scale * dk_acc, dv_acc=dv_acc), dict(a=a, da=da, ds=ds, dot=dot)


def token_model(q, k, v, scale, go, rounding=True):
    f = lambda t: t.float()
    r = rb if rounding else (lambda t: t)
    m = _token_explicit(f(q), f(k), f(v), scale, f(go), r, not rounding)[0]
    return dict(o=m["o"], dq=m["dq"], dk=r(m["dk_acc"]), dv=r(m["dv_acc"]))


def token_pair_model(q, q2, k, v, scale, go, go2, rounding=True):
    f = lambda t: t.float()
    r = rb if rounding else (lambda t: t)
    a = _token_explicit(f(q), f(k), f(v), scale, f(go), r, not rounding)[0]
    b = _token_explicit(f(q2), f(k), f(v), scale, f(go2), r, not rounding)[0]
    return dict(o=a["o"], o2=b["o"], dq=a["dq"], dq2=b["dq"], dk=r(a["dk_acc"] + b["dk_acc"]), dv=r(a["dv_acc"] + b["dv_acc"]))


def token_cond(q, k, v, scale, go):
    """sc_r   = max_c scale sum_n |q[n][r]| |k[n][c]|
       o[n][r]  : A = sum_c A[r][c] |v[n][c]|                               B = 2 sc_r A
       dA[r][c] = sum_n v[n][c] dO[n][r], adA likewise with absolute values;  aS = A |dA - dot|
       eS[r][c] = 2 sc_r aS + A (adA + (1 + 2 sc_r) sum_c' A[r][c'] adA[r][c'])
       dq[n][r] : A = scale sum_c aS[r][c] |k[n][c]|                        B = scale sum_c eS[r][c] |k[n][c]|
       dk[n][c] : A = scale sum_r aS[r][c] |q[n][r]|                        B = scale sum_r eS[r][c] |q[n][r]|
       dv[n][c] : A = sum_r A[r][c] |dO[n][r]|                              B = 2 sum_r sc_r A[r][c] |dO[n][r]|"""
    _, z = _token_explicit(q, k, v, scale, go, lambda t: t, False)
    a, da, dot = z["a"], z["da"], z["dot"]
    sc = (scale * torch.einsum("wnhr,wnhc->whrc", q.abs(), k.abs())).max(-1, keepdim=True).values      # (W, H, 4, 1)
    a_s = a * (da - dot).abs()
    ada = torch.einsum("wnhc,wnhr->whrc", v.abs(), go.abs())
    e_s = 2 * sc * a_s + a * (ada + (1 + 2 * sc) * (a * ada).sum(-1, keepdim=True))
    ao = torch.einsum("whrc,wnhc->wnhr", a, v.abs())
    return dict(
        o=(ao, 2 * sc[..., 0][:, None] * ao),
        dq=(scale * torch.einsum("whrc,wnhc->wnhr", a_s, k.abs()), scale * torch.einsum("whrc,wnhc->wnhr", e_s, k.abs())),
        dk=(scale * torch.einsum("whrc,wnhr->wnhc", a_s, q.abs()), scale * torch.einsum("whrc,wnhr->wnhc", e_s, q.abs())),
        dv=(torch.einsum("whrc,wnhr->wnhc", a, go.abs()), 2 * torch.einsum("whrc,wnhr->wnhc", a * sc, go.abs())))


def token_pair_cond(q, q2, k, v, scale, go, go2):
    a, b = token_cond(q, k, v, scale, go), token_cond(q2, k, v, scale, go2)
    add = lambda x, y: (x[0] + y[0], x[1] + y[1])
    return dict(o=a["o"], o2=b["o"], dq=a["dq"], dq2=b["dq"], dk=add(a["dk"], b["dk"]), dv=add(a["dv"], b["dv"]))


# ------------------------------------------------------------------------------------------------------ DETR MHA core
def _heads(t, H):
    B, T, E = t.shape
    return t.reshape(B, T, H, E // H).transpose(1, 2)         # (B, H, T, hd)


def _merge(t):
    B, H, T, hd = t.shape
    return t.transpose(1, 2).reshape(B, T, H * hd)


def mha_ref64(q, k, v, H, kpm, mult, scale, go):
    """q, go (B, L, E), k, v (B, S, E) fp64, kpm (B, S) bool (True = padding) or None, mult (B, H, L, S) fp64 dropout multipliers
    or None -> o (B, L, E) merged heads, lse (B, H, L), dq, dk, dv.  A row with every key masked is NaN here and is left out of
    every case: the model never produces one."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    s = scale * _heads(q, H) @ _heads(k, H).transpose(-1, -2)
    if kpm is not None:
        s = s.masked_fill(kpm.bool()[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    o = _merge((p if mult is None else p * mult) @ _heads(v, H))
    g = torch.autograd.grad(o, [q, k, v], go)
    return dict(o=o.detach(), lse=torch.logsumexp(s, -1).detach(), dq=g[0], dk=g[1], dv=g[2])


def _mha_parts(q, k, v, H, kpm, mult, scale, go):
    qh, kh, vh, gh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(go, H)
    s = scale * qh @ kh.transpose(-1, -2)
    if kpm is not None:
        s = s.masked_fill(kpm.bool()[:, None, None, :], float("-inf"))
    return qh, kh, vh, gh, s


def mha_model(q, k, v, H, kpm, mult, scale, go, rounding=True):
    """mha_fwd_kernel / mha_bwd_kernel of mfattn.hip: online softmax over 32-key tiles (P relative to the RUNNING maximum is the bf16
    operand, O and l rescaled by alpha between tiles), LSE = m + log l; the backward recomputes P = exp(S - LSE) in fp32, takes
    delta = dO . O from the STORED bf16 O, and rounds dS (for dQ, dK) and P x multiplier (for dV) to bf16.
    rounding=False: the unfused fp32 path (gwd_bmm -> softmax -> gwd_bmm) with reversed reduction order."""
    f = lambda t: t.float()
    q, k, v, go = f(q), f(k), f(v), f(go)
    mult = None if mult is None else f(mult)
    alt = not rounding
    r = rb if rounding else (lambda t: t)
    qh, kh, vh, gh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(go, H)
    B, _, L, hd = qh.shape
    S = kh.shape[2]
    s = scale * _flip(qh, 3, alt) @ _flip(kh, 3, alt).transpose(-1, -2)
    masked = None if kpm is None else kpm.bool()[:, None, None, :].expand(B, H, L, S)
    if rounding:
        m = torch.full((B, H, L, 1), -1e30)
        l = torch.zeros(B, H, L, 1)
        ot = torch.zeros(B, H, L, hd)
        neg = float(torch.tensor(-1e30).bfloat16())          # the mask k-step adds bf16(-1e30) to the fp32 score
        for t0 in range(0, S, 32):
            a = s[..., t0:t0 + 32]
            if masked is not None:
                a = torch.where(masked[..., t0:t0 + 32], a + neg, a)
            mn = torch.maximum(m, a.max(-1, keepdim=True).values)
            alpha = torch.exp(m - mn)
            p = torch.exp(a - mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            m = mn
            if mult is not None:
                p = p * mult[..., t0:t0 + 32]
            ot = ot * alpha + r(p) @ vh[:, :, t0:t0 + 32]
        oh = r(ot / l)
        lse = (m + torch.log(l))[..., 0]
        sm = s if masked is None else s.masked_fill(masked, float("-inf"))
        p = torch.exp(sm - lse[..., None])
    else:
        sm = s if masked is None else s.masked_fill(masked, float("-inf"))
        mx = sm.max(-1, keepdim=True).values
        pu = torch.exp(sm - mx)
        l = _flip(pu, 3, alt).sum(-1, keepdim=True)
        p = pu / l
        lse = (mx + torch.log(l))[..., 0]
        oh = _flip(p if mult is None else p * mult, 3, alt) @ _flip(vh, 2, alt)
    pd = p if mult is None else p * mult
    dp = _flip(gh, 3, alt) @ _flip(vh, 3, alt).transpose(-1, -2)
    if mult is not None:
        dp = dp * mult
    if rounding:
        delta = (gh * oh).sum(-1, keepdim=True)              # mha_delta_kernel: dO . O with the stored bf16 O
    else:
        delta = _flip(p * dp, 3, alt).sum(-1, keepdim=True)  # softmax backward of the unfused path
    ds = p * (dp - delta)
    dq = r(scale * _flip(r(ds), 3, alt) @ _flip(kh, 2, alt))
    dk = r(scale * _flip(r(ds), 2, alt).transpose(-1, -2) @ _flip(qh, 2, alt))
    dv = r(_flip(r(pd), 2, alt).transpose(-1, -2) @ _flip(gh, 2, alt))
    return dict(o=_merge(oh), lse=lse, dq=_merge(dq), dk=_merge(dk), dv=_merge(dv))


def mha_cond(q, k, v, H, kpm, mult, scale, go):
    """m_ij the dropout multiplier (1 without dropout), P the softmax BEFORE dropout:
         sc_i    = max_j scale sum_d |q_id| |k_jd|  over the unmasked keys
         o_id    : A = sum_j P_ij m_ij |v_jd|                              B = 2 sc_i A
         lse_i   : (fp32 output) A = sc_i + 1                              (the scores' terms; log l, l in [1, S])
         dP_ij   = m_ij sum_d dO_id v_jd, adP_ij = m_ij sum_d |dO_id| |v_jd|;  delta_i = sum_j P_ij dP_ij = dO_i . O_i
         aS_ij   = P_ij |dP_ij - delta_i|
         eO_i    = sum_d |dO_id| (|o_id| + A[o_id])        the bf16 kernel takes delta from the STORED bf16 O: its rounding
                                                           and the rounding of P inside it reach every dS_ij of the row as P_ij eO_i
         eS_ij   = 2 sc_i aS_ij + P_ij (adP_ij + (1 + 2 sc_i) sum_j' P_ij' adP_ij')      fp32 error of dS in units of 2^-24
         dq_id   : A = scale sum_j (aS_ij + P_ij eO_i) |k_jd|              B = scale sum_j eS_ij |k_jd|
         dk_jd   : A = scale sum_i (aS_ij + P_ij eO_i) |q_id|              B = scale sum_i eS_ij |q_id|
         dv_jd   : A = sum_i P_ij m_ij |dO_id|                             B = 2 sum_i sc_i P_ij m_ij |dO_id|
    Masked keys have P = 0: every term of their dk / dv is zero and the kernel must give exact zeros."""
    qh, kh, vh, gh, s = _mha_parts(q, k, v, H, kpm, mult, scale, go)
    p = torch.softmax(s, -1)
    mm = torch.ones_like(p) if mult is None else mult
    sc = scale * qh.abs() @ kh.abs().transpose(-1, -2)
    if kpm is not None:
        sc = sc.masked_fill(kpm.bool()[:, None, None, :], 0.0)
    sc = sc.max(-1, keepdim=True).values
    ao = (p * mm) @ vh.abs()
    oh = (p * mm) @ vh
    dp = mm * (gh @ vh.transpose(-1, -2))
    adp = mm * (gh.abs() @ vh.abs().transpose(-1, -2))
    delta = (p * dp).sum(-1, keepdim=True)
    a_s = p * (dp - delta).abs()
    e_o = (gh.abs() * (oh.abs() + ao)).sum(-1, keepdim=True)
    e_s = 2 * sc * a_s + p * (adp + (1 + 2 * sc) * (p * adp).sum(-1, keepdim=True))
    a_t = a_s + p * e_o
    return dict(
        o=(_merge(ao), _merge(2 * sc * ao)),
        lse=((sc + 1.0)[..., 0], None),
        dq=(_merge(scale * a_t @ kh.abs()), _merge(scale * e_s @ kh.abs())),
        dk=(_merge(scale * a_t.transpose(-1, -2) @ qh.abs()), _merge(scale * e_s.transpose(-1, -2) @ qh.abs())),
        dv=(_merge((p * mm).transpose(-1, -2) @ gh.abs()), _merge(2 * (p * mm * sc).transpose(-1, -2) @ gh.abs())))


# ---------------------------------------------------------------------------------------------------------- row softmax
def softmax_ref64(x, gy, scale=1.0, key_mask=None, rows_per_mask=1):
    """y = softmax(scale x (+ -inf where key_mask)) over the last dim, gx = scale y (gy - sum y gy); x, gy (rows, L) fp64;
    key_mask (rows / rows_per_mask, L) bool."""
    x = x.detach().clone().requires_grad_(True)
    s = x * scale
    if key_mask is not None:
        s = s.masked_fill(key_mask.bool().repeat_interleave(rows_per_mask, 0), float("-inf"))
    y = torch.softmax(s, -1)
    (gx,) = torch.autograd.grad(y, x, gy)
    return dict(y=y.detach(), gx=gx)


def softmax_backward_ref64(y, gy, scale=1.0):
    """The backward kernels' own contract: they take the STORED y."""
    return scale * y * (gy - (y * gy).sum(-1, keepdim=True))


def softmax_cond(x, gy, scale=1.0, key_mask=None, rows_per_mask=1, y_stored=None):
    """y_j   : A = 0 (one rounding of the result: the |ref| term)            B = 2 y_j max_j |scale x_j| + y_j      (exp argument, sum l)
       gx_j  : from the stored y:  A = |scale| y_j sum_j' y_j' |gy_j'|  +  |scale| y_j |gy_j - sum y gy|     (y is stored in the output
               type: its rounding reaches the row sum and the product)       B = the same (fp32 sum and products)"""
    s = x * scale
    if key_mask is not None:
        s = s.masked_fill(key_mask.bool().repeat_interleave(rows_per_mask, 0), float("-inf"))
    y = torch.softmax(s, -1) if y_stored is None else y_stored
    big = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
    dot = (y * gy).sum(-1, keepdim=True)
    ag = abs(scale) * y * ((y * gy.abs()).sum(-1, keepdim=True) + (gy - dot).abs())
    return dict(y=(torch.zeros_like(y), y * (2 * big + 1)), gx=(ag, ag))


def softmax_model(x, gy, scale=1.0, key_mask=None, rows_per_mask=1, out_dtype=torch.float32):
    """fp32 arithmetic, reversed summation, the result stored in out_dtype; the backward reads the stored y."""
    xf = x.float() * scale
    if key_mask is not None:
        xf = xf.masked_fill(key_mask.bool().repeat_interleave(rows_per_mask, 0), float("-inf"))
    e = torch.exp(xf - xf.max(-1, keepdim=True).values)
    y = (e / torch.flip(e, (1,)).sum(-1, keepdim=True)).to(out_dtype)
    yf, g = y.float(), gy.float()
    gx = (scale * yf * (g - torch.flip(yf * g, (1,)).sum(-1, keepdim=True))).to(out_dtype)
    return dict(y=y, gx=gx)


# ------------------------------------------------------------------------------------------------------ reference points
def ref_scores_ref64(q, ref_k, B, scale, g):
    """q (B*nwin, 49, H, hd), ref_k (B, R, H*hd) -> ra (B, nwin*49, R, H) = scale q . ref_k per head; g the gradient of ra."""
    W, _, H, hd = q.shape
    R = ref_k.shape[1]
    q, ref_k = q.detach().clone().requires_grad_(True), ref_k.detach().clone().requires_grad_(True)
    ra = scale * torch.einsum("bthd,brhd->btrh", q.reshape(B, -1, H, hd), ref_k.reshape(B, R, H, hd))
    gq, gk = torch.autograd.grad(ra, [q, ref_k], g)
    return dict(ra=ra.detach(), dq=gq, dk=gk)


def ref_scores_cond(q, ref_k, B, scale, g):
    """Plain fp32 sums, one rounding of the result:  ra: B = scale sum_d |q| |ref_k|;  dq: B = scale sum_r |g| |ref_k|  (A = 0);
    dk (fp32 output): A = scale sum_t |g| |q|."""
    W, _, H, hd = q.shape
    R = ref_k.shape[1]
    qa, ka, ga = q.abs().reshape(B, -1, H, hd), ref_k.abs().reshape(B, R, H, hd), g.abs()
    ra = scale * torch.einsum("bthd,brhd->btrh", qa, ka)
    dq = (scale * torch.einsum("btrh,brhd->bthd", ga, ka)).reshape(q.shape)
    dk = (scale * torch.einsum("btrh,bthd->brhd", ga, qa)).reshape(ref_k.shape)
    return dict(ra=(torch.zeros_like(ra), ra), dq=(torch.zeros_like(dq), dq), dk=(dk, None))


def ref_mix_ref64(ra, ref_v, H, g):
    """ra (B, T, R, H), ref_v (B, R, H*hd) -> q_new (B, T, H*hd) = softmax_r(ra) . ref_v per head."""
    B, T, R, _ = ra.shape
    ra, ref_v = ra.detach().clone().requires_grad_(True), ref_v.detach().clone().requires_grad_(True)
    a = torch.softmax(ra, 2)
    out = torch.einsum("btrh,brhd->bthd", a, ref_v.reshape(B, R, H, -1)).reshape(B, T, -1)
    d_ra, dv = torch.autograd.grad(out, [ra, ref_v], g)
    return dict(q_new=out.detach(), att=a.detach(), d_ra=d_ra, dv=dv)


def ref_scores_model(q, ref_k, B, scale, g, out_dtype):
    """refattn.hip: fp32 sums (here over the reversed axis), ra and dq stored in the operand type, d ref_k in fp32."""
    W, _, H, hd = q.shape
    R_ = ref_k.shape[1]
    qf, kf, gf = q.float().reshape(B, -1, H, hd), ref_k.float().reshape(B, R_, H, hd), g.float()
    ra = scale * torch.einsum("bthd,brhd->btrh", torch.flip(qf, (3,)), torch.flip(kf, (3,)))
    dq = scale * torch.einsum("btrh,brhd->bthd", torch.flip(gf, (2,)), torch.flip(kf, (1,)))
    dk = scale * torch.einsum("btrh,bthd->brhd", torch.flip(gf, (1,)), torch.flip(qf, (1,)))
    return dict(ra=ra.to(out_dtype), dq=dq.reshape(q.shape).to(out_dtype), dk=dk.reshape(ref_k.shape))


def ref_mix_backward_ref64(att, ref_v, H, g):
    """The backward kernels' contract: from the STORED att.  d_ra = att (dA - sum_r att dA), dA = g . ref_v;  dv = sum_t att g."""
    B, T, R_, _ = att.shape
    gh, vh = g.reshape(B, T, H, -1), ref_v.reshape(B, R_, H, -1)
    da = torch.einsum("bthd,brhd->btrh", gh, vh)
    return dict(d_ra=att * (da - (att * da).sum(2, keepdim=True)), dv=torch.einsum("btrh,bthd->brhd", att, gh).reshape(ref_v.shape))


def ref_mix_cond(ra, ref_v, H, g, att_stored):
    """att    : one rounding (|ref|);                                         B = att (2 max_r |ra| + 1)
       q_new  : the fp32 att is the operand: A = 0                            B = (2 max_r |ra| + 2) sum_r att |v|
       d_ra   : exact stored att: A = 0;   B = att (adA + sum_r att adA) + |d_ra|,  adA = |g| . |ref_v|
       dv     : fp32 output: A = sum_t att |g|"""
    B, T, R_, _ = ra.shape
    a = torch.softmax(ra, 2)
    big = ra.abs().max(2, keepdim=True).values
    vh, gh = ref_v.reshape(B, R_, H, -1), g.reshape(B, T, H, -1)
    aq = torch.einsum("btrh,brhd->bthd", a, vh.abs())
    ada = torch.einsum("bthd,brhd->btrh", gh.abs(), vh.abs())
    bw = ref_mix_backward_ref64(att_stored, ref_v, H, g)
    z = torch.zeros_like
    return dict(att=(z(a), a * (2 * big + 1)), q_new=(z(aq).reshape(B, T, -1), ((2 * big[:, :, 0, :, None] + 2) * aq).reshape(B, T, -1)),
                d_ra=(z(a), att_stored * (ada + (att_stored * ada).sum(2, keepdim=True)) + bw["d_ra"].abs()),
                dv=(torch.einsum("btrh,bthd->brhd", att_stored, gh.abs()).reshape(ref_v.shape), None))


def ref_mix_model(ra, ref_v, H, g, out_dtype):
    B, T, R_, _ = ra.shape
    x = ra.float()
    e = torch.exp(x - x.max(2, keepdim=True).values)
    a = e / torch.flip(e, (2,)).sum(2, keepdim=True)
    vh, gh = ref_v.float().reshape(B, R_, H, -1), g.float().reshape(B, T, H, -1)
    q_new = torch.einsum("btrh,brhd->bthd", torch.flip(a, (2,)), torch.flip(vh, (1,))).reshape(B, T, -1)
    att = a.to(out_dtype)
    af = att.float()
    da = torch.einsum("bthd,brhd->btrh", torch.flip(gh, (3,)), torch.flip(vh, (3,)))
    d_ra = af * (da - torch.flip(af * da, (2,)).sum(2, keepdim=True))
    dv = torch.einsum("btrh,bthd->brhd", torch.flip(af, (1,)), torch.flip(gh, (1,))).reshape(ref_v.shape)
    return dict(att=att, q_new=q_new.to(out_dtype), d_ra=d_ra.to(out_dtype), dv=dv)


# ------------------------------------------------------------------------------------------------------------ constants
# C[operation][dtype name][output]: twice the largest model ratio over the case matrix (see the module docstring), one decimal up.
C = {
    "mha": {"bf16": dict(dk=2.2, dq=1.3, dv=3.7, lse=4.1, o=3.2), "f32": dict(dk=0.7, dq=0.8, dv=2.0, lse=4.4, o=2.5)},
    "ref_mix": {"bf16": dict(att=4.0, d_ra=4.0, dv=6.9, q_new=4.0), "f32": dict(att=2.1, d_ra=4.6, dv=9.2, q_new=1.6)},
    "ref_scores": {"bf16": dict(dk=2.8, dq=4.0, ra=4.0), "f32": dict(dk=6.4, dq=5.8, ra=5.5)},
    "softmax": {"bf16": dict(gx=2.0, y=4.0), "f32": dict(gx=3.7, y=3.2)},
    "token": {"bf16": dict(dk=3.9, dq=3.6, dv=4.0, o=3.6), "f32": dict(dk=1.4, dq=1.0, dv=5.3, o=3.0)},
    "token_pair": {"bf16": dict(dk=3.9, dq=3.6, dq2=3.6, dv=3.8, o=3.6, o2=3.6)},
    "window": {"bf16": dict(dbias=1.5, dk=3.7, dq=3.7, dv=3.9, o=3.5), "f32": dict(dbias=1.4, dk=0.8, dq=1.1, dv=2.4, o=2.8)},
}


def dtype_name(dtype):
    return {torch.bfloat16: "bf16", torch.float32: "f32"}[dtype]

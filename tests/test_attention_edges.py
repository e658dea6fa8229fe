"""GPU: the attention kernels against fp64 references, element by element, on hard logits, hard masks and edge sizes.

Every case (tests/attn_cases.py) is built on the CPU from a seed, its regime's property is asserted on the fp64 scores, and every
output the kernels write - forward, log-sum-exp, all gradients - must satisfy  |got - ref| <= c u (|ref| + cond)  for EVERY element
(tests/attn_ref.py: the references, the cond expressions and how each c was measured on the CPU, never against a kernel).  Outputs
live inside larger sentinel-filled buffers (one slot of a packed (nwin, 49, 3, H, hd) tensor, one half of a packed q|k gradient, a
window / rows after the last one) and everything outside the target must keep its bits.

bf16 runs the matrix-core kernels of csrc/mfattn.hip; fp32 the lane-per-row kernels of winattn.hip / tokattn.hip and, for the DETR
attention core, the unfused path of model.MultiheadAttention (ops.matmul_nt -> ops.attention_softmax -> ops.matmul_nn).

A query row with EVERY key masked is NaN in the reference and never occurs in the model (an image always has un-padded pixels):
no case has one."""
import pytest
import torch

from gw_depth_amd import hip, ops
from tests import attn_cases as K
from tests import attn_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "f32"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    return hip.library()


def cu(t, dtype):
    return t.to(dtype).cuda()


class Guarded:
    """A sentinel-filled buffer with a target view inside it; check() demands bit-equality of everything outside the target."""
    SENT = {torch.bfloat16: -1.5e38, torch.float32: -3.0e38}

    def __init__(self, shape, dtype, pick, zero=False):
        self.buf = torch.full(shape, self.SENT[dtype], dtype=dtype, device="cuda")
        self.bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.fill = self.buf.view(self.bits).flatten()[0].clone()
        self.t = pick(self.buf)
        marker = torch.zeros(shape, dtype=torch.bool, device="cuda")
        pick(marker).fill_(True)
        self.target = marker
        if zero:
            self.t.zero_()

    def check(self, what):
        wrong = (self.buf.view(self.bits) != self.fill) & ~self.target
        if bool(wrong.any()):
            raise AssertionError("%s: %d elements outside the target were written, first at index %s of the %s buffer"
                                 % (what, int(wrong.sum()), torch.nonzero(wrong)[0].tolist(), list(self.buf.shape)))
        unwritten = (self.buf.view(self.bits) == self.fill) & self.target
        assert not bool(unwritten.any()), "%s: %d target elements were never written, first at index %s" % (
            what, int(unwritten.sum()), torch.nonzero(unwritten)[0].tolist())


def flat_guard(shape, dtype, zero=False, pad=64):
    """A contiguous tensor of `shape` with `pad` sentinel elements before and after it."""
    n = 1
    for s in shape:
        n *= s
    return Guarded((n + 2 * pad,), dtype, lambda b: b[pad:pad + n].view(shape), zero=zero)


def compare(op, dtype, got, ref, cond, names, case, u_of=None):
    """Every output of one case; returns the worst ratios (printed, so that a run kept in a file shows every figure)."""
    cs = R.C[op][R.dtype_name(dtype)]
    worst, errors = {}, []
    for o in got:
        u = (u_of or {}).get(o, R.unit_roundoff(dtype))
        try:
            worst[o] = R.assert_elementwise(got[o], ref[o], cond[o], cs[o.split(":")[0]], names[o.split(":")[0]], u=u,
                                            what="%s %s %s %s" % (op, R.dtype_name(dtype), case, o))
        except AssertionError as e:
            errors.append(str(e))
    print("%s %s %s: worst ratio / c  %s" % (op, R.dtype_name(dtype), case,
                                           "  ".join("%s %.2f/%.1f" % (o, w, cs[o.split(":")[0]]) for o, w in worst.items())))
    assert not errors, "\n".join(errors)


# ------------------------------------------------------------------------------------------------------ window attention
WIN_NAMES = dict(o=("window", "token", "head", "channel"), dq=("window", "token", "head", "channel"), dk=("window", "token", "head", "channel"),
                 dv=("window", "token", "head", "channel"), dbias=("head", "query", "key"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(K.WINDOW_CASES))
def test_window_attention_elementwise(dev, name, dtype):
    """gwd_winattn_forward / _backward as ops._WinAttnPackedFn calls them: q, k, v are the slots of ONE packed (nwin, 49, 3, H, hd)
    projection; the output goes to slot 1 of a sentinel-filled packed buffer with one extra window, the three gradients to the slots
    of another; the bias gradient (dense, table, or the head-major table scratch for head_dim 8 / 16) accumulates into a zeroed
    span between sentinels.  Labels: model.shift_regions (0..8, windows with 1, 2 and 4 labels) and a synthetic map with 9..15,
    which the one-hot k-step must serve as well (the ABI promises 0..15)."""
    c = K.window_case(name, dtype)
    K.check_window_regime(c)
    nwin, H, hd, wpi, scale = c["nwin"], c["H"], c["hd"], c["wpi"], c["scale"]
    a = (c["q"], c["k"], c["v"], c["bias"], c["region"], wpi, scale, c["go"])
    ref, cond = R.window_ref64(*a), R.window_cond(*a)
    qkv = cu(torch.stack([c["q"], c["k"], c["v"]], 2), dtype)
    go = cu(c["go"], dtype)
    region = None if c["region"] is None else c["region"].cuda()
    table = c["table"] is not None
    rel = c["rel"].reshape(-1).contiguous().cuda() if table else None
    bias = cu(c["table"] if table else c["bias"], torch.float32).contiguous()
    out = Guarded((nwin + 1, 49, 3, H, hd), dtype, lambda b: b[:nwin, :, 1])
    dev.winattn_forward(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], out.t, bias, region, wpi, scale, rel_index=rel)
    g = Guarded((nwin + 1, 49, 3, H, hd), dtype, lambda b: b[:nwin])
    hm = table and hd in (8, 16)
    db = flat_guard((H, 169) if hm else tuple(bias.shape), torch.float32, zero=True)
    dev.winattn_backward(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], go, g.t[:, :, 0], g.t[:, :, 1], g.t[:, :, 2], bias, db.t, region, wpi, scale,
                         rel_index=rel, head_major=hm)
    torch.cuda.synchronize()
    out.check(name + " o")
    g.check(name + " gradients")
    db.check(name + " dbias")
    got = dict(o=out.t, dq=g.t[:, :, 0], dk=g.t[:, :, 1], dv=g.t[:, :, 2], dbias=db.t.t() if hm else db.t)
    names = dict(WIN_NAMES)
    if table:
        tg = lambda x: None if x is None else R.table_grad(x, c["rel"], 169)
        ref["dbias"], cond["dbias"] = tg(ref["dbias"]), tuple(tg(x) for x in cond["dbias"])
        names["dbias"] = ("table row", "head")
    compare("window", dtype, got, ref, cond, names, name, u_of=dict(dbias=R.U_F32))


# ------------------------------------------------------------------------------------------------- class-token attention
TOK_NAMES = {k: ("window", "token", "head", "channel") for k in ("o", "o2", "dq", "dq2", "dk", "dv")}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(K.TOKEN_CASES))
def test_token_attention_elementwise(dev, name, dtype):
    """gwd_tokattn_forward / _backward: q (nwin, 49, H, 4) against the k / v slots of a packed (nwin, 49, 2, H, e) tensor; outputs and
    query gradients in the lower 4 channels of 8-channel sentinel rows, k / v gradients in a packed buffer with one extra window."""
    c = K.token_case(name, dtype)
    K.check_token_regime(c)
    nwin, H, e, scale = c["nwin"], c["H"], c["e"], c["scale"]
    a = (c["q"], c["k"], c["v"], scale, c["go"])
    ref, cond = R.token_ref64(*a), R.token_cond(*a)
    q, go, kv = cu(c["q"], dtype), cu(c["go"], dtype), cu(torch.stack([c["k"], c["v"]], 2), dtype)
    o = Guarded((nwin + 1, 49, H, 8), dtype, lambda b: b[:nwin, :, :, :4])
    gq = Guarded((nwin + 1, 49, H, 8), dtype, lambda b: b[:nwin, :, :, :4])
    gkv = Guarded((nwin + 1, 49, 2, H, e), dtype, lambda b: b[:nwin])
    dev.tokattn_forward(q, kv[:, :, 0], kv[:, :, 1], o.t, scale)
    dev.tokattn_backward(q, kv[:, :, 0], kv[:, :, 1], go, gq.t, gkv.t[:, :, 0], gkv.t[:, :, 1], scale)
    torch.cuda.synchronize()
    for gbuf, what in ((o, "o"), (gq, "dq"), (gkv, "dk / dv")):
        gbuf.check(name + " " + what)
    compare("token", dtype, dict(o=o.t, dq=gq.t, dk=gkv.t[:, :, 0], dv=gkv.t[:, :, 1]), ref, cond, TOK_NAMES, name)


@pytest.mark.parametrize("name", list(K.TOKEN_CASES))
def test_token_attention_pair_elementwise(dev, name):
    """gwd_tokattn_pair_*: both class tokens in one launch (bf16), k / v gradients summed in the accumulators before the one rounding."""
    dtype = torch.bfloat16
    c = K.token_case(name, dtype)
    nwin, H, e, scale = c["nwin"], c["H"], c["e"], c["scale"]
    a = (c["q"], c["q2"], c["k"], c["v"], scale, c["go"], c["go2"])
    ref, cond = R.token_pair_ref64(*a), R.token_pair_cond(*a)
    q, q2, go, go2 = (cu(c[n], dtype) for n in ("q", "q2", "go", "go2"))
    kv = cu(torch.stack([c["k"], c["v"]], 2), dtype)
    # o | o2 and gq | gq2 side by side in 8-channel rows: each call's target is one half, the pair fills both
    o = Guarded((nwin + 1, 49, H, 8), dtype, lambda b: b[:nwin])
    gq = Guarded((nwin + 1, 49, H, 8), dtype, lambda b: b[:nwin])
    gkv = Guarded((nwin + 1, 49, 2, H, e), dtype, lambda b: b[:nwin])
    assert dev.tokattn_pair_forward(q, q2, kv[:, :, 0], kv[:, :, 1], o.t[..., :4], o.t[..., 4:], scale) is not False
    assert dev.tokattn_pair_backward(q, q2, kv[:, :, 0], kv[:, :, 1], go, go2, gq.t[..., :4], gq.t[..., 4:], gkv.t[:, :, 0], gkv.t[:, :, 1],
                                     scale) is not False
    torch.cuda.synchronize()
    for gbuf, what in ((o, "o"), (gq, "dq"), (gkv, "dk / dv")):
        gbuf.check(name + " " + what)
    got = dict(o=o.t[..., :4], o2=o.t[..., 4:], dq=gq.t[..., :4], dq2=gq.t[..., 4:], dk=gkv.t[:, :, 0], dv=gkv.t[:, :, 1])
    compare("token_pair", dtype, got, ref, cond, TOK_NAMES, name)


# --------------------------------------------------------------------------------------------------------------- MHA core
MHA_NAMES = dict(o=("batch", "query", "channel (32 head + d)"), lse=("batch", "head", "query"), dq=("batch", "query", "channel (32 head + d)"),
                 dk=("batch", "key", "channel (32 head + d)"), dv=("batch", "key", "channel (32 head + d)"))


def rows_guard(B, T, width, E, dtype, lo=0):
    """(B, T, E) target = channels lo..lo+E of the first B*T rows of a (B*T + 2, width) sentinel buffer (dense batches, as the kernels want)."""
    return Guarded((B * T + 2, width), dtype, lambda b: b[:B * T].view(B, T, width)[..., lo:lo + E])


def check_exact_zeros(c, got):
    """Gradients of a masked key and outputs / gradients of a query row whose multipliers are all 0 are exact zeros (the element-wise bound
    is zero there; asserted again by name so that the case cannot lose them unnoticed)."""
    if c["kpm"] is not None:
        m = c["kpm"].cuda()
        assert bool((got["dk"][m] == 0).all()) and bool((got["dv"][m] == 0).all())
    if c["mult"] is not None and "zero_row" in c["name"]:
        L = c["L"]
        for b, h, i in ((0, 1, L // 2), (1, 0, L - 1)):
            assert bool((got["o"][b, i, 32 * h:32 * h + 32] == 0).all()) and bool((got["dq"][b, i, 32 * h:32 * h + 32] == 0).all())


@pytest.mark.parametrize("name", list(K.MHA_CASES))
def test_mha_flash_elementwise(dev, name):
    """gwd_mha_flash_forward / _backward (bf16) as ops._MhaFlashFn calls them: packed q|k with ONE packed gradient, or separate q / k with
    every gradient in the left half of a double-width sentinel buffer; two sentinel rows after the last token; the log-sum-exp between
    sentinels.  Masks: leading / middle key tiles fully masked, a single surviving key, per-image masks, the masks of ragged image
    pairs at the 15 x 20 and 30 x 40 token maps; dropout multipliers with p = 0.1 / 0.5 and query rows with every multiplier 0."""
    dtype = torch.bfloat16
    c = K.mha_case(name, dtype)
    K.check_mha_regime(c)
    B, L, S, H, E, scale = c["B"], c["L"], c["S"], c["H"], c["E"], c["scale"]
    a = (c["q"], c["k"], c["v"], H, c["kpm"], c["mult"], scale, c["go"])
    ref, cond = R.mha_ref64(*a), R.mha_cond(*a)
    kpm = None if c["kpm"] is None else c["kpm"].cuda().view(torch.uint8)
    mult = None if c["mult"] is None else cu(c["mult"], dtype).contiguous()
    v, go = cu(c["v"], dtype), cu(c["go"], dtype)
    if c["packed"]:
        qk = cu(torch.cat([c["q"], c["k"]], -1), dtype)
        q, k = qk[..., :E], qk[..., E:]
        gqk = rows_guard(B, L, 2 * E, 2 * E, dtype)
        gq, gk, guards = gqk.t[..., :E], gqk.t[..., E:], [(gqk, "dq | dk")]
    else:
        q, k = cu(c["q"], dtype), cu(c["k"], dtype)
        gq_, gk_ = rows_guard(B, L, 2 * E, E, dtype), rows_guard(B, S, 2 * E, E, dtype, lo=E)
        gq, gk, guards = gq_.t, gk_.t, [(gq_, "dq"), (gk_, "dk")]
    out, gv = rows_guard(B, L, 2 * E, E, dtype), rows_guard(B, S, 2 * E, E, dtype)
    lse, delta = flat_guard((B, H, L), torch.float32), flat_guard((B, H, L), torch.float32)
    dev.mha_flash_forward(q, k, v, kpm, mult, out.t, lse.t, H, scale)
    dev.mha_flash_backward(q, k, v, go, out.t, kpm, mult, lse.t, delta.t, gq, gk, gv.t, H, scale)
    torch.cuda.synchronize()
    for gbuf, what in guards + [(out, "o"), (gv, "dv"), (lse, "lse"), (delta, "delta")]:
        gbuf.check(name + " " + what)
    got = dict(o=out.t, lse=lse.t, dq=gq, dk=gk, dv=gv.t)
    check_exact_zeros(c, got)
    compare("mha", dtype, got, ref, cond, MHA_NAMES, name, u_of=dict(lse=R.U_F32))


@pytest.mark.parametrize("name", list(K.MHA_CASES))
def test_mha_unfused_fp32_elementwise(dev, name):
    """The fp32 parity path of model.MultiheadAttention (model.py:257-266): ops.matmul_nt -> ops.attention_softmax (scale and key mask
    folded in) -> x multipliers -> ops.matmul_nn, gradients through the ops' own autograd nodes.  (The ops allocate their outputs: the
    guard bands of this path are those of the softmax tests below.)"""
    dtype = torch.float32
    c = K.mha_case(name, dtype)
    K.check_mha_regime(c)
    B, L, S, H, E, scale = c["B"], c["L"], c["S"], c["H"], c["E"], c["scale"]
    a = (c["q"], c["k"], c["v"], H, c["kpm"], c["mult"], scale, c["go"])
    ref, cond = R.mha_ref64(*a), R.mha_cond(*a)
    q, k, v = (cu(c[n], dtype).requires_grad_(True) for n in ("q", "k", "v"))
    kpm = None if c["kpm"] is None else c["kpm"].cuda()
    qh, kh, vh = (t.reshape(B, -1, H, 32).transpose(1, 2) for t in (q, k, v))
    att = ops.attention_softmax(ops.matmul_nt(qh, kh), kpm, scale)
    if c["mult"] is not None:
        att = att * cu(c["mult"], dtype)
    o = ops.matmul_nn(att, vh).transpose(1, 2).reshape(B, L, E)
    gq, gk, gv = torch.autograd.grad(o, [q, k, v], cu(c["go"], dtype))
    torch.cuda.synchronize()
    got = dict(o=o.detach(), dq=gq, dk=gk, dv=gv)
    check_exact_zeros(c, got)
    compare("mha", dtype, got, ref, cond, MHA_NAMES, name)


# ------------------------------------------------------------------------------------------------------ reference points
REF_NAMES = dict(ra=("image", "token", "reference", "head"), dq=("window", "token", "head", "channel"), dk=("image", "reference", "channel"),
                 att=("image", "token", "reference", "head"), q_new=("image", "token", "channel"), d_ra=("image", "token", "reference", "head"),
                 dv=("image", "reference", "channel"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(K.REF_CASES))
def test_reference_point_kernels_elementwise(dev, name, dtype):
    """gwd_ref_scores_* / gwd_ref_mix_* with R in {1, 7, 40, 128} as ops._RefScoresFn / _RefMixFn call them: q read from slot 0 of the
    packed projection, dq written to slot 0 of a sentinel-filled packed gradient (the k / v slots are another node's), everything else
    between sentinels.  The mix backward takes the STORED att and is checked against the formula on the att the forward wrote."""
    c = K.ref_case(name, dtype)
    K.check_ref_regime(c)
    B, nwin, Rn, H, hd, scale = c["B"], c["nwin"], c["R"], c["H"], c["hd"], c["scale"]
    T, W = nwin * 49, B * nwin
    a = (c["q"], c["ref_k"], B, scale, c["g_ra"])
    ref, cond = R.ref_scores_ref64(*a), R.ref_scores_cond(*a)
    qkv = torch.zeros(W, 49, 3, H, hd, dtype=dtype, device="cuda")
    qkv[:, :, 0] = cu(c["q"], dtype)
    ref_k, g_ra = cu(c["ref_k"], dtype), cu(c["g_ra"], dtype)
    ra = flat_guard((B, T, Rn, H), dtype)
    gqkv = Guarded((W + 1, 49, 3, H, hd), dtype, lambda b: b[:W, :, 0])
    dk = flat_guard((B, Rn, H * hd), torch.float32)
    dev.ref_scores_forward(qkv[:, :, 0], ref_k, ra.t, B, nwin, scale)
    dev.ref_scores_backward(qkv[:, :, 0], ref_k, g_ra, gqkv.t, dk.t, B, nwin, scale)
    torch.cuda.synchronize()
    for gbuf, what in ((ra, "ra"), (gqkv, "dq"), (dk, "d ref_k")):
        gbuf.check(name + " " + what)
    compare("ref_scores", dtype, dict(ra=ra.t, dq=gqkv.t, dk=dk.t), ref, cond, REF_NAMES, name, u_of=dict(dk=R.U_F32))

    ra2, ref_v, g_q = cu(c["ra2"], dtype), cu(c["ref_v"], dtype), cu(c["g_q"], dtype)
    q_new, att = flat_guard((B, T, H * hd), dtype), flat_guard((B, T, Rn, H), dtype)
    d_ra, dv = flat_guard((B, T, Rn, H), dtype), flat_guard((B, Rn, H * hd), torch.float32)
    dev.ref_mix_forward(ra2, ref_v, q_new.t, att.t, H)
    dev.ref_mix_backward(att.t, ref_v, g_q, d_ra.t, dv.t, H)
    torch.cuda.synchronize()
    for gbuf, what in ((q_new, "q_new"), (att, "att"), (d_ra, "d_ra"), (dv, "d ref_v")):
        gbuf.check(name + " " + what)
    a = (c["ra2"], c["ref_v"], H, c["g_q"])
    stored = att.t.double().cpu()
    ref = R.ref_mix_ref64(*a)
    ref.update(R.ref_mix_backward_ref64(stored, c["ref_v"], H, c["g_q"]))
    cond = R.ref_mix_cond(*a, att_stored=stored)
    compare("ref_mix", dtype, dict(att=att.t, q_new=q_new.t, d_ra=d_ra.t, dv=dv.t), ref, cond, REF_NAMES, name, u_of=dict(dv=R.U_F32))


# ------------------------------------------------------------------------------------------------------------ row softmax
SM_NAMES = dict(y=("row", "column"), gx=("row", "column"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked_scaled"])
def test_softmax_rows_elementwise(dev, masked, dtype):
    """gwd_softmax_forward / _backward and gwd_softmax_masked_forward / _scaled_backward over every L of the list, row counts that are
    not a multiple of the 4 rows a workgroup takes, logits up to +-80 (+-1e4 in fp32); y and gx between sentinels.  The backward
    kernels take the STORED y: they are checked against the formula on the y the forward kernel wrote."""
    for rows, L, amp in K.softmax_cases(dtype):
        c = K.softmax_case(rows, L, amp, dtype, masked)
        case = "rows %d L %d amplitude %g" % (rows, L, amp)
        x, gy = cu(c["x"], dtype), cu(c["gy"], dtype)
        y, gx = flat_guard((rows, L), dtype), flat_guard((rows, L), dtype)
        if masked:
            dev.softmax_masked_forward(x, c["mask"].cuda().view(torch.uint8), y.t, rows, L, c["rpm"], c["scale"])
            dev.softmax_scaled_backward(gy, y.t, gx.t, rows, L, c["scale"])
        else:
            dev.softmax_forward(x, y.t, rows, L)
            dev.softmax_backward(gy, y.t, gx.t, rows, L)
        torch.cuda.synchronize()
        y.check(case + " y")
        gx.check(case + " gx")
        ref = R.softmax_ref64(c["x"], c["gy"], c["scale"], c["mask"], c["rpm"])
        ys = y.t.double().cpu()
        cond = R.softmax_cond(c["x"], c["gy"], c["scale"], c["mask"], c["rpm"])
        cond["gx"] = R.softmax_cond(c["x"], c["gy"], c["scale"], c["mask"], c["rpm"], y_stored=ys)["gx"]
        ref["gx"] = R.softmax_backward_ref64(ys, c["gy"], c["scale"])
        if masked and L > 1:
            assert bool((y.t[:, : L // 2] == 0).all()), case + ": a masked key got weight"
        compare("softmax", dtype, dict(y=y.t, gx=gx.t), ref, cond, SM_NAMES, case)


# ------------------------------------------------------------------------------------------- declined calls fall back
def _misaligned(t, off):
    """A view with t's values and strides whose storage offset is `off` elements further."""
    base = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = base[off:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("how", ["offset_4_bytes", "token_stride_6"])
def test_token_attention_pair_declined_falls_back(dev, how):
    """ops.token_attention_pair on operands the pair kernels decline: a q whose storage starts 4 bytes past an 8-byte boundary, and a q
    whose token stride (H*4 + 2 elements) is not a multiple of 4.  gwd_tokattn_pair_* returns -4 from tok::run's operand check, which
    stands BEFORE the launch (csrc/mfattn.hip: the loop over s[i] at the top of run(), then the kernel call), so nothing has been
    written when ops issues the two single calls; the single calls take the same lane-per-token kernels either way, so the result is
    bit-equal to two ops.token_attention calls, forward and backward (gk / gv: the bf16 sum autograd forms from two nodes)."""
    nwin, H, e, dtype = 5, 16, 16, torch.bfloat16
    g = torch.Generator().manual_seed(7)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).cuda()
    q0, q2, k, v = mk(nwin, 49, H, 4), mk(nwin, 49, H, 4), mk(nwin, 49, H, e), mk(nwin, 49, H, e)
    w1, w2 = mk(nwin, 49, H * 4), mk(nwin, 49, H * 4)
    if how == "offset_4_bytes":
        q = _misaligned(q0, 2)
        assert q.data_ptr() % 8 == 4
    else:
        q = torch.empty(nwin, 49, H * 4 + 2, dtype=dtype, device="cuda")[..., :H * 4].view(nwin, 49, H, 4)
        q.copy_(q0)
        assert q.stride(1) % 4 == 2 and q.stride(3) == 1
    o = torch.empty(nwin, 49, H, 4, dtype=dtype, device="cuda")
    assert dev.tokattn_pair_forward(q, q2, k, v, o, torch.empty_like(o), 0.5) is False          # the library declines this call ...
    leaves = [t.detach().requires_grad_(True) for t in (q, q2, k, v)]
    a, b = ops.token_attention_pair(*leaves, 0.5)                                                # ... and ops falls back
    g_pair = torch.autograd.grad((a.float() * w1).sum() + (b.float() * w2).sum(), leaves)
    leaves1 = [t.detach().requires_grad_(True) for t in (q, q2, k, v)]
    a1, b1 = ops.token_attention(leaves1[0], leaves1[2], leaves1[3], 0.5), ops.token_attention(leaves1[1], leaves1[2], leaves1[3], 0.5)
    g_two = torch.autograd.grad((a1.float() * w1).sum() + (b1.float() * w2).sum(), leaves1)
    torch.cuda.synchronize()
    assert torch.equal(a, a1) and torch.equal(b, b1)
    for x, y_, n in zip(g_pair, g_two, ("gq", "gq2", "gk", "gv")):
        assert torch.equal(x, y_), n
    # and the fallback is right, not only consistent: element-wise against fp64
    f = lambda t: t.detach().double().cpu()
    args = (f(q), f(q2), f(k), f(v), 0.5, f(w1).view(nwin, 49, H, 4), f(w2).view(nwin, 49, H, 4))
    ref, cond = R.token_pair_ref64(*args), R.token_pair_cond(*args)
    # two nodes: gk / gv are two rounded results added in bf16 - one more rounding of the sum than the pair kernel's accumulators
    cond["dk"] = (cond["dk"][0] + ref["dk"].abs(), cond["dk"][1])
    cond["dv"] = (cond["dv"][0] + ref["dv"].abs(), cond["dv"][1])
    got = dict(o=a.view(nwin, 49, H, 4), o2=b.view(nwin, 49, H, 4), dq=g_pair[0], dq2=g_pair[1], dk=g_pair[2], dv=g_pair[3])
    compare("token_pair", dtype, got, ref, cond, TOK_NAMES, "declined " + how)


@pytest.mark.parametrize("shift", [0, 3])
def test_window_map_multi_declined_falls_back(dev, shift):
    """ops.window_gather_multi / window_scatter_multi with a token width that is not a multiple of 4 in fp32 (rows that are not whole
    16-byte vectors): gwd_window_map_multi returns -4 from the loop that validates every C[i], which stands BEFORE the launch
    (csrc/winmap.hip), ops then issues gwd_window_map per map - the same calls ops.window_gather / window_scatter make, so forward and
    backward are bit-equal to those; the per-element form of gwd_window_map is checked against the index arithmetic in torch."""
    from tests.fake_device import FakeDevice
    B, H, W, Cs = 2, 15, 20, (16, 6, 3)
    g = torch.Generator().manual_seed(3 + shift)
    xs = [torch.randn(B, H, W, c, generator=g).cuda() for c in Cs]
    ress = [torch.randn(B, H, W, Cs[0], generator=g).cuda(), None, torch.randn(B, H, W, Cs[2], generator=g).cuda()]
    nw = B * 3 * 3
    outs = [torch.empty(nw, 49, c, device="cuda") for c in Cs]
    assert dev.window_map_multi(xs, outs, B, H, W, list(Cs), shift, True) is False
    leaves = [x.clone().requires_grad_(True) for x in xs]
    rl = [None if r is None else r.clone().requires_grad_(True) for r in ress]
    wins = ops.window_gather_multi(leaves, shift)
    multi = ops.window_scatter_multi(list(wins), B, H, W, shift, rl)
    leaves1 = [x.clone().requires_grad_(True) for x in xs]
    rl1 = [None if r is None else r.clone().requires_grad_(True) for r in ress]
    wins1 = [ops.window_gather(x, shift) for x in leaves1]
    single = [ops.window_scatter(w_, B, H, W, shift, residual=r) for w_, r in zip(wins1, rl1)]
    ws = [torch.randn(B, H, W, c, generator=g).cuda() for c in Cs]
    inputs = lambda ls, rs: ls + [r for r in rs if r is not None]
    gm = torch.autograd.grad(sum((m * w_).sum() for m, w_ in zip(multi, ws)), inputs(leaves, rl))
    gs = torch.autograd.grad(sum((m * w_).sum() for m, w_ in zip(single, ws)), inputs(leaves1, rl1))
    torch.cuda.synchronize()
    for x, y_ in zip(list(wins) + list(multi) + list(gm), wins1 + single + list(gs)):
        assert torch.equal(x, y_)
    fake = FakeDevice()
    for x, wn, c in zip(xs, wins, Cs):
        want = torch.empty(nw, 49, c)
        fake.window_map(x.cpu(), want, B, H, W, c, shift, True)
        assert torch.equal(wn.detach().cpu(), want)
    for x, r, m in zip(xs, ress, multi):                     # gather then scatter is the identity on the un-padded map (+ residual)
        want = x if r is None else x + r
        assert torch.equal(m.detach(), want)
    # bf16 rows of 6 and 3 channels (12 and 6 bytes) go the same way
    xb = [x.bfloat16() for x in xs]
    wb = ops.window_gather_multi(xb, shift)
    for x, wn, c in zip(xb, wb, Cs):
        want = torch.empty(nw, 49, c, dtype=torch.bfloat16)
        fake.window_map(x.cpu(), want, B, H, W, c, shift, True)
        assert torch.equal(wn.cpu(), want)

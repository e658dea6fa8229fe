"""The case matrix of the attention edge tests: every operand is generated on the CPU from a seed, rounded to the storage type
of the kernel under test, and handed out as fp64 (tests/attn_ref.py consumes that; the GPU tests cast it back, which is exact).
The CPU tests (tests/test_attn_ref.py) size the comparator's constants over exactly these cases; the GPU tests
(tests/test_attention_edges.py) run the kernels on them."""
import torch
import torch.nn.functional as F

from gw_depth_amd import model as M
from tests import attn_ref as R

NT = 49


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def st(x, dtype):
    return R.as_storage(x, dtype)


# ------------------------------------------------------------------------------------------------------ window attention
# name: (nwin, heads, head_dim, wpi, regions, regime, bias form)
#   regions: None | ("shift", Hp, Wp) = model.shift_regions of that padded map (wpi = its window count) | "high" = labels 9..15
#   bias form: "dense" (H, 49, 49) | "table" (169, H) through relative_position_index
# 259 windows: gwd_mfattn_window caps gridDim.x at 256, so 3 workgroups walk two windows and 253 one - the last round is partly empty;
# 37 / 3 / 1 windows make gridDim.x = n_windows with most of the chip idle; 2100 is the 1/4-scale window count of a 2-image batch.
WINDOW_CASES = {
    "benign_w37_h4_d32": (37, 4, 32, 1, None, "benign", "table"),
    "benign_w1_h4_d4": (1, 4, 4, 1, None, "benign", "dense"),
    "benign_w2_h8_d8": (2, 8, 8, 1, None, "benign", "table"),
    "benign_w3_h4_d16": (3, 4, 16, 1, None, "benign", "dense"),
    "benign_w259_h4_d16": (259, 4, 16, 1, None, "benign", "table"),
    "benign_w2100_h4_d8": (2100, 4, 8, 1, None, "benign", "table"),
    "hot_last_w37_h4_d32": (37, 4, 32, 1, None, "hot_last", "table"),
    "hot_first_w37_h4_d16": (37, 4, 16, 1, None, "hot_first", "dense"),
    "hot_last_w3_h4_d4": (3, 4, 4, 1, None, "hot_last", "table"),
    "flat_w3_h4_d8": (3, 4, 8, 1, None, "flat", "table"),
    "bias_only_w3_h4_d32": (3, 4, 32, 1, None, "bias_only", "table"),
    # 21 x 28 padded map: 12 windows, the last one holds labels 4, 5, 7, 8; 2 images
    "shift_21x28_h4_d32": (24, 4, 32, 12, ("shift", 21, 28), "benign", "table"),
    "shift_hot_21x28_h4_d16": (24, 4, 16, 12, ("shift", 21, 28), "hot_last", "table"),
    # 35 x 42: 30 windows (the 1/16-scale map of a 480 x 640 image is 30 x 40 -> padded 35 x 42)
    "shift_35x42_h8_d8": (30, 8, 8, 30, ("shift", 35, 42), "benign", "dense"),
    "over_fill_21x28_h4_d32": (12, 4, 32, 12, ("shift", 21, 28), "over_fill", "table"),
    "over_fill_21x28_h4_d4": (12, 4, 4, 12, ("shift", 21, 28), "over_fill", "dense"),
    "high_ids_w6_h4_d16": (6, 4, 16, 3, "high", "benign", "table"),
    "high_ids_hot_w6_h4_d32": (6, 4, 32, 3, "high", "hot_first", "dense"),
}


def window_regions(spec):
    if spec is None:
        return None
    if spec == "high":
        # synthetic labels 9..15 (the ABI takes 0..15): window 0 two labels split mid-tile, window 1 all seven, window 2 a single label
        t = torch.arange(NT)
        return torch.stack([9 + (t >= 20).int() * 6, 9 + (t % 7).int(), torch.full((NT,), 12, dtype=torch.int32)]).to(torch.int32)
    _, Hp, Wp = spec
    return M.shift_regions(Hp, Wp, "cpu").clone()


def window_case(name, dtype, seed=0):
    nwin, H, hd, wpi, rspec, regime, bform = WINDOW_CASES[name]
    g = gen(1000 + seed + sum(map(ord, name)))
    scale = hd ** -0.5
    region = window_regions(rspec)
    q, k, v, go = (randn(g, nwin, NT, H, hd) for _ in range(4))
    rel = M.relative_position_index().to(torch.int32)
    table = st(randn(g, 169, H) * 0.5, torch.float32)
    dense = st(randn(g, H, NT, NT) * 0.5, torch.float32)
    if regime == "flat":
        k = k[:, :1].expand(-1, NT, -1, -1).clone()
        table, dense = table * 0, dense * 0
    elif regime == "bias_only":
        q = q * 0
    elif regime in ("hot_last", "hot_first"):
        # the big scores live in one key tile (keys 32..48 / 0..31); elsewhere they stay O(1)
        hot = slice(32, NT) if regime == "hot_last" else slice(0, 32)
        s = torch.einsum("wihd,wjhd->whij", st(q, dtype), st(k, dtype))[..., hot].abs().max() * scale
        k[:, hot] *= 45.0 / s
    elif regime == "over_fill":
        # every query looks along one direction; the keys of ONE label carry a large component along it, so that for queries of the
        # other labels the best key of another region beats their best own-region key by more than the fill of 100
        d = torch.ones(hd, dtype=torch.float64) / hd ** 0.5
        q = 0.1 * q + 4.0 * d
        big = (region == region.max(dim=1, keepdim=True).values).repeat(nwin // wpi, 1)       # (nwin, 49): the window's highest label
        k = 0.1 * k + torch.where(big[:, :, None, None], 40.0 * hd ** 0.5, 0.0) * d
    bias = dense if bform == "dense" else R.dense_bias(table, rel)
    c = dict(name=name, nwin=nwin, H=H, hd=hd, wpi=wpi, region=region, regime=regime, scale=scale, rel=rel,
             table=table if bform == "table" else None, bias=bias,
             q=st(q, dtype), k=st(k, dtype), v=st(v, dtype), go=st(go, dtype))
    return c


def check_window_regime(c):
    """The property the regime's name promises, asserted on the fp64 scores."""
    s = R.window_scores(c["q"], c["k"], c["bias"], None, 1, c["scale"])
    raw = (s - c["bias"][None]).abs().max()
    p = torch.softmax(R.window_scores(c["q"], c["k"], c["bias"], c["region"], c["wpi"], c["scale"]), -1)
    if c["regime"] in ("hot_last", "hot_first"):
        assert 30 <= float(raw) <= 60, float(raw)
        hot = slice(32, NT) if c["regime"] == "hot_last" else slice(0, 32)
        cold = slice(0, 32) if c["regime"] == "hot_last" else slice(32, NT)
        assert float((s - c["bias"][None])[..., cold].abs().max()) < 0.5 * float(raw)
        assert float((p.max(-1).values > 0.9).double().mean()) > 0.4     # rows near one-hot: 4 in 10 give one key more than 0.9
    elif c["regime"] == "flat":
        assert float((p - 1.0 / NT).abs().max()) < 1e-12
    elif c["regime"] == "bias_only":
        assert float(raw) == 0.0
    elif c["regime"] == "over_fill":
        reg = c["region"].repeat(c["nwin"] // c["wpi"], 1)
        same = (reg[:, :, None] == reg[:, None, :])[:, None]
        best_same = s.masked_fill(~same, float("-inf")).max(-1).values
        best_other = s.masked_fill(same, float("-inf")).max(-1).values
        over = best_other - best_same > 100
        assert int(over.sum()) >= 40, int(over.sum())
        # ... and there the finite fill decides: the weight sits on a key of ANOTHER region (with -inf it could not)
        other_w = (p * (~same)).sum(-1)
        assert float(other_w[over].min()) > 0.99


# ------------------------------------------------------------------------------------------------- class-token attention
# name: (nwin, heads, e, regime)
TOKEN_CASES = {
    "benign_w3_e12": (3, 16, 12, "benign"),
    "benign_w1_e16": (1, 16, 16, "benign"),
    "benign_w3000_e24": (3000, 4, 24, "benign"),
    "benign_w3_h6_e24": (3, 6, 24, "benign"),            # 18 problems: not a multiple of the 4 / 2 waves of a workgroup
    "hot_w3_e12": (3, 16, 12, "hot"),
    "hot_w3_e16": (3, 16, 16, "hot"),
    "hot_w1_e24": (1, 16, 24, "hot"),
    "flat_w3_e12": (3, 16, 12, "flat"),
    "flat_w3_e24": (3, 16, 24, "flat"),
    "q0_w3_e16": (3, 16, 16, "bias_only"),
}


def token_case(name, dtype, seed=0):
    nwin, H, e, regime = TOKEN_CASES[name]
    g = gen(2000 + seed + sum(map(ord, name)))
    scale = 0.5
    q, q2, go, go2 = (randn(g, nwin, NT, H, 4) for _ in range(4))
    k, v = randn(g, nwin, NT, H, e), randn(g, nwin, NT, H, e)
    if regime == "hot":
        for t in (q, q2):
            s = scale * torch.einsum("wnhr,wnhc->whrc", st(t, dtype), st(k, dtype)).abs().max()
            t *= 45.0 / s
    elif regime == "flat":
        k = k[..., :1].expand(-1, -1, -1, e).clone()          # every feature channel the same column: uniform 1 / e
    elif regime == "bias_only":
        q, q2 = q * 0, q2 * 0
    return dict(name=name, nwin=nwin, H=H, e=e, regime=regime, scale=scale,
                q=st(q, dtype), q2=st(q2, dtype), k=st(k, dtype), v=st(v, dtype), go=st(go, dtype), go2=st(go2, dtype))


def check_token_regime(c):
    s = c["scale"] * torch.einsum("wnhr,wnhc->whrc", c["q"], c["k"])
    if c["regime"] == "hot":
        assert 30 <= float(s.abs().max()) <= 60
    elif c["regime"] == "flat":
        assert float((torch.softmax(s, -1) - 1.0 / c["e"]).abs().max()) < 1e-12      # the padded channels e..31 weigh nothing
    elif c["regime"] == "bias_only":
        assert float(s.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------- MHA core
# name: (B, L, S, heads, packed, mask, dropout p, regime)       head_dim 32 (the only one gwd_mha_flash_* takes)
MHA_CASES = {
    "sep_1x1200_benign": (2, 1, 1200, 2, False, None, 0.0, "benign"),
    "sep_1200x1_benign": (1, 1200, 1, 2, False, None, 0.0, "benign"),
    "sep_31x33_benign": (2, 31, 33, 2, False, None, 0.0, "benign"),
    "sep_33x31_p01": (2, 33, 31, 2, False, None, 0.1, "benign"),
    "sep_32x64_first_tile": (2, 32, 64, 2, False, "first_tile", 0.0, "benign"),
    "sep_64x32_benign": (2, 64, 32, 2, False, None, 0.0, "benign"),
    "sep_63x65_but_last": (2, 63, 65, 2, False, "all_but_last", 0.0, "benign"),
    "sep_65x63_but_first": (2, 65, 63, 2, False, "all_but_first", 0.0, "hot_last"),
    "sep_100x300_first_two_hot": (2, 100, 300, 2, False, "first_two", 0.0, "hot_last"),
    "sep_100x300_middle_hot_first": (2, 100, 300, 2, False, "middle", 0.0, "hot_first"),
    "sep_300x100_per_batch_p05": (3, 300, 100, 2, False, "per_batch", 0.5, "benign"),
    "sep_100x300_ragged15x20": (2, 100, 300, 8, False, "ragged_15x20", 0.1, "benign"),
    "sep_100x1200_ragged30x40_hot": (2, 100, 1200, 2, False, "ragged_30x40", 0.0, "hot_last"),
    "sep_33x65_flat_first_tile": (2, 33, 65, 2, False, "first_tile", 0.0, "flat"),
    "sep_33x65_q0": (2, 33, 65, 2, False, "middle", 0.0, "bias_only"),
    "packed_1x1": (2, 1, 1, 2, True, None, 0.0, "benign"),
    "packed_33_hot": (2, 33, 33, 2, True, None, 0.0, "hot_last"),
    "packed_64_first_tile_hot": (2, 64, 64, 2, True, "first_tile", 0.0, "hot_last"),
    "packed_65_zero_row": (2, 65, 65, 2, True, "per_batch", 0.5, "benign"),
    "packed_300_ragged15x20_hot": (2, 300, 300, 8, True, "ragged_15x20", 0.0, "hot_first"),
    "packed_1200_ragged30x40": (2, 1200, 1200, 1, True, "ragged_30x40", 0.0, "benign"),
}


def ragged_mask(h, w):
    """The padding mask of a ragged image pair at a (h, w) token map, as NestedTensor + the backbone's nearest resize produce it
    (util/misc.py:273-313, backbone.py:79-88): a 32x canvas, image 0 fills it, image 1 is 13/15 of its height and 17/20 of its width."""
    Hc, Wc = 32 * h, 32 * w
    pad = torch.ones(2, Hc, Wc, dtype=torch.bool)
    pad[0, :, :] = False
    pad[1, :Hc * 13 // 15, :Wc * 17 // 20] = False
    return F.interpolate(pad[None].float(), size=(h, w)).to(torch.bool)[0].reshape(2, h * w)


def mha_mask(kind, B, S):
    if kind is None:
        return None
    m = torch.zeros(B, S, dtype=torch.bool)
    if kind == "first_tile":
        m[:, :32] = True
    elif kind == "first_two":
        m[:, :64] = True
    elif kind == "middle":
        m[:, 32:64] = True
    elif kind == "all_but_last":
        m[:, :S - 1] = True
    elif kind == "all_but_first":
        m[:, 1:] = True
    elif kind == "per_batch":
        m[0, :S // 2] = True                    # leading half
        m[1, S // 3:] = True                    # trailing two thirds
        if B > 2:
            m[2, 1::2] = True                   # every other key
    elif kind == "ragged_15x20":
        m = ragged_mask(15, 20)
    elif kind == "ragged_30x40":
        m = ragged_mask(30, 40)
    assert m.shape == (B, S) and not bool(m.all(-1).any())       # a row with every key masked is NaN in the reference: left out
    return m


def mha_case(name, dtype, seed=0):
    B, L, S, H, packed, mkind, p, regime = MHA_CASES[name]
    g = gen(3000 + seed + sum(map(ord, name)))
    E, scale = 32 * H, 32 ** -0.5
    q, go = randn(g, B, L, E), randn(g, B, L, E)
    k, v = randn(g, B, S, E), randn(g, B, S, E)
    kpm = mha_mask(mkind, B, S)
    live = torch.ones(B, S, dtype=torch.bool) if kpm is None else ~kpm
    if regime in ("hot_last", "hot_first"):
        # the large scores sit on the last (first) 32 un-masked keys of every image: walking the key tiles, the running maximum
        # rises at the last tile (is set by the first one and everything after is rescaled against it)
        hot = torch.zeros(B, S, dtype=torch.bool)
        for b in range(B):
            idx = torch.nonzero(live[b])[:, 0]
            hot[b, idx[-32:] if regime == "hot_last" else idx[:32]] = True
        s = scale * (R._heads(st(q, dtype), H) @ R._heads(st(k, dtype), H).transpose(-1, -2)).abs()
        s = s.masked_fill(~hot[:, None, None, :], 0.0).max()
        k = torch.where(hot[:, :, None], k * (45.0 / s), k * 0.2)
    elif regime == "flat":
        k = k[:, :1].expand(-1, S, -1).clone()
    elif regime == "bias_only":
        q = q * 0
    mult = None
    if p > 0:
        keep = torch.rand(B, H, L, S, generator=g) >= p
        mult = keep.double() / (1.0 - p)                 # 1 / (1 - p) = 1.11.. is rounded to the storage type like every operand
        if "zero_row" in name:
            mult[0, 1, L // 2] = 0.0                     # one query row with every probability dropped
            mult[1, 0, L - 1] = 0.0
        mult = st(mult, dtype)
    return dict(name=name, B=B, L=L, S=S, H=H, E=E, packed=packed, kpm=kpm, mult=mult, p=p, regime=regime, scale=scale,
                q=st(q, dtype), k=st(k, dtype), v=st(v, dtype), go=st(go, dtype))


def check_mha_regime(c):
    s = c["scale"] * R._heads(c["q"], c["H"]) @ R._heads(c["k"], c["H"]).transpose(-1, -2)
    if c["kpm"] is not None:
        s = s.masked_fill(c["kpm"][:, None, None, :], float("-inf"))
    fin = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s))
    p = torch.softmax(s, -1)
    if c["regime"] in ("hot_last", "hot_first"):
        assert 30 <= float(fin.max()) <= 60, float(fin.max())
        assert float((p.max(-1).values > 0.9).double().mean()) > 0.4
    elif c["regime"] == "flat":
        n = (~c["kpm"]).sum(-1).double() if c["kpm"] is not None else torch.full((c["B"],), float(c["S"]), dtype=torch.float64)
        assert float((p.max(-1).values - (1.0 / n)[:, None, None]).abs().max()) < 1e-12
    elif c["regime"] == "bias_only":
        assert float(fin.max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ row softmax
# (rows, L, amplitude): rows never a multiple of the rows a workgroup takes (they are odd and prime-ish); amplitude 80 for both
# types, 1e4 for fp32 only (bf16 holds 1e4 with a spacing of 64: nothing to learn from it)
SOFTMAX_LS = [1, 2, 7, 24, 40, 49, 63, 64, 65, 80, 100, 300, 1000, 1200]


def softmax_cases(dtype):
    out = []
    for i, L in enumerate(SOFTMAX_LS):
        rows = [13, 37, 101, 7][i % 4]
        amps = [1.0, 80.0] + ([1e4] if dtype == torch.float32 else [])
        for amp in amps:
            out.append((rows, L, amp))
    return out


def softmax_case(rows, L, amp, dtype, masked, seed=0):
    g = gen(4000 + seed + rows * 7 + L)
    x = randn(g, rows, L).clamp(-3, 3) / 3 * amp
    gy = randn(g, rows, L)
    scale, mask, rpm = 1.0, None, 1
    if masked:
        scale = 0.25 if amp < 100 else 1.0              # scale x stays within +-1e4
        rpm = rows                                       # one mask row for all rows, as one (image, all heads and queries) block
        mask = torch.zeros(1, L, dtype=torch.bool)
        if L > 1:
            mask[0, : L // 2] = True                     # the leading half padded: the maximum is found among the survivors only
    return dict(x=st(x, dtype), gy=st(gy, dtype), scale=scale, mask=mask, rpm=rpm)


# ------------------------------------------------------------------------------------------------------ reference points
# name: (B, nwin, R, heads, head_dim, regime)      ra amplitude ~45 in the hot cases (rows of the softmax over r near one-hot)
REF_CASES = {
    "r1_benign": (2, 1, 1, 4, 8, "benign"),
    "r7_benign": (2, 3, 7, 4, 16, "benign"),
    "r7_hot": (2, 3, 7, 4, 16, "hot"),
    "r40_benign": (2, 3, 40, 16, 32, "benign"),
    "r40_hot": (1, 2, 40, 16, 32, "hot"),
    "r128_benign": (1, 1, 128, 4, 32, "benign"),
    "r128_hot": (2, 1, 128, 8, 8, "hot"),
}


def ref_case(name, dtype, seed=0):
    B, nwin, Rn, H, hd, regime = REF_CASES[name]
    g = gen(5000 + seed + sum(map(ord, name)))
    scale = hd ** -0.5
    q = randn(g, B * nwin, NT, H, hd)
    ref_k, ref_v = randn(g, B, Rn, H * hd), randn(g, B, Rn, H * hd)
    if regime == "hot":
        s = scale * torch.einsum("bthd,brhd->btrh", st(q, dtype).reshape(B, -1, H, hd), st(ref_k, dtype).reshape(B, Rn, H, hd)).abs().max()
        ref_k = ref_k * (45.0 / s)
    T = nwin * NT
    ra2 = randn(g, B, T, Rn, H) * (15.0 if regime == "hot" else 1.0)           # the mix reads the diffused scores: its own operand
    return dict(name=name, B=B, nwin=nwin, R=Rn, H=H, hd=hd, scale=scale, regime=regime, q=st(q, dtype), ref_k=st(ref_k, dtype),
                ref_v=st(ref_v, dtype), g_ra=st(randn(g, B, T, Rn, H), dtype), ra2=st(ra2, dtype), g_q=st(randn(g, B, T, H * hd), dtype))


def check_ref_regime(c):
    if c["regime"] == "hot":
        ra = R.ref_scores_ref64(c["q"], c["ref_k"], c["B"], c["scale"], c["g_ra"])["ra"]
        assert 30 <= float(ra.abs().max()) <= 60 and 30 <= float(c["ra2"].abs().max()) <= 90


# ------------------------------------------------------------------------------------------------- sizing the constants
def measure_c(which=("window", "token", "mha", "softmax", "ref")):
    """Largest |model - ref64| / (u (|ref| + cond)) of the rounding models over the whole matrix:
    {(operation, type, output): (maximum, case)}.  tests/attn_ref.py's C is twice these, rounded up to one decimal."""
    res = {}

    def upd(op, dn, out, val, case):
        if val > res.get((op, dn, out), (-1.0, ""))[0]:
            res[(op, dn, out)] = (val, case)

    for dtype in (torch.bfloat16, torch.float32):
        dn, u, rounding = R.dtype_name(dtype), R.unit_roundoff(dtype), dtype == torch.bfloat16
        if "window" in which:
            for name in WINDOW_CASES:
                c = window_case(name, dtype)
                a = (c["q"], c["k"], c["v"], c["bias"], c["region"], c["wpi"], c["scale"], c["go"])
                ref, cond, mod = R.window_ref64(*a), R.window_cond(*a), R.window_model(*a, rounding=rounding)
                for o in ref:
                    upd("window", dn, o, float(R.ratio(mod[o], ref[o], cond[o], R.U_F32 if o == "dbias" else u).max()), name)
        if "token" in which:
            for name in TOKEN_CASES:
                c = token_case(name, dtype)
                a = (c["q"], c["k"], c["v"], c["scale"], c["go"])
                ref, cond, mod = R.token_ref64(*a), R.token_cond(*a), R.token_model(*a, rounding=rounding)
                for o in ref:
                    upd("token", dn, o, float(R.ratio(mod[o], ref[o], cond[o], u).max()), name)
                if rounding:
                    a = (c["q"], c["q2"], c["k"], c["v"], c["scale"], c["go"], c["go2"])
                    ref, cond, mod = R.token_pair_ref64(*a), R.token_pair_cond(*a), R.token_pair_model(*a)
                    for o in ref:
                        upd("token_pair", dn, o, float(R.ratio(mod[o], ref[o], cond[o], u).max()), name)
        if "mha" in which:
            for name in MHA_CASES:
                c = mha_case(name, dtype)
                a = (c["q"], c["k"], c["v"], c["H"], c["kpm"], c["mult"], c["scale"], c["go"])
                ref, cond, mod = R.mha_ref64(*a), R.mha_cond(*a), R.mha_model(*a, rounding=rounding)
                for o in ref:
                    upd("mha", dn, o, float(R.ratio(mod[o], ref[o], cond[o], R.U_F32 if o == "lse" else u).max()), name)
        if "ref" in which:
            for name in REF_CASES:
                c = ref_case(name, dtype)
                a = (c["q"], c["ref_k"], c["B"], c["scale"], c["g_ra"])
                ref, cond, mod = R.ref_scores_ref64(*a), R.ref_scores_cond(*a), R.ref_scores_model(*a, out_dtype=dtype)
                for o in ref:
                    upd("ref_scores", dn, o, float(R.ratio(mod[o], ref[o], cond[o], R.U_F32 if o == "dk" else u).max()), name)
                a = (c["ra2"], c["ref_v"], c["H"], c["g_q"])
                mod = R.ref_mix_model(*a, out_dtype=dtype)
                ref = R.ref_mix_ref64(*a)
                ref.update(R.ref_mix_backward_ref64(mod["att"].double(), c["ref_v"], c["H"], c["g_q"]))
                cond = R.ref_mix_cond(*a, att_stored=mod["att"].double())
                for o in mod:
                    upd("ref_mix", dn, o, float(R.ratio(mod[o], ref[o], cond[o], R.U_F32 if o == "dv" else u).max()), name)
        if "softmax" in which:
            for rows, L, amp in softmax_cases(dtype):
                for masked in (False, True):
                    c = softmax_case(rows, L, amp, dtype, masked)
                    args = (c["x"], c["gy"], c["scale"], c["mask"], c["rpm"])
                    ref, cond, mod = R.softmax_ref64(*args), R.softmax_cond(*args), R.softmax_model(*args, out_dtype=dtype)
                    case = "rows %d L %d amplitude %g%s" % (rows, L, amp, " masked" if masked else "")
                    upd("softmax", dn, "y", float(R.ratio(mod["y"], ref["y"], cond["y"], u).max()), case)
                    ys = mod["y"].double()                           # the backward reads the stored y
                    gref = R.softmax_backward_ref64(ys, c["gy"], c["scale"])
                    gcond = R.softmax_cond(*args, y_stored=ys)["gx"]
                    upd("softmax", dn, "gx", float(R.ratio(mod["gx"], gref, gcond, u).max()), case)
    return res

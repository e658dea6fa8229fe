"""GPU: the two post-processing kernels of csrc/postproc.hip against plain torch on the same inputs.

gwd_dense_postprocess: depth_out / depth_mm / label equal BIT FOR BIT to where(isnan, min, clamp), round(d * 1000).clamp(max =
65535) and argmax; padding 0 / 0 / 255; guard bytes before and behind every output untouched.
gwd_line_postprocess: scores within 2e-5 of softmax(...)[..., 0] (the fp32 kernel bar of tests/test_hip_kernels.py), lines_px
equal to the fp32 product bit for bit, order == argsort(descending, stable) and count == the reference count on inputs whose
reference scores are further apart than the bar can move them."""
import pytest
import torch

from gw_depth_amd import hip, ops

MIN_D, MAX_D = 1e-3, 10.0
GUARD = 256             # bytes, a multiple of 16: the guarded outputs keep the alignment of the allocation
FILL = 0xA5


@pytest.fixture()
def dev():
    hip.set_library(None)
    return torch.device("cuda")


def canned(n, H, W, seed=21):
    """The canned map of oracle/make_golden_eval.py::canned_inputs (out-of-range, +-inf, nan, a row of tied logits), re-stated,
    plus NaN logits in either class and in both."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(n, 1, H, W, generator=g) * 11.0 - 0.5            # (-0.5, 10.5): both clamps fire
    pred[:, :, 3, 5] = float("inf")
    pred[:, :, 4, 6] = float("-inf")
    pred[:, :, 7, 9] = float("nan")
    pred[:, :, 8, 1] = 70.0                                             # beyond the uint16 millimetre range before the clamp
    logits = torch.randn(n, 2, H, W, generator=g)
    logits[:, :, 10, :] = 0.0                                           # ties: argmax picks class 0
    logits[:, 0, 12, 3] = float("nan")
    logits[:, 1, 12, 4] = float("nan")
    logits[:, :, 12, 5] = float("nan")
    logits[:, 0, 13, 2] = float("inf")
    logits[:, :, 13, 3] = float("inf")
    return pred, logits


def dense_reference(depth, logits, sizes, max_d=MAX_D):
    d = depth.float().reshape(depth.shape[0], *depth.shape[-2:])
    B, H, W = d.shape
    out = torch.where(torch.isnan(d), torch.full_like(d, MIN_D), d.clamp(MIN_D, max_d))
    mm = torch.round(out * 1000.0).clamp(max=65535.0)
    lab = logits.float().argmax(1)
    if sizes is not None:
        ys, xs = torch.arange(H, device=d.device)[None, :, None], torch.arange(W, device=d.device)[None, None, :]
        inside = (ys < sizes[:, 0, None, None]) & (xs < sizes[:, 1, None, None])
        out = torch.where(inside, out, torch.zeros_like(out))
        mm = torch.where(inside, mm, torch.zeros_like(mm))
        lab = torch.where(inside, lab, torch.full_like(lab, 255))
    return out, mm.to(torch.int32), lab.to(torch.int32)


def guarded(shape, dtype, device):
    n = 1
    for s in shape:
        n *= s
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
    return raw, raw[GUARD:GUARD + nbytes].view(dtype).view(shape)


def guards_intact(raw):
    return bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw", "pixel_major"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 60, 80), (3, 61, 83), (2, 960, 1280)])
def test_dense_postprocess_bit_exact(dev, shape, dtype, layout):
    B, H, W = shape
    pred, logits = canned(B, H, W)
    pred, logits = pred.to(dev).to(dtype), logits.to(dev).to(dtype)
    if layout == "pixel_major":
        logits = logits.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # the model's view: (B,2,H,W) over (B,H,W,2)
        assert not logits.is_contiguous()
    ragged = torch.tensor([[H, W], [H - 7, W - 13], [H // 2 + 1, 5]][:B], dtype=torch.int32, device=dev)
    for sizes in (None, ragged):
        bufs = [guarded((B, H, W), dt, dev) for dt in (torch.float32, torch.uint16, torch.uint8)]
        out = ops.dense_postprocess(pred, logits, sizes, MIN_D, MAX_D, out=tuple(b[1] for b in bufs))
        torch.cuda.synchronize()
        ref_d, ref_mm, ref_lab = dense_reference(pred, logits, sizes)
        assert out[0].dtype == torch.float32 and out[1].dtype == torch.uint16 and out[2].dtype == torch.uint8
        assert torch.equal(out[0].view(torch.int32), ref_d.view(torch.int32))        # bit for bit (no NaN left to compare unequal)
        assert torch.equal(out[1].to(torch.int32), ref_mm)
        assert torch.equal(out[2].to(torch.int32), ref_lab)
        assert all(guards_intact(raw) for raw, _ in bufs)
        if sizes is not None:
            pad = ref_lab == 255
            assert bool(pad.any()) and bool((out[0][pad] == 0).all()) and bool((out[1].to(torch.int32)[pad] == 0).all())
        # the special values went where the rule says
        assert float(out[0][0, 3, 5]) == MAX_D and float(out[0][0, 4, 6]) == pytest.approx(MIN_D) and float(out[0][0, 7, 9]) == pytest.approx(MIN_D)
        assert out[2][0, 10].to(torch.int32).sum() == 0
        assert [int(v) for v in out[2][0, 12, 3:6]] == [0, 1, 0]


@pytest.mark.gpu
def test_dense_postprocess_millimetres_saturate_and_mm_is_optional(dev):
    B, H, W = 1, 16, 24
    pred, logits = canned(B, H, W)
    pred, logits = pred.to(dev), logits.to(dev)
    d, mm, lab = ops.dense_postprocess(pred, logits, None, MIN_D, 100.0)
    ref_d, ref_mm, ref_lab = dense_reference(pred, logits, None, max_d=100.0)
    mm32 = mm.to(torch.int32)
    assert int(mm32[0, 8, 1]) == 65535 and int(mm32[0, 3, 5]) == 65535
    assert torch.equal(d, ref_d) and torch.equal(mm32, ref_mm) and torch.equal(lab.to(torch.int32), ref_lab)
    d2, none, lab2 = ops.dense_postprocess(pred, logits, None, MIN_D, 100.0, with_mm=False)
    assert none is None and torch.equal(d2, d) and torch.equal(lab2, lab)


def line_inputs(B, Q, ld, seed):
    """Scores whose order the reference decides: per image the logit difference is a seeded shuffle of linspace(-2.5, 2.5, Q),
    so neighbouring reference scores are >= 3.5e-4 apart and >= 5.3e-4 from the threshold 0.6 for every Q used here."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.empty(B, Q, 2)
    for b in range(B):
        d = torch.linspace(-2.5, 2.5, Q)[torch.randperm(Q, generator=g)]
        a = 3.0 * torch.randn(Q, generator=g)
        logits[b] = torch.stack([a + d / 2, a - d / 2], -1)
    lines = torch.rand(B, Q, ld, generator=g)
    return logits, lines


@pytest.mark.gpu
@pytest.mark.parametrize("ld", [4, 6])
@pytest.mark.parametrize("Q", [1, 63, 64, 100, 1000])
def test_line_postprocess(dev, Q, ld):
    B, thresh, gap = 3, 0.6, 1e-4
    logits, lines = line_inputs(B, Q, ld, seed=100 + Q)
    ref = torch.softmax(logits.to(dev), -1)[..., 0]
    srt = ref.sort(-1).values
    if Q > 1:
        assert float((srt[:, 1:] - srt[:, :-1]).min()) >= gap, "the inputs do not decide the order"
    assert float((ref - thresh).abs().min()) >= gap, "the inputs do not decide the count"
    if Q >= 63:                                                        # exact duplicates: equal logit pairs, equal scores on both sides
        for b in range(B):
            for src, dst in ((5, 40), (40 + b, 7), (Q - 1, 0)):
                logits[b, dst] = logits[b, src]
    logits, lines = logits.to(dev), lines.to(dev)
    sizes = torch.tensor([[480, 640], [960, 1280], [427, 569]], dtype=torch.int32, device=dev)
    scores, lines_px, order, count = ops.line_postprocess(logits, lines, sizes, thresh)
    torch.cuda.synchronize()
    ref = torch.softmax(logits, -1)[..., 0]
    assert scores.shape == (B, Q) and float((scores - ref).abs().max()) <= 2e-5
    h, w = sizes[:, 0].float(), sizes[:, 1].float()
    want = lines[..., :4] * torch.stack([w, h, w, h], 1)[:, None, :]
    assert lines_px.shape == (B, Q, 4) and torch.equal(lines_px, want)
    assert order.dtype == torch.int32 and torch.equal(order.long(), torch.argsort(ref, dim=-1, descending=True, stable=True))
    assert count.dtype == torch.int32 and torch.equal(count.long(), (ref > thresh).sum(-1))


@pytest.mark.gpu
def test_line_postprocess_refuses_more_than_1024_queries(dev):
    logits, lines = line_inputs(1, 1025, 4, seed=1)
    sizes = torch.tensor([[480, 640]], dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="status -2"):
        ops.line_postprocess(logits.to(dev), lines.to(dev), sizes)
    ok = ops.line_postprocess(logits[:, :1024].to(dev), lines[:, :1024].to(dev), sizes)
    assert torch.equal(ok[2].long().sort(-1).values, torch.arange(1024, device=dev)[None])


def test_postprocess_entry_points_refuse_cpu_tensors():
    hip.set_library(None)
    lib = hip.library()
    z = torch.zeros
    with pytest.raises(hip.HipUnavailable):
        lib.dense_postprocess(z(1, 8, 8), z(1, 2, 8, 8), (128, 1, 64), None, z(1, 8, 8), None, z(1, 8, 8, dtype=torch.uint8), 1, 8, 8, 1e-3, 10.0)
    with pytest.raises(hip.HipUnavailable):
        lib.line_postprocess(z(1, 4, 2), z(1, 4, 4), z(1, 2, dtype=torch.int32), z(1, 4), z(1, 4, 4), z(1, 4, dtype=torch.int32),
                             z(1, dtype=torch.int32), 1, 4, 4, 0.6)

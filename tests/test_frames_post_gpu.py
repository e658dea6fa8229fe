"""GPU: gwd_dense_postprocess_resized alone against its fp64 restatement (tests/frames_ref.py) on the shapes of frames_ref.SHAPES:
fp32 and bf16 sources, interleaved and planar logits, with and without a twin, with and without millimetres.  The padding of
the sources is NaN / 1e30, so a kernel that reads padding fails; the outputs sit between guard bytes.

BOUND.  depth_out within K * 2^-24 * max_depth of the restatement, K = 10, counted from the kernel's fp32 arithmetic on values in
[0, max_depth] (bf16 -> fp32 is exact; u = 2^-24 * max_depth):
  twin: the add rounds once, the halving is exact                                                     1 u on every sample
  one blend (1 - l) a + l b: the division behind l moves the result by at most l |b - a| 2^-24         1 u
                             1 - l and its product with a: two roundings of at most (1 - l) a 2^-24,
                             the product l b: one of l b 2^-24 - together at most 2 max(a, b) 2^-24    2 u
                             the sum                                                                   1 u
  rows are blended first (4 u), the column blend passes that on (a convex combination: 4 u) and adds its own 4 u
  1 + 4 + 4 = 9 u to first order; one more u covers the second-order terms and the fp64 restatement's own rounding.   K = 10
(fused multiply-adds only drop roundings from this count.)
depth_mm is bit-equal to round(depth_out * 1000).clamp(max=65535) of the kernel's OWN depth_out (the rule of
tests/test_postproc_kernels.py).  label equals the restatement's wherever the margin |l0 - l1| of the interpolated logits
exceeds 2 K 2^-24 max |logit| (doubled under a twin: the sums are twice as large); at most 1 % of the pixels may be excused that
way, which is asserted here and, for the same seeds, in tests/test_frames_post.py."""
import functools

import pytest
import torch

from gw_depth_amd import hip, ops
from tests import frames_ref as R

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5
DEPTH_BOUND = R.K * R.U * R.MAX_D


@pytest.fixture()
def dev():
    hip.set_library(None)
    return torch.device("cuda")


def guarded(shape, dtype, device):
    n = 1
    for s in shape:
        n *= s
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
    return raw, raw[GUARD:GUARD + nbytes].view(dtype).view(shape)


def guards_intact(raw):
    return bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all())


def planted(depth, seg):
    """Non-finite depth samples and NaN logits at known pixels inside every image's un-padded region (rows < 9, columns < 13)."""
    depth, seg = depth.clone(), seg.clone()
    depth[:, 1, 2], depth[:, 1, 9], depth[:, 2, 5] = float("nan"), float("inf"), float("-inf")
    depth[0, 0, 0], depth[-1, 1, 12] = float("inf"), float("nan")
    seg[:, 0, 1, 6], seg[:, 1, 2, 1], seg[:, :, 2, 10] = float("nan"), float("nan"), float("nan")
    return depth, seg


@functools.lru_cache(maxsize=None)
def case(seed, shape, twin, plant=False):
    """The inputs and their restatement, computed once per (seed, shape, twin) and shared by every dtype and layout."""
    depth, seg, sizes, frames, out_hw = R.inputs(seed, shape, twin)
    tol = R.label_tolerance(seg, sizes, twin)
    if plant:
        depth, seg = planted(depth, seg)
    ref = R.dense_resized(depth, seg, sizes, frames, out_hw, R.MIN_D, R.MAX_D, twin=len(sizes) if twin else 0)
    return depth, seg, sizes, frames, out_hw, tol, ref


def on_device(depth, seg, dtype, layout, dev):
    depth, seg = depth.to(dev).to(dtype), seg.to(dev).to(dtype)
    if layout == "pixel_major":                                        # the model's view: (B,2,H,W) over (B,H,W,2)
        seg = seg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return depth, seg


def run_and_check(dev, seed, shape, twin, dtype, layout, with_mm=True, plant=False):
    depth, seg, sizes, frames, out_hw, tol, (ref_d, _, ref_lab, margin) = case(seed, shape, twin, plant)
    B = len(sizes)
    dd, ds = dtype if isinstance(dtype, tuple) else (dtype, dtype)
    d, s = on_device(depth, seg, dd, layout, dev)[0], on_device(depth, seg, ds, layout, dev)[1]
    sz = torch.tensor(sizes, dtype=torch.int32, device=dev)
    fz = torch.tensor(frames, dtype=torch.int32, device=dev)
    bufs = [guarded((B, *out_hw), dt, dev) for dt in (torch.float32, torch.uint16, torch.uint8)]
    out = ops.dense_postprocess_resized(d, s, sz, fz, out_hw, R.MIN_D, R.MAX_D, twin=B if twin else 0,
                                        out=(bufs[0][1], bufs[1][1] if with_mm else None, bufs[2][1]))
    torch.cuda.synchronize()
    assert all(guards_intact(raw) for raw, _ in bufs)
    got_d, got_lab = out[0].cpu(), out[2].cpu().to(torch.int64)
    inside = ref_lab != 255
    assert int(inside.sum()) == sum(fh * fw for fh, fw in frames)
    err = float((got_d.double() - ref_d).abs().max())
    print("%s seed %d twin %d %s %s: depth error %.3e (bound %.3e)" % (shape, seed, twin, dtype, layout, err, DEPTH_BOUND))
    assert bool(torch.isfinite(got_d).all()) and err <= DEPTH_BOUND
    assert float(got_d[inside].min()) >= R.MIN_D and float(got_d[inside].max()) <= R.MAX_D
    if with_mm:
        assert torch.equal(out[1].cpu().to(torch.int64), torch.round(got_d * 1000.0).clamp(max=65535.0).to(torch.int64))
    else:
        assert out[1] is None and bool((bufs[1][0] == FILL).all())
    # outside every frame: 0 / 0 / 255 exactly
    assert bool((got_d[~inside] == 0).all()) and bool((got_lab[~inside] == 255).all())
    decided = inside & (margin > tol)
    excused = int((inside & ~decided).sum())
    print("    labels: %d of %d pixels excused (margin <= %.2e)" % (excused, int(inside.sum()), tol))
    assert excused <= 0.01 * int(inside.sum())
    assert torch.equal(got_lab[decided], ref_lab[decided]) and int(got_lab[inside].max()) <= 1
    return out, margin, inside


@pytest.mark.parametrize("layout", ["nchw", "pixel_major"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("twin", [False, True], ids=["single", "twin"])
@pytest.mark.parametrize("shape", sorted(R.SHAPES))
def test_resized_postprocess(dev, shape, twin, dtype, layout):
    for seed in R.SEEDS:
        run_and_check(dev, seed, shape, twin, dtype, layout)


@pytest.mark.parametrize("dtype", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)], ids=["fp32-bf16", "bf16-fp32"])
@pytest.mark.parametrize("shape", ["src16_vec", "up_px"])
def test_mixed_source_dtypes_and_no_millimetres(dev, shape, dtype):
    run_and_check(dev, R.SEEDS[0], shape, True, dtype, "pixel_major", with_mm=False)
    run_and_check(dev, R.SEEDS[0], shape, False, dtype, "nchw", with_mm=False)


@pytest.mark.parametrize("layout", ["nchw", "pixel_major"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("twin", [False, True], ids=["single", "twin"])
@pytest.mark.parametrize("shape", ["up_vec", "src16_vec", "down_px"])
def test_non_finite_samples_follow_san_and_nan_logits_the_argmax_rule(dev, shape, twin, dtype, layout):
    """NaN, +inf and -inf depth samples inside the region are sanitised BEFORE they are blended (the result stays finite and within
    the bound of the restatement, which does the same); a NaN logit makes the blended logit NaN wherever its weight is not zero, and
    the label there follows the rule (a NaN is the maximum, the first one wins) - those pixels have margin inf in the restatement and
    are compared like every other."""
    _, margin, inside = run_and_check(dev, R.SEEDS[1], shape, twin, dtype, layout, plant=True)
    assert int((torch.isinf(margin) & inside).sum()) >= 3


@pytest.mark.parametrize("layout", ["nchw", "pixel_major"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["up_px", "src16_vec"])
def test_identity_is_the_plain_postprocessing_bit_for_bit(dev, shape, dtype, layout):
    depth, seg, sizes, _, _ = R.inputs(9, shape, False)
    depth, seg = planted(depth, seg)
    seg[:, 0, 3, 3], seg[:, :, 3, 4], seg[:, :, 4, 2] = float("inf"), float("inf"), 0.25       # an inf, a tie of infs, a plain tie
    B, H, W = depth.shape
    d, s = on_device(depth, seg, dtype, layout, dev)
    sz = torch.tensor(sizes, dtype=torch.int32, device=dev)
    for sizes_dev in (sz, None):
        want = ops.dense_postprocess(d, s, sizes_dev, R.MIN_D, R.MAX_D)
        got = ops.dense_postprocess_resized(d, s, sizes_dev, sz if sizes_dev is not None else torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev),
                                            (H, W), R.MIN_D, R.MAX_D)
        torch.cuda.synchronize()
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        assert torch.equal(got[1].to(torch.int32), want[1].to(torch.int32)) and torch.equal(got[2], want[2])
    assert int((want[2] == 255).sum()) == 0 and int((ops.dense_postprocess(d, s, sz, R.MIN_D, R.MAX_D)[2] == 255).sum()) > 0


def test_sizes_above_16384_are_refused(dev):
    d = torch.zeros(1, 2, 8, device=dev)
    s = torch.zeros(1, 2, 2, 8, device=dev)
    fz = torch.tensor([[2, 8]], dtype=torch.int32, device=dev)
    for out_hw in ((16385, 8), (2, 16392)):
        with pytest.raises(RuntimeError, match="status -1"):
            ops.dense_postprocess_resized(d, s, None, fz, out_hw, R.MIN_D, R.MAX_D)
    wide = torch.zeros(1, 1, 16392, device=dev)
    with pytest.raises(RuntimeError, match="status -1"):
        ops.dense_postprocess_resized(wide, torch.zeros(1, 2, 1, 16392, device=dev), None, fz, (2, 8), R.MIN_D, R.MAX_D)
    out = ops.dense_postprocess_resized(d, s, None, fz, (2, 8), R.MIN_D, R.MAX_D)
    torch.cuda.synchronize()
    assert float(out[0].min()) == pytest.approx(R.MIN_D) and int(out[2].max()) == 0


def test_resized_entry_point_refuses_cpu_tensors():
    hip.set_library(None)
    z = torch.zeros
    with pytest.raises(hip.HipUnavailable):
        hip.library().dense_postprocess_resized(z(1, 8, 8), z(1, 2, 8, 8), (128, 1, 64), None, z(1, 2, dtype=torch.int32), 0, z(1, 8, 8), None,
                                                z(1, 8, 8, dtype=torch.uint8), 1, 8, 8, 8, 8, 1e-3, 10.0)

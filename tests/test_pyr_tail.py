"""CPU: the identity behind the low-resolution pyramid tail in fp64 (forward and backward), the route selection on the CPU stand-in,
and the new entry points in header, binding and library."""
import ctypes
import os

import pytest
import torch

from gw_depth_amd import hip, ops
from gw_depth_amd.model import PyramidLayer
from tests import pyr_tail_ref as R
from tests.fake_device import FakeDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLS = (16, 8, 4, 2)
SIZES = [(16, 16), (24, 32), (30, 40), (17, 19)]


def _case(H, W, C2=4, N=6, B=2, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    x = torch.randn(B, H, W, C2, generator=g, dtype=torch.float64)
    ys = [torch.randn(B, H // k, W // k, C2, generator=g, dtype=torch.float64) for k in POOLS]
    w = torch.randn(N, 3, 3, 5 * C2, generator=g, dtype=torch.float64) * 0.3
    return x, ys, w


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("nlow", [1, 3, 4])
def test_identity_forward_and_backward_fp64(H, W, nlow):
    x, ys, w = _case(H, W)
    leaves = [t.clone().requires_grad_(True) for t in [x] + ys + [w]]
    ref = R.tail_direct(leaves[0], leaves[1:5], leaves[5])
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    gref = torch.autograd.grad(ref, leaves, gout)
    leaves2 = [t.clone().requires_grad_(True) for t in [x] + ys + [w]]
    got = R.tail_decomposed(leaves2[0], leaves2[1:5], leaves2[5], nlow)
    ggot = torch.autograd.grad(got, leaves2, gout)
    scale = float(ref.detach().abs().max())
    assert float((got - ref).detach().abs().max()) <= 1e-12 * scale
    for a, b in zip(ggot, gref):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_references_are_that_decomposition(H, W):
    """tail_z / tail_G (what the GPU test holds the kernels to) against the direct formulation and autograd."""
    x, ys, w = _case(H, W, seed=3)
    B, _, _, C2 = x.shape
    N, nlow = w.shape[0], 3
    w_hi = torch.cat([w[..., :C2], w[..., (1 + nlow) * C2:]], dim=-1)
    part = R.conv3x3(torch.cat([x, R.up_ac(ys[3], H, W)], dim=-1), w_hi)
    Zs = []
    for k in range(nlow):
        wl = w[..., (k + 1) * C2:(k + 2) * C2].permute(1, 2, 0, 3).reshape(9 * N, C2)
        Zs.append((ys[k] @ wl.t()).reshape(B, ys[k].shape[1], ys[k].shape[2], 9, N).requires_grad_(True))
    z, S = R.tail_z(part, [Z.detach() for Z in Zs])
    ref = R.tail_direct(x, ys, w)
    assert float((z - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((S >= z.abs() - 1e-12).all())
    # the gradient of every product map: tail_G against autograd through the same sum
    zz = part.clone()
    for Z in Zs:
        up = torch.einsum("Yh,Xw,bhwtn->bYXtn", R.resize_matrix(Z.shape[1], H), R.resize_matrix(Z.shape[2], W), Z)
        for t in range(9):
            ty, tx = t // 3 - 1, t % 3 - 1
            pad = torch.nn.functional.pad(up[:, :, :, t], (0, 0, 1, 1, 1, 1))
            zz = zz + pad[:, 1 + ty:1 + ty + H, 1 + tx:1 + tx + W]
    gz = torch.randn(z.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    grads = torch.autograd.grad(zz, Zs, gz)
    for Z, g in zip(Zs, grads):
        G, Sg, n = R.tail_G(gz, Z.shape[1], Z.shape[2])
        assert float((G - g).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max()))
        assert bool((Sg >= G.abs() - 1e-12).all()) and float(n.max()) <= H * W and float(n.min()) >= 1


def test_pool16_map_of_16x16_is_one_pixel():
    U = R.resize_matrix(1, 16)
    assert U.shape == (16, 1) and bool((U == 1.0).all())


def test_cpu_stand_in_keeps_the_old_route_bit_for_bit():
    hip.set_library(FakeDevice())
    try:
        torch.manual_seed(0)
        layer = PyramidLayer(8)
        x = torch.randn(1, 16, 24, 8)
        outs = []
        for flag in (True, False):
            old = ops.PYRAMID_TAIL_LOWRES
            ops.PYRAMID_TAIL_LOWRES = flag
            try:
                called = []
                orig = ops.pyramid_tail
                ops.pyramid_tail = lambda *a, **k: called.append(1) or orig(*a, **k)
                try:
                    outs.append(layer(x).detach().clone())
                finally:
                    ops.pyramid_tail = orig
                assert not called
            finally:
                ops.PYRAMID_TAIL_LOWRES = old
        assert torch.equal(outs[0], outs[1])
    finally:
        hip.set_library(None)


def test_header_binding_and_library_agree_on_the_new_symbols():
    names = ("gwd_pyr_tail_forward", "gwd_pyr_tail_backward", "gwd_pyr_tail_fold_wgrad")
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for n in names:
        assert ("int %s(" % n) in header and n in hip.ENTRY_POINTS and hasattr(lib, n), n
    assert lib.gwd_version() == 10

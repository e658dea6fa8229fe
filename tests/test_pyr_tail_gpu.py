"""GPU: the low-resolution pyramid tail (csrc/pyrtail.hip, ops._PyramidTailFn).  Run with -x.

Kernels alone: every element of z and of every G_k against the fp64 reference of tests/pyr_tail_ref.py, bound (n - 1) 2^-24 S with S
the fp64 sum of the |terms| of the element and n their number (+ 2^-8 |ref| for a bf16 output); y / mean / rstd against an fp64
LayerNorm of the kernel's own z with the bounds of tests/row_ref.py.  The module: both routes of PyramidLayer(80) in one process
against the fp64 oracle.  Capture: the new route inside TrainStep(graph=True)."""
import zlib

import pytest
import torch

from gw_depth_amd import hip, ops
from tests import pyr_tail_ref as R
from tests import row_ref
from tests import row_witness as RW

pytestmark = pytest.mark.gpu

POOLS = (16, 8, 4, 2)
SIZES = [(16, 16), (24, 32), (30, 40), (17, 19)]
B = 2
U24, U8 = 2.0 ** -24, 2.0 ** -8


@pytest.fixture(autouse=True)
def real_library():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    assert not getattr(hip.library(), "is_fake", False)
    yield


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _assert_bound(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print("%s: max abs error %.3e, worst error / bound %.3f" % (name, float(err.max()), worst))
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements beyond the bound, first at %r" % (name, int(bad.sum()), tuple(bad.nonzero()[0].tolist()))


def _forward_case(H, W, N, nb, dt, gelu=True):
    g = _gen("f", H, W, N, nb, str(dt))
    part = torch.randn(B, H, W, N, generator=g).to(dt)
    Zs = [torch.randn(B, H // k, W // k, 9, N, generator=g).to(dt) for k in POOLS[:nb]]
    gamma, beta = 1.0 + 0.5 * torch.randn(N, generator=g), 0.5 * torch.randn(N, generator=g)
    lib = hip.library()
    dev = lambda t: t.cuda()
    outs = []
    for keep_z in (True, False):
        z = torch.empty(B, H, W, N, dtype=dt, device="cuda") if keep_z else None
        y = torch.empty(B, H, W, N, dtype=dt, device="cuda")
        mean, rstd = torch.empty(B * H * W, device="cuda"), torch.empty(B * H * W, device="cuda")
        assert lib.pyr_tail_forward(dev(part), [dev(Z) for Z in Zs], dev(gamma), dev(beta), z, y, mean, rstd, gelu) is True
        torch.cuda.synchronize()
        outs.append((z, y, mean, rstd))
    (z, y, mean, rstd), (_, y2, mean2, rstd2) = outs
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)       # z is optional and changes nothing
    ref, S = R.tail_z(part, Zs)
    bound = 36 * nb * U24 * S + (U8 * ref.abs() if dt == torch.bfloat16 else 0.0)
    _assert_bound("z %dx%d N %d nb %d %s" % (H, W, N, nb, dt), z, ref, bound)
    c = RW.parse_call("LF %d %d %d 0 1 0 %d" % (RW.BF16 if dt == torch.bfloat16 else RW.F32, B * H * W, N, int(gelu)))
    got = dict(y=y.cpu().view(-1, N), mean=mean.cpu(), rstd=rstd.cpu())
    row_ref.check(c, got, dict(x=z.cpu().view(-1, N), gamma=gamma, beta=beta), what="pyr_tail LayerNorm")


def _backward_case(H, W, N, nb, dt, ring=False):
    g = _gen("b", H, W, N, nb, str(dt), ring)
    gz = torch.randn(B, H, W, N, generator=g).to(dt)
    if ring:                                   # only the outermost pixel ring: every tap that leaves the map is a zero-padding term
        gz[:, 1:-1, 1:-1] = 0
    Gs = [torch.full((B, H // k, W // k, 9, N), float("nan"), dtype=dt, device="cuda") for k in POOLS[:nb]]
    hip.library().pyr_tail_backward(gz.cuda(), Gs)
    torch.cuda.synchronize()
    for G in Gs:
        h, w = G.shape[1], G.shape[2]
        ref, S, n = R.tail_G(gz, h, w)
        bound = (n - 1).clamp_min(0)[None, :, :, :, None] * U24 * S + (U8 * ref.abs() if dt == torch.bfloat16 else 0.0)
        _assert_bound("G %dx%d of %dx%d N %d %s%s" % (h, w, H, W, N, dt, " ring" if ring else ""), G, ref, bound)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("H,W", SIZES)
def test_forward_kernel(H, W, N, dt):
    for nb in (1, 2, 3):                        # 16x16 and 17x19: the pool-16 map is one pixel high (h_k == 1)
        _forward_case(H, W, N, nb, dt, gelu=(nb != 2))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("H,W", SIZES)
def test_backward_kernel(H, W, N, dt):
    for nb in (1, 2, 3):
        _backward_case(H, W, N, nb, dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_backward_kernel_outer_ring_only(dt):
    _backward_case(30, 40, 64, 3, dt, ring=True)
    _backward_case(17, 19, 64, 3, dt, ring=True)


def test_fold_puts_every_slice_where_the_parameter_keeps_it():
    N, C2, nbr, nlow = 32, 8, 4, 3
    g = _gen("fold")
    d_hi = torch.randn(N, 3, 3, (1 + nbr - nlow) * C2, generator=g)
    d_lo = [torch.randn(9 * N, 1, 1, C2, generator=g) for _ in range(nlow)]
    dw0 = torch.randn(N, 3, 3, (1 + nbr) * C2, generator=g)
    want = dw0.clone()
    want[..., :C2] += d_hi[..., :C2]
    want[..., (1 + nlow) * C2:] += d_hi[..., C2:]
    for k, d in enumerate(d_lo):
        want[..., (k + 1) * C2:(k + 2) * C2] += d.view(3, 3, N, C2).permute(2, 0, 1, 3)
    dw = dw0.cuda()
    hip.library().pyr_tail_fold_wgrad(d_hi.cuda(), [d.cuda() for d in d_lo], dw, C2)
    assert torch.equal(dw.cpu(), want)


# ------------------------------------------------------------------------------------------------ the module, both routes
def _oracle(layer, x):
    """fp64 evaluation of the same module on the CPU: output and the gradients of the input and of every parameter that is used."""
    from oracle import gwdepth_ref as O
    sd = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in layer.state_dict().items()}
    xin = x.detach().double().cpu().permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = O.pyramid(xin, O.View(sd)).permute(0, 2, 3, 1)
    gout = torch.randn(out.shape, generator=_gen("gout", tuple(out.shape)), dtype=torch.float64)
    names = [k for k in sd if ".layer4." not in k and not k.startswith("layer4.")]
    grads = torch.autograd.grad(out, [xin] + [sd[k] for k in names], gout)
    ref = {"out": out.detach(), "d input": grads[0].permute(0, 2, 3, 1)}
    for k, gr in zip(names, grads[1:]):
        ref["d " + k] = gr.permute(0, 2, 3, 1) if gr.dim() == 4 else gr
    return ref, gout


def _route_error(layer, x, ref, gout, lowres):
    """Largest error of the route over the output and every gradient, each relative to the largest magnitude of its reference."""
    old = ops.PYRAMID_TAIL_LOWRES
    ops.PYRAMID_TAIL_LOWRES = lowres
    calls = []
    orig = ops.pyramid_tail
    ops.pyramid_tail = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        for p in layer.parameters():
            p.grad = None
        xin = x.clone().requires_grad_(True)
        out = layer(xin)
        (out.float() * gout.to(out.device).float()).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.PYRAMID_TAIL_LOWRES = old
        ops.pyramid_tail = orig
    assert bool(calls) == lowres, "the switch did not select the route"
    got = {"out": out.detach(), "d input": xin.grad}
    for k, p in layer.named_parameters():
        if p.grad is not None:
            got["d " + k] = p.grad
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    worst, where = 0.0, None
    for k in ref:
        e = float((got[k].double().cpu() - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30))
        if e > worst:
            worst, where = e, k
    return worst, where


@pytest.mark.parametrize("dt,factor", [(torch.float32, 2.0), (torch.bfloat16, 1.5)])
@pytest.mark.parametrize("H,W", [(24, 32), (30, 40)])
def test_module_new_route_is_as_exact_as_the_old(H, W, dt, factor):
    from gw_depth_amd.model import PyramidLayer
    torch.manual_seed(3)
    layer = PyramidLayer(80).cuda()
    x = torch.randn(B, H, W, 80, generator=_gen("x", H, W)).to(dt).cuda()
    ref, gout = _oracle(layer, x)
    e_old, w_old = _route_error(layer, x, ref, gout, False)
    e_new, w_new = _route_error(layer, x, ref, gout, True)
    print("PyramidLayer(80) %dx%d %s: old route %.3e (%s), new route %.3e (%s), ratio %.3f" % (H, W, dt, e_old, w_old, e_new, w_new, e_new / e_old))
    assert e_new <= factor * e_old


# ------------------------------------------------------------------------------------------------------------------ capture
def test_new_route_in_a_captured_step_equals_the_eager_step():
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import synth_batch
    from tests.golden_check import build, rel, to_device
    old = ops.PYRAMID_TAIL_LOWRES
    ops.PYRAMID_TAIL_LOWRES = True
    calls = []
    orig = ops.pyramid_tail
    ops.pyramid_tail = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        b = to_device(synth_batch(2, 96, 128, seed=91, n_lines=[4, 6]), "cuda")
        res = []
        for graph in (False, True):
            cfg, model, crits = build(device="cuda")
            step = TrainStep(model, crits, cfg, compute_dtype=torch.float32, graph=graph, max_graphs=16)
            out, total, terms = step(b)
            torch.cuda.synchronize()
            if graph:
                assert step.graph_stats()["replays"] == 1 and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
            res.append((float(total), {k: float(v) for k, v in terms.items()}, step.flat_g.clone(), out["pred_depth"][-1].clone()))
    finally:
        ops.PYRAMID_TAIL_LOWRES = old
        ops.pyramid_tail = orig
    assert calls, "the step did not take the low-resolution route"
    (l0, t0, g0, d0), (l1, t1, g1, d1) = res
    print("loss %r %r  depth rel %.3e  flat_g rel %.3e" % (l0, l1, rel(d1, d0), rel(g1, g0)))
    assert abs(l0 - l1) <= 2e-5 * abs(l0)
    for k in t0:
        assert abs(t0[k] - t1[k]) <= 2e-5 * max(1.0, abs(t0[k])), k
    assert rel(d1, d0) < 2e-5
    assert rel(g1, g0) < 1e-3

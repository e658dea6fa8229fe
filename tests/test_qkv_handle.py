"""CPU: the packed qkv gradient of the 1/32 stage (model.WindowAttention) travels on an autograd edge.  ops.ref_scores(handle=True)
returns the projection again as a second output of its node; ops.window_attention_qkv, given that handle, leaves the q slot of the
packed gradient it returns unwritten, and ref_scores' backward receives that very tensor and writes (or zeroes) the q slot.  Compared
against the same pieces WITHOUT the handle, where each node returns a packed tensor with the other's slots zero-filled and autograd
adds the two: adding an exact zero changes no bit, so every comparison is torch.equal.  fp32 on tests/fake_device.py, dim 64,
2 images x 4 windows, R = 7 reference tokens."""
import pytest
import torch

from gw_depth_amd import hip, model as M, ops
from tests.fake_device import FakeDevice

DIM, IMAGES, NWIN, NREF = 64, 2, 4, 7


@pytest.fixture()
def fake():
    hip.set_library(FakeDevice())
    yield
    hip.set_library(None)


def compose(att, xw, x_ref, handle, detach_ra=False):
    """model.WindowAttention.forward from its own pieces -> (y, q_new, qkv).  handle False: ref_scores and window_attention_qkv both
    take the plain qkv, so autograd adds their two packed gradients.  detach_ra: no gradient reaches ref_scores through ra."""
    B_, N, C = xw.shape
    hd = C // M.HEADS
    qkv = att.qkv(xw).view(B_, N, 3, M.HEADS, hd)
    rq, rv = att.ref_qk(x_ref).split(C, dim=-1)
    ref_k = ops.row_affine(rq, att.diff_mu, att.diff_logsigma)
    if handle:
        ra, kv = ops.ref_scores(qkv, ref_k, rq.shape[0], att.scale, handle=True)
    else:
        ra, kv = ops.ref_scores(qkv, ref_k, rq.shape[0], att.scale), qkv
    if detach_ra:
        ra = ra.detach()
    for _ in range(3):
        upd, ra = ops.conv2d(ra, att.ref_attn_diffusion.weight, att.ref_attn_diffusion.bias, pad=1, fanout=True)
        ra = ops.inorm_gelu_residual(ra, upd, 1e-5)
    q_new = ops.ref_mix(ra, rv, M.HEADS).view(B_, N, M.HEADS, hd)
    y = att.proj(ops.window_attention_qkv(q_new, kv, att.relative_position_bias_table, att.rel_index(), None, 1, att.scale))
    return y, q_new, qkv


def problem():
    torch.manual_seed(0)
    att = M.WindowAttention(DIM)
    for p in att.parameters():
        torch.nn.init.normal_(p, std=0.2)
    g = torch.Generator().manual_seed(1)
    xw = (torch.randn(IMAGES * NWIN, 49, DIM, generator=g) * 0.5).requires_grad_(True)
    x_ref = (torch.randn(IMAGES, NREF, DIM, generator=g) * 0.5).requires_grad_(True)
    wgt = torch.randn(IMAGES * NWIN, 49, DIM, generator=g)
    return att, xw, x_ref, wgt, [xw, x_ref] + list(att.parameters())


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:          # no gradient on one side: none, or an exact zero, on the other (a node that ran hands zeros on)
            assert all(t is None or not t.any() for t in (x, y))
        else:
            assert torch.isfinite(x).all() and torch.equal(x, y)


def test_both_edges_live(fake):
    att, xw, x_ref, wgt, leaves = problem()
    y0 = att(xw, x_ref, None)                                                # the module itself asks for the handle
    g0 = torch.autograd.grad((y0 * wgt).sum(), leaves)
    y1, _, qkv1 = compose(att, xw, x_ref, handle=True)
    g1 = torch.autograd.grad((y1 * wgt).sum(), leaves + [qkv1])
    y2, _, qkv2 = compose(att, xw, x_ref, handle=False)
    g2 = torch.autograd.grad((y2 * wgt).sum(), leaves + [qkv2])
    assert torch.equal(y0, y2) and torch.equal(y1, y2)
    same(g0, g2[:-1])
    same(g1, g2)
    assert all(bool(g2[-1][:, :, i].abs().sum() > 0) for i in range(3))     # every slot of the packed gradient carries something


def test_ra_detached(fake):
    """Nothing reaches ref_scores through ra: its backward still runs for the handle, zeroes the q slot and passes the k / v slots on."""
    att, xw, x_ref, wgt, leaves = problem()
    res = []
    for handle in (True, False):
        y, _, qkv = compose(att, xw, x_ref, handle, detach_ra=True)
        res.append((y, torch.autograd.grad((y * wgt).sum(), leaves + [qkv], allow_unused=True)))
    assert torch.equal(res[0][0], res[1][0])
    same(res[0][1], res[1][1])
    gqkv = res[0][1][-1]
    assert bool((gqkv[:, :, 0] == 0).all()) and bool(gqkv[:, :, 1].abs().sum() > 0) and bool(gqkv[:, :, 2].abs().sum() > 0)
    assert res[0][1][0] is not None and bool(res[0][1][0].abs().sum() > 0)   # and it arrives at xw through the qkv Linear


def test_subset_of_inputs_then_full_backward(fake):
    """torch.autograd.grad with respect to q_new only never runs ref_scores' backward; nothing is left behind for the next backward."""
    att, xw, x_ref, wgt, leaves = problem()
    res = []
    for handle in (True, False):
        y, q_new, _ = compose(att, xw, x_ref, handle)
        gq = torch.autograd.grad((y * wgt).sum(), [q_new])
        y, _, qkv = compose(att, xw, x_ref, handle)                          # a fresh forward, backward in full
        res.append((gq, torch.autograd.grad((y * wgt).sum(), leaves + [qkv])))
    same(res[0][0], res[1][0])
    same(res[0][1], res[1][1])
    assert bool(res[0][0][0].abs().sum() > 0)

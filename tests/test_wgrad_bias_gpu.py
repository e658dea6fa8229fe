"""GPU: the bias gradient summed inside the LDS-DMA weight-gradient kernels (gwd_conv_desc.dbias).

All operands are small integers stored as bf16 - x in {-2 .. 2}, dY in {-3 .. 3} - so every product and every partial sum is an integer
below 2^24 and fp32 addition is exact in ANY order: dW and dbias must EQUAL the int64 reference, whatever order the atomics land in.
Every case runs with dbias NULL and with dbias set; dbias starts from a non-zero integer pattern (accumulated into, not overwritten)."""
import functools

import pytest
import torch

from gw_depth_amd import hip, ops

pytestmark = pytest.mark.gpu

# name: (B, Hi, Wi, Cin, Cout, k, stride); Linear = 1x1 on M one-pixel images.  M = 1031: a ragged last 32-pixel step and >= 2 reduction
# splits; N = 200 on the 128-wide tile: two N tiles, the second with 72 columns; K = 320: three K tiles (a bias counted once per K tile
# would come out 3x)
CASES = {
    "linear_128x128": (1031, 1, 1, 320, 200, 1, 1),
    "linear_64x64": (1031, 1, 1, 192, 48, 1, 1),
    "linear_32x128": (1031, 1, 1, 256, 24, 1, 1),
    "linear_160x128": (1031, 1, 1, 256, 160, 1, 1),      # single launch, never grouped
    "conv_fast1": (2, 12, 16, 16, 72, 3, 1),             # stride-1 'same' path
    "conv_fast0": (2, 13, 17, 16, 72, 3, 2),             # general gather
}


def _dims(B, Hi, Wi, Cin, Cout, k, stride):
    pad = k // 2
    return (B, Hi, Wi, Cin, (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1, Cout, k, k), pad


def _prefill(n):
    return (torch.arange(n) % 5 + 1).to(torch.float32)                      # 1 .. 5: never zero


@functools.lru_cache(maxsize=None)
def _problem(shape, seed=0):
    """Integer operands (CPU, int64) and the exact references, made once per shape and shared: (x, dy, dw_ref, db_ref)."""
    dims, pad = _dims(*shape)
    B, Hi, Wi, Cin, Ho, Wo, Cout, k, _ = dims
    stride = shape[6]
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randint(-2, 3, (B, Hi, Wi, Cin), generator=g)
    dy = torch.randint(-3, 4, (B, Ho, Wo, Cout), generator=g)
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    dw = torch.zeros((Cout, k, k, Cin), dtype=torch.int64)
    dyf = dy.reshape(-1, Cout)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :].reshape(-1, Cin)
            dw[:, kh, kw, :] = dyf.t() @ xs
    db = dyf.sum(0)
    assert int(dw.abs().max()) < 2 ** 24 and int(db.abs().max()) + 5 < 2 ** 24      # what makes "equal" a fair demand
    return x, dy, dw, db


def _device_operands(shape, seed=0):
    x, dy, dw, db = _problem(shape, seed)
    return x.to(torch.bfloat16).cuda(), dy.to(torch.bfloat16).cuda(), dw, db


def _run(lib, shape, with_bias, seed=0):
    dims, pad = _dims(*shape)
    x, dy, _, _ = _device_operands(shape, seed)
    dw = torch.zeros((dims[6], dims[7], dims[8], dims[3]), dtype=torch.float32, device="cuda")
    dbias = _prefill(dims[6]).cuda() if with_bias else None
    lib.conv_wgrad(x, dy, dw, dims, stride=shape[6], pad=pad, dbias=dbias)
    torch.cuda.synchronize()
    return dw.cpu(), None if dbias is None else dbias.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_single_call(name):
    lib = hip.library()
    shape = CASES[name]
    dims, pad = _dims(*shape)
    x, dy, dw_ref, db_ref = _device_operands(shape)
    assert lib.conv_wgrad_takes_bias(x, dy, dims, False, stride=shape[6], pad=pad)
    dw0, _ = _run(lib, shape, False)
    dw1, db1 = _run(lib, shape, True)
    print(name, "max |dW - ref|", float((dw1.double() - dw_ref.double()).abs().max()),
          "max |dbias - ref|", float((db1.double() - (db_ref.double() + _prefill(dims[6]).double())).abs().max()))
    assert torch.equal(dw0.to(torch.int64), dw_ref) and torch.equal(dw0, dw0.round())
    assert torch.equal(dw1, dw0)
    assert torch.equal(db1, db1.round()) and torch.equal(db1.to(torch.int64), db_ref + _prefill(dims[6]).to(torch.int64))


def _batch(lib, shapes, biased):
    """One gwd_conv_wgrad_batch call over shapes[i] (operand seed i); biased[i]: the job carries a dbias.  Returns the jobs' (dw, dbias)."""
    jobs, outs = [], []
    for i, shape in enumerate(shapes):
        dims, pad = _dims(*shape)
        x, dy, _, _ = _device_operands(shape, i)
        dw = torch.zeros((dims[6], dims[7], dims[8], dims[3]), dtype=torch.float32, device="cuda")
        dbias = _prefill(dims[6]).cuda() if biased[i] else None
        jobs.append((x, dy, dw, dims, dict(stride=shape[6], pad=pad, dbias=dbias)))
        outs.append((dw, dbias))
    lib.conv_wgrad_batch(jobs)
    torch.cuda.synchronize()
    return outs


def _check_batch(shapes, biased):
    lib = hip.library()
    plain = _batch(lib, shapes, [False] * len(shapes))
    outs = _batch(lib, shapes, biased)
    for i, shape in enumerate(shapes):
        _, _, dw_ref, db_ref = _problem(shape, i)
        assert torch.equal(plain[i][0].cpu().to(torch.int64), dw_ref), i
        assert torch.equal(outs[i][0], plain[i][0]), i
        if biased[i]:
            assert torch.equal(outs[i][1].cpu().to(torch.int64), db_ref + _prefill(shape[4]).to(torch.int64)), i


def test_batch_middle_job_without_bias():
    # three jobs of the 64 x 64 tile in one grouped launch; a bias written through the wrong job index lands in (or misses) job 0 / 2
    _check_batch([(1031, 1, 1, 192, 48, 1, 1), (517, 1, 1, 192, 48, 1, 1), (300, 1, 1, 128, 40, 1, 1)], [True, False, True])


def test_batch_crosses_the_group_boundary():
    # 17 biased jobs of one shape class: WG_GROUP = 16 go in the first grouped launch, the last one in a second
    _check_batch([(300, 1, 1, 64, 48, 1, 1)] * 17, [True] * 17)


def test_fp32_descriptor_with_bias_is_refused():
    lib = hip.library()
    x = torch.randint(-2, 3, (1031, 1, 1, 320)).float().cuda()
    dy = torch.randint(-3, 4, (1031, 1, 1, 200)).float().cuda()
    dims, _ = _dims(1031, 1, 1, 320, 200, 1, 1)
    assert not lib.conv_wgrad_takes_bias(x, dy, dims, False)
    dw = torch.zeros((200, 1, 1, 320), dtype=torch.float32, device="cuda")
    dbias = _prefill(200).cuda()
    with pytest.raises(RuntimeError, match="status -4"):
        lib.conv_wgrad(x, dy, dw, dims, dbias=dbias)
    with pytest.raises(RuntimeError, match="status -4"):
        lib.conv_wgrad_batch([(x, dy, dw, dims, dict(dbias=dbias))])
    torch.cuda.synchronize()
    assert not bool(dw.any()) and torch.equal(dbias.cpu(), _prefill(200))      # nothing was launched


def _param(t):
    """A parameter as engine.TrainStep manages it: its gradient accumulates into p._gwd_grad, p._gwd_hook fires when it has been enqueued."""
    p = torch.nn.Parameter(t.float().cuda())
    p._gwd_grad = torch.zeros_like(p.data)
    p._gwd_fired = []
    p._gwd_hook = lambda p=p: p._gwd_fired.append(1)
    return p


@pytest.mark.parametrize("name", ["linear_128x128", "conv_fast1", "conv_fast0"])
def test_ops_backward_queued_and_direct(name):
    shape = CASES[name]
    dims, pad = _dims(*shape)
    x, dy, dw_ref, db_ref = _device_operands(shape)
    Cout, Cin, k = dims[6], dims[3], dims[7]
    g = torch.Generator().manual_seed(7)
    w0 = torch.randint(-1, 2, (Cout, k, k, Cin), generator=g)
    b0 = torch.randint(-2, 3, (Cout,), generator=g)
    grads = []
    for queued in (True, False):
        w, b = _param(w0 if k > 1 else w0.view(Cout, Cin)), _param(b0)
        xin = x.view(-1, Cin) if k == 1 else x

        def step():
            y = ops.linear(xin, w, b) if k == 1 else ops.conv2d(xin, w, b, stride=shape[6], pad=pad)
            y.backward(dy.view(y.shape))

        if queued:
            with ops.COLSUMS, ops.WGRADS:
                step()
                assert not b._gwd_fired            # the bias rides with the queued weight-gradient job: not enqueued yet
        else:
            step()
        torch.cuda.synchronize()
        assert len(w._gwd_fired) == 1 and len(b._gwd_fired) == 1
        assert torch.equal(w._gwd_grad.cpu().to(torch.int64).view(dw_ref.shape), dw_ref)
        grads.append(b._gwd_grad.cpu())
    assert torch.equal(grads[0], grads[1])
    assert torch.equal(grads[0].to(torch.int64), db_ref)

"""GPU: graphs.GraphSide.capture on toy passes over tensors of 64 floats - no model, linear chains only.  A pass is a Python function
of the static input x that rewrites the state y in place; its eager run on the side stream is the reference, bit for bit."""
import pytest
import torch

from gw_depth_amd import graphs

pytestmark = pytest.mark.gpu
N = 64


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, generator=g).cuda(), torch.zeros(N, device="cuda")


def _fill(x, seed):
    x.copy_(torch.randn(N, generator=torch.Generator().manual_seed(seed)).cuda())


def _eager(side, run, y):
    with side.handover():
        run(None)
    torch.cuda.synchronize()
    return y.clone()


def _replayed(side, chain, y):
    y.fill_(float("nan"))                              # whatever the chain does not rewrite shows
    with side.handover():
        for g, _ in chain:
            g.replay()
    torch.cuda.synchronize()
    return y.clone()


def _two_updates(x, y, fail=False):
    def run(cut):
        y.copy_(x)
        y.mul_(3.0)
        if fail:
            raise ValueError("between two launches")
        if cut is not None:
            cut([0], False)
        y.addcmul_(x, x)
        if cut is not None:
            cut([1], True)
        return y
    return run


def _uncut(x, y, k):
    def run(cut):
        y.copy_(x)
        y.mul_(k)
        y.add_(x)
        return y
    return run


def test_cut_chain_replays_like_the_eager_pass():
    side = graphs.GraphSide()
    x, y = _tensors(1)
    run = _two_updates(x, y)
    _eager(side, run, y)                               # warm-up on the side stream
    chain, res = side.capture(run)
    assert res is y
    assert len(chain) == 2 and [ids for _, ids in chain] == [[0], [1]]          # no third, empty graph
    assert chain[0][0] is not chain[1][0]
    _fill(x, 2)
    want = _eager(side, run, y)
    torch.testing.assert_close(want, x * 3.0 + x * x)                           # the toy pass is what it says
    got = _replayed(side, chain, y)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the first segment alone stops at the cut
    y.fill_(float("nan"))
    with side.handover():
        chain[0][0].replay()
    torch.cuda.synchronize()
    assert torch.equal(y, x * 3.0)


def test_uncut_pass_is_one_graph_and_the_pool_is_shared():
    side = graphs.GraphSide()
    x1, y1 = _tensors(3)
    x2, y2 = _tensors(4)
    run1, run2 = _uncut(x1, y1, 2.0), _uncut(x2, y2, 5.0)
    _eager(side, run1, y1)
    chain1, _ = side.capture(run1)
    assert len(chain1) == 1 and chain1[0][1] == []
    pool = side._pool
    _eager(side, run2, y2)
    chain2, _ = side.capture(run2)
    assert len(chain2) == 1 and chain2[0][1] == [] and side._pool is pool and pool is not None
    _fill(x2, 5)
    want2 = _eager(side, run2, y2)
    assert torch.equal(_replayed(side, chain2, y2).view(torch.int32), want2.view(torch.int32))
    _fill(x1, 6)
    want1 = _eager(side, run1, y1)
    assert torch.equal(_replayed(side, chain1, y1).view(torch.int32), want1.view(torch.int32))     # the first one still replays
    assert torch.equal(y2.view(torch.int32), want2.view(torch.int32))                               # and left the second's state alone


def test_python_exception_ends_the_open_capture():
    """A ValueError between two launches of a captured pass: a Python exception, no device error.  The owner already holds a captured
    graph, as a session or a train step that meets a failing signature does: the caching allocator keeps a pool handle usable only
    while a graph captured out of it is alive, and the graph of the failed capture dies with the exception."""
    side = graphs.GraphSide()
    x0, y0 = _tensors(9)
    _eager(side, _uncut(x0, y0, 2.0), y0)
    held, _ = side.capture(_uncut(x0, y0, 2.0))
    pool = side._pool
    x, y = _tensors(7)
    _eager(side, _two_updates(x, y), y)
    with pytest.raises(ValueError, match="between two launches"):
        side.capture(_two_updates(x, y, fail=True))
    with torch.cuda.stream(side.stream()):
        assert not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
    assert side._pool is pool
    run = _two_updates(x, y)
    chain, _ = side.capture(run)                       # same stream, same pool
    assert [ids for _, ids in chain] == [[0], [1]]
    _fill(x, 8)
    want = _eager(side, run, y)
    assert torch.equal(_replayed(side, chain, y).view(torch.int32), want.view(torch.int32))
    want0 = _eager(side, _uncut(x0, y0, 2.0), y0)
    assert torch.equal(_replayed(side, held, y0).view(torch.int32), want0.view(torch.int32))       # the graph held before still replays

"""Trace witness of the conv-family autograd nodes (ops._ConvFn, _PadConvFn, _LayerNormFn, _ConvLnFn, _PyramidTailFn) and of the
Swin / class-token attention family (ops._WinAttnFn, _RefScoresFn, _RefMixFn, _TokAttnFn, _WindowMapFn).

A Recorder stands in for the device library (hip.set_library) and writes one text line per library method call: the method name,
the arguments without a default in order, every keyword whose value is not its default as `name=value`, scalars verbatim, every tensor
as `t<k>[+<storage offset>][<shape>]<dtype>[s[<strides>]]` (offset and strides where they are not 0 / contiguous; k numbers the
underlying storages in order of first appearance; the recorder keeps every tensor it has seen alive until the case ends, so an
address is never met again under another label) and the answer where the method gives one.  The parameters of a case carry
`_gwd_grad` / `_gwd_hook` as engine.TrainStep sets them; a hook writes `hook <parameter name>`.  After the backward one line
says which leaf gradients are None.  A refactor of ops.py that keeps the sequence of library calls, their operands and the hook
firings leaves every line as it is: tests/golden/autograd_trace.txt holds the lines, tools/make_autograd_trace.py writes them.

Two modes:
  dry (CPU suite)    nothing is computed, outputs stay as allocated; the methods that can decline (conv_forward with ln= or a GELU
                     gate, act_backward_colsum, layernorm_backward, stride_place, resample_backward with a gate,
                     resample_backward_sep, tokattn_pair_forward / _backward, window_map_multi) answer from the case's script, so
                     every fallback arm is forced without a special shape.
  delegating (gpu)   the same lines, every call forwarded to the real library, whose answers decide the path.

ATen operations that launch work are part of the trace in BOTH modes (`aten <operator> <shapes and scalars>`, through a
TorchDispatchMode; view operations and `empty` allocations are left out): autograd carries the dispatch mode over to the
backward's device thread, and the gpu sections of the golden file show the backward's `zeros` fills and `add`s.  What the real
library does inside a call (its zero page) is not logged.

CASES is the one list both modes use (the gpu-only cases need real answers or the x.is_cuda arms); ARMS, below it, names the case
that takes each arm of the nodes."""
import contextlib
import inspect

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from gw_depth_amd import hip, model, ops
from gw_depth_amd.hip import ACT_ELU, ACT_GELU, ACT_NONE, ACT_RELU

# the keyword defaults of a convolution descriptor: conv_forward / conv_wgrad take them as **kw
_DESC_DEFAULTS = {k: p.default for k, p in inspect.signature(hip.HipLibrary._desc).parameters.items() if p.default is not p.empty}
_EMPTY = {"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::new_empty", "aten::new_empty_strided"}


def _differs(v, default):
    return torch.is_tensor(v) or torch.is_tensor(default) or v != default


def _desc_kw(kw):
    return {k: v for k, v in kw.items() if _differs(v, _DESC_DEFAULTS[k])}


def _bound(name, args, kw):
    """The call in canonical form -> (values of the parameters without a default, {keyword: value} of those that differ from their
    default): a keyword left out and the same keyword given its default value are one call, and read the same."""
    sig = inspect.signature(getattr(hip.HipLibrary, name))
    ba = sig.bind(None, *args, **kw) if next(iter(sig.parameters), None) == "self" else sig.bind(*args, **kw)
    required, keywords = [], {}
    for k, v in ba.arguments.items():
        par = sig.parameters[k]
        if k == "self":
            continue
        if par.kind == par.VAR_KEYWORD:                 # conv_forward / conv_wgrad: the descriptor's keywords
            keywords.update(_desc_kw(v))
        elif par.kind == par.VAR_POSITIONAL:
            required += list(v)
        elif par.default is par.empty:
            required.append(v)
        elif _differs(v, par.default):
            keywords[k] = v
    if name == "conv_wgrad_batch":
        required = [[tuple(j[:4]) + (_desc_kw(j[4]),) for j in required[0]]]
    return required, keywords


def _x(sizes):
    return "x".join(str(int(v)) for v in sizes)


def _dt(t):
    return {torch.float32: "f32", torch.bfloat16: "bf16"}.get(t.dtype) or str(t.dtype).replace("torch.", "")


class Recorder:
    is_fake = True

    def __init__(self, real=None, script=None):
        self.real = real
        self.script = {k: list(v) for k, v in (script or {}).items()}
        self.lines, self.keep, self.labels, self.mute = [], [], {}, False

    def label(self, t):
        self.keep.append(t)
        key = (t.device.type, t.untyped_storage().data_ptr())
        k = self.labels.setdefault(key, len(self.labels))
        text = "t%d%s[%s]%s" % (k, "+%d" % t.storage_offset() if t.storage_offset() else "", _x(t.shape), _dt(t))
        return text if t.is_contiguous() else text + "s[%s]" % _x(t.stride())

    def fmt(self, v):
        if torch.is_tensor(v):
            return self.label(v)
        if isinstance(v, tuple) and v and all(isinstance(e, int) for e in v):
            return "(%s)" % _x(v)
        if isinstance(v, (list, tuple)):
            return ("[%s]" if isinstance(v, list) else "(%s)") % ", ".join(self.fmt(e) for e in v)
        if isinstance(v, dict):
            return "{%s}" % ", ".join("%s=%s" % (k, self.fmt(v[k])) for k in sorted(v))
        return repr(v)

    def _scripted(self, name, default=True):
        q = self.script.get(name)
        return q.pop(0) if q else default

    def _dry(self, name, args, kw):
        if name == "conv_forward":
            if kw.get("ln") is not None or (kw.get("gate") is not None and kw.get("gate_act") == ACT_GELU):
                return None if self._scripted(name) else False
            return None
        if name in ("act_backward_colsum", "stride_place", "resample_backward_sep", "tokattn_pair_forward", "tokattn_pair_backward",
                    "window_map_multi"):
            return self._scripted(name)
        if name == "layernorm_backward":
            return self._scripted(name) if (kw.get("gskip") is not None or kw.get("elu_input")) else True
        if name == "resample_backward":
            return self._scripted(name) if kw.get("gate") is not None else True
        if name == "pyr_tail_forward":
            return True
        if name == "colsum_batchable":
            return hip.HipLibrary.colsum_batchable(*args)
        if name == "workspace_bytes":
            n = 4
            for d in args[1:]:
                n *= int(d)
            return n
        if name == "conv_wgrad_takes_bias":
            return False
        return None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            required, keywords = _bound(name, args, kw)
            text = ", ".join([self.fmt(v) for v in required] + ["%s=%s" % (k, self.fmt(v)) for k, v in keywords.items()])
            if self.real is None:
                ret = self._dry(name, args, kw)
            else:
                muted, self.mute = self.mute, True
                try:
                    ret = getattr(self.real, name)(*args, **kw)
                finally:
                    self.mute = muted
            self.lines.append("%s(%s)%s" % (name, text, "" if ret is None else " -> %r" % (ret,)))
            return ret
        return call


class _AtenLog(TorchDispatchMode):
    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def _fmt(self, v):
        if torch.is_tensor(v):
            return "[%s]%s" % (_x(v.shape), _dt(v))
        if isinstance(v, (list, tuple)):
            return "[%s]" % ", ".join(self._fmt(e) for e in v)
        return str(v)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        schema = func._schema
        view = any(r.alias_info is not None and not r.alias_info.is_write for r in schema.returns)
        if not self.rec.mute and not view and schema.name not in _EMPTY:
            parts = [self._fmt(a) for a in args] + ["%s=%s" % (k, self._fmt(v)) for k, v in sorted(kwargs.items())
                                                     if v is not None and k not in ("device", "layout", "pin_memory")]
            self.rec.lines.append("aten %s %s" % (str(func).replace("aten.", "", 1), " ".join(parts)))
        return out


class Builder:
    """What a case body makes its leaves with: activations x(...), parameters p(name, ...) with or without a sink."""

    def __init__(self, rec, dev, dtype, seed):
        self.rec, self.dev, self.dtype = rec, dev, dtype
        self.gen = torch.Generator().manual_seed(seed)
        self.leaves = {}

    @contextlib.contextmanager
    def _muted(self):
        muted, self.rec.mute = self.rec.mute, True
        try:
            yield
        finally:
            self.rec.mute = muted

    def randn(self, *shape, dtype=None):
        with self._muted():
            return (torch.randn(*shape, generator=self.gen) * 0.5).to(dtype or self.dtype).to(self.dev)

    def leaf(self, t, grad=True):
        t.requires_grad_(grad)
        self.leaves["x%d" % sum(k.startswith("x") for k in self.leaves)] = t
        return t

    def x(self, *shape, grad=True):
        return self.leaf(self.randn(*shape), grad)

    def mult(self, *shape):
        with self._muted():
            return ((torch.rand(*shape, generator=self.gen) > 0.3).to(self.dtype) * 2).to(self.dev)

    def _register(self, name, p, sink):
        if sink:
            p._gwd_grad = torch.zeros_like(p.data)
            p._gwd_hook = lambda: self.rec.lines.append("hook %s" % name)
        self.leaves[name] = p
        return p

    def p(self, name, *shape, sink=True, ones=False):
        with self._muted():
            t = self.randn(*shape, dtype=torch.float32)
            return self._register(name, torch.nn.Parameter(t + 1.0 if ones else t), sink)

    def module(self, make, sink=True):
        """make() -> a module; its parameters become leaves under their named_parameters() names, with values from the case's generator."""
        with self._muted():
            m = make().to(self.dev)
            for name, p in m.named_parameters():
                p.data.copy_(self.randn(*p.shape, dtype=torch.float32))
                self._register(name, p, sink)
        return m


class Case:
    def __init__(self, name, body, script=None, queued=False, gpu_only=False, dtype=torch.float32, pooled=False):
        self.name, self.body, self.script, self.queued, self.gpu_only, self.dtype = name, body, script, queued or pooled, gpu_only, dtype
        self.pooled = pooled


def run_case(case, dev="cpu"):
    """The trace of one case as a list of lines.  dev 'cpu': dry mode; otherwise delegating mode on that device.  A queued case
    runs inside `with ops.COLSUMS, ops.WGRADS:`, a pooled one twice - the second pass takes its scratch from the pooled buffer, so the order of the
    WGRADS.scratch requests shows as offsets."""
    dry = dev == "cpu"
    real = None if dry else hip.library()
    rec = Recorder(real, case.script if dry else None)
    ops.WGRADS.__init__()
    ops.COLSUMS.__init__()
    capturing = torch.cuda.is_current_stream_capturing
    if dry:
        torch.cuda.is_current_stream_capturing = lambda: False          # WgradQueue.__exit__ asks; there is no device to ask here
    hip.set_library(rec)
    try:
        with _AtenLog(rec):
            for n in range(2 if case.pooled else 1):
                T = Builder(rec, dev, case.dtype, 1234 + n)
                if case.pooled:
                    rec.lines.append("pass %d" % n)
                with contextlib.ExitStack() as queues:
                    if case.queued:
                        queues.enter_context(ops.COLSUMS)
                        queues.enter_context(ops.WGRADS)
                    outs = case.body(T)
                    if outs is not None:
                        outs = [outs] if torch.is_tensor(outs) else list(outs)
                        gouts = [T.randn(*o.shape) for o in outs]
                        rec.lines.append("backward")
                        torch.autograd.backward(outs, gouts)
                if not dry:
                    torch.cuda.synchronize()
                if outs is not None:
                    rec.lines.append("grads None: " + " ".join("%s=%s" % (k, v.grad is None) for k, v in T.leaves.items()))
    finally:
        hip.set_library(real)
        torch.cuda.is_current_stream_capturing = capturing
        ops.WGRADS.__init__()
        ops.COLSUMS.__init__()
    left = {k: v for k, v in rec.script.items() if v}
    assert not left, "case %s: scripted answers nobody asked for: %r" % (case.name, left)
    return rec.lines


B, H, W, C = 1, 4, 6, 8


def _conv(act=ACT_NONE, bias=False, sink=True, res=False, mult=False, xgrad=True, **kw):
    def body(T):
        x = T.x(B, H, W, C, grad=xgrad)
        w = T.p("w", C, 3, 3, C, sink=sink)
        b = T.p("b", C, sink=sink) if bias else None
        r = T.x(B, H, W, C) if res else None
        m = T.mult(B, H, W, C) if mult else None
        return ops.conv2d(x, w, b, pad=1, act=act, residual=r, mult=m, **kw)
    return body


def _conv_fanout(g_in, xgrad=True):
    def body(T):
        x = T.x(B, H, W, C, grad=xgrad)
        y, x2 = ops.conv2d(x, T.p("w", C, 3, 3, C), pad=1, fanout=True)
        return (y, x2) if g_in else y
    return body


def _relu_pair(T):
    h = ops.conv2d(T.x(B, H, W, C), T.p("w0", C, 1, 1, C), T.p("b0", C), act=ACT_RELU, defer=True)
    return ops.conv2d(h, T.p("w1", C, 3, 3, C), pad=1, in_gate=ACT_RELU)


def _gelu_mlp(T):
    h, z = ops.linear(T.x(B, H * W, C), T.p("w1", 16, C), T.p("b1", 16), act=ACT_GELU, defer=True)
    return ops.linear(h, T.p("w2", C, 16), T.p("b2", C), in_gate=ACT_GELU, gate_src=z)


def _gelu_producer_unconsumed(T):
    # the producer's output is only the dropout multiplier of another layer, which has no gradient: its backward gets gy = None
    h, z = ops.linear(T.x(B * H * W, C), T.p("w1", C, C), T.p("b1", C), act=ACT_GELU, defer=True)
    return ops.conv2d(T.x(B, H, W, C), T.p("w", C, 1, 1, C), mult=h.view(B, H, W, C))


def _linear_rows(T):
    return ops.linear(T.x(B, H * W, C), T.p("w", 3 * C, C), T.p("b", 3 * C), rows=(C, 2 * C))


def _row_scale(sink):
    def body(T):
        rs, sh = T.randn(C, dtype=torch.float32), T.randn(C, dtype=torch.float32)
        return ops.conv2d(T.x(B, H, W, C), T.p("w", C, 3, 3, C, sink=sink), pad=1, act=ACT_RELU, row_scale=rs, shift=sh)
    return body


def _stride2(fan):
    def body(T):
        x = T.x(B, H, W, C)
        if fan:
            return ops.conv2d(x, T.p("w", C, 1, 1, C), stride=2, fanout=True)
        return ops.conv2d(x, T.p("w", C, 1, 1, C), stride=2)
    return body


def _upsampled(gate, skip):
    def body(T):
        x = T.x(B, H, W, C)
        if gate:
            x = ops.conv2d(x, T.p("w0", C, 1, 1, C), act=ACT_RELU, defer=True)
        g = ACT_RELU if gate else ACT_NONE
        if skip:
            return ops.conv2d(x, T.p("w", C, 3, 3, C), pad=1, upsample_to=(2 * H, 2 * W), in_gate=g, fanout=True)
        return ops.conv2d(x, T.p("w", C, 3, 3, C), pad=1, upsample_to=(2 * H, 2 * W), in_gate=g)
    return body


def _upsampled_general(T):
    return ops.conv2d(T.x(B, H, W, C), T.p("w", C, 3, 3, C, sink=False), T.p("b", C, sink=False), pad=1, upsample_to=(3 * H, 2 * W))


GEOM = (8, 6, 8)        # 6 real channels in and out, each padded to 8


def _padded(sink=True, fan=False, xgrad=True):
    def body(T):
        x = T.x(B, H, W, 8, grad=xgrad)
        w = T.p("w", 6, 3, 3, 6, sink=sink)
        return ops.conv2d_padded(x, w, 1, GEOM, fanout=True) if fan else ops.conv2d_padded(x, w, 1, GEOM)
    return body


def _ln(C_aff=C, sink=True, affine=True, gelu=False, res=False, fan=False, elu=False):
    def body(T):
        x = T.x(B, H, W, C)
        if elu:
            x = ops.conv2d(x, T.p("w0", C, 1, 1, C), act=ACT_ELU, defer=True)
        g = T.p("gamma", C_aff, sink=sink, ones=True) if affine else None
        b = T.p("beta", C_aff, sink=sink) if affine else None
        r = T.x(B, H, W, C) if res else None
        return ops.layer_norm(x, g, b, gelu=gelu, residual=r, fanout=fan, in_gate=ACT_ELU if elu else ACT_NONE)
    return body


def _conv_ln(geom=None, sink=True, res=False, fan=False, gelu=False, infer=False):
    def body(T):
        n = 6 if geom else C
        x = T.x(B, H, W, C, grad=not infer)
        w, g, b = T.p("w", n, 3, 3, n, sink=sink), T.p("gamma", n, sink=sink, ones=True), T.p("beta", n, sink=sink)
        r = T.x(B, H, W, C) if res else None
        if infer:
            with torch.no_grad():
                ops.conv_ln(x, w, g, b, 1, gelu=gelu, geom=geom)
            return None
        return ops.conv_ln(x, w, g, b, 1, gelu=gelu, residual=r, geom=geom, fanout=fan)
    return body


def _tail(nlow, sink=True):
    def body(T):
        N, C2 = 32, 8
        x = T.x(B, 8, 8, C2)
        ys = [T.x(B, 2, 2, C2), T.x(B, 4, 4, C2)]
        w, g, b = T.p("w", N, 3, 3, 3 * C2, sink=sink), T.p("gamma", N, sink=sink, ones=True), T.p("beta", N, sink=sink)
        return ops.pyramid_tail(x, ys, w, g, b, gelu=True, nlow=nlow)
    return body


# ---- gpu only: the x.is_cuda arms and real declines
def _up2x_bf16(T):
    return ops.conv2d(T.x(B, 8, 8, 16), T.p("w", 16, 3, 3, 16), T.p("b", 16), pad=1, act=ACT_RELU, upsample_to=(16, 16))


def _bias_in_wgrad(T):
    return ops.linear(T.x(300, 64), T.p("w", 48, 64), T.p("b", 48))


def _cout6_bf16(T):
    return ops.conv2d(T.x(B, H, W, C), T.p("w", 6, 3, 3, C), T.p("b", 6), pad=1, act=ACT_RELU)


def _ln6_bf16(T):
    return ops.layer_norm(T.x(B, H, W, 6), T.p("gamma", 6, ones=True), T.p("beta", 6), fanout=True)


# ---- the Swin / class-token attention family: 2 windows of 49 tokens, 16 heads of 4 channels (dim 64), token width e = 12, R = 7
NW, NT, HD, TE, NREF = 2, 49, 4, 12, 7
DIM = model.HEADS * HD
RHD = 8                     # the ref_scores kernels of the device start at head dim 8: the cases that run them use dim 128
RDIM = model.HEADS * RHD


def _win_operands(T, sink, region):
    """table parameter, rel index, region table, windows per image, scale"""
    table = T.p("table", (2 * model.WS - 1) ** 2, model.HEADS, sink=sink)
    with T._muted():
        rel = model.relative_position_index().reshape(-1).to(torch.int32).to(T.dev)
        reg = (torch.arange(NW * NT, dtype=torch.int32).view(NW, NT) % 3).to(T.dev) if region else None
    return table, rel, reg, (NW if region else 1), HD ** -0.5


def _win_packed(sink=True, region=False):
    def body(T):
        return ops.window_attention_packed(T.x(NW, NT, 3, model.HEADS, HD), *_win_operands(T, sink, region))
    return body


def _win_separate(sink=True, region=False, strided=False):
    def body(T):
        q = T.x(NW, NT, HD, model.HEADS).transpose(2, 3) if strided else T.x(NW, NT, model.HEADS, HD)      # strided: no unit channel stride
        return ops.window_attention(q, T.x(NW, NT, model.HEADS, HD), T.x(NW, NT, model.HEADS, HD), *_win_operands(T, sink, region))
    return body


def _win_query(sink=True, region=False):
    def body(T):
        return ops.window_attention_qkv(T.x(NW, NT, model.HEADS, HD), T.x(NW, NT, 3, model.HEADS, HD), *_win_operands(T, sink, region))
    return body


def _win_block(sink=True, region=False):
    """model.WindowAttention whole: ref_scores and window_attention_qkv share ONE packed qkv gradient."""
    def body(T):
        att = T.module(lambda: model.WindowAttention(RDIM), sink=sink)
        with T._muted():
            att.rel_index()
            reg = (torch.arange(NW * NT, dtype=torch.int32).view(NW, NT) % 3).to(T.dev) if region else None
        return att(T.x(NW, NT, RDIM), T.x(1, NREF, RDIM), reg)
    return body


def _ref_alone(T):
    ra = ops.ref_scores(T.x(NW, NT, 3, model.HEADS, RHD), T.x(1, NREF, RDIM), 1, RHD ** -0.5)
    return ops.ref_mix(ra, T.x(1, NREF, RDIM), model.HEADS)


def _tok_single(T):
    return ops.token_attention(T.x(NW, NT, model.HEADS, 4), T.x(NW, NT, model.HEADS, TE), T.x(NW, NT, model.HEADS, TE), 0.5)


def _tok_pair(T):
    return ops.token_attention_pair(T.x(NW, NT, model.HEADS, 4), T.x(NW, NT, model.HEADS, 4), T.x(NW, NT, model.HEADS, TE),
                                    T.x(NW, NT, model.HEADS, TE), 0.5)


def _tok_pair_misaligned(T):
    # the operands of test_token_attention_pair_declined_falls_back[offset_4_bytes]: q starts 4 bytes past an 8-byte boundary
    nwin, e = 5, 16
    q = T.leaf(T.randn(nwin * NT * model.HEADS * 4 + 2)[2:].view(nwin, NT, model.HEADS, 4))
    return ops.token_attention_pair(q, T.x(nwin, NT, model.HEADS, 4), T.x(nwin, NT, model.HEADS, e), T.x(nwin, NT, model.HEADS, e), 0.5)


MB, MH, MW = 1, 8, 10        # padded to 14 x 14: 4 windows


def _map_single(shift, res):
    def body(T):
        win = ops.window_gather(T.x(MB, MH, MW, DIM), shift)
        return ops.window_scatter(win, MB, MH, MW, shift, residual=T.x(MB, MH * MW, DIM) if res else None)
    return body


def _map_multi(shift, Cs=(DIM, 64, 64), res=(True, True, True)):
    def body(T):
        wins = ops.window_gather_multi([T.x(MB, MH, MW, c) for c in Cs], shift)
        return ops.window_scatter_multi(list(wins), MB, MH, MW, shift, [T.x(MB, MH * MW, c) if r else None for c, r in zip(Cs, res)])
    return body


BF16 = torch.bfloat16

CASES = [
    # conv2d / linear
    Case("conv_plain_nosink", _conv(sink=False)),
    Case("conv_plain_sink", _conv()),
    Case("conv_plain_sink_queued", _conv(bias=True), queued=True),
    Case("conv_relu_bias_sink", _conv(ACT_RELU, bias=True)),
    Case("conv_relu_bias_sink_declined", _conv(ACT_RELU, bias=True), script={"act_backward_colsum": [False]}),
    Case("conv_relu_bias_sink_declined_queued", _conv(ACT_RELU, bias=True), script={"act_backward_colsum": [False]}, queued=True),
    Case("conv_gelu_bias_nosink", _conv(ACT_GELU, bias=True, sink=False)),
    Case("conv_act_scale", _conv(ACT_NONE, act_scale=2.0)),
    Case("conv_bias_residual", _conv(bias=True, res=True)),
    Case("conv_w_only", _conv(ACT_RELU, bias=True, res=True, xgrad=False)),
    Case("conv_mult_relu_bias_sink", _conv(ACT_RELU, bias=True, mult=True)),
    Case("conv_mult_relu_declined_then_taken", _conv(ACT_RELU, bias=True, mult=True), script={"act_backward_colsum": [False, True]}),
    Case("conv_mult_relu_declined_twice", _conv(ACT_RELU, bias=True, mult=True), script={"act_backward_colsum": [False, False]}),
    Case("conv_mult_residual_bias_sink", _conv(bias=True, res=True, mult=True)),
    Case("conv_mult_residual_declined", _conv(bias=True, res=True, mult=True), script={"act_backward_colsum": [False]}),
    Case("conv_mult_nobias", _conv(ACT_RELU, mult=True)),
    Case("conv_mult_bias_nosink", _conv(ACT_RELU, bias=True, mult=True, sink=False)),
    Case("conv_fanout_g_in", _conv_fanout(True)),
    Case("conv_fanout_alone", _conv_fanout(False)),
    Case("conv_fanout_g_in_no_input_grad", _conv_fanout(True, xgrad=False)),
    Case("relu_defer_in_gate", _relu_pair),
    Case("gelu_mlp_gated", _gelu_mlp),
    Case("gelu_mlp_gate_declined", _gelu_mlp, script={"conv_forward": [False]}),
    Case("gelu_mlp_queued", _gelu_mlp, queued=True),
    Case("gelu_producer_unconsumed", _gelu_producer_unconsumed),
    Case("linear_rows", _linear_rows),
    Case("conv_row_scale_shift_sink", _row_scale(True)),
    Case("conv_row_scale_shift_nosink", _row_scale(False)),
    Case("conv_1x1_stride2", _stride2(False)),
    Case("conv_1x1_stride2_fanout", _stride2(True)),
    Case("conv_1x1_stride2_declined", _stride2(True), script={"stride_place": [False]}),
    Case("upsampled_general", _upsampled_general),
    Case("upsampled_2x", _upsampled(False, False)),
    Case("upsampled_2x_skip", _upsampled(False, True)),
    Case("upsampled_gate", _upsampled(True, False)),
    Case("upsampled_gate_declined", _upsampled(True, False), script={"resample_backward": [False]}),
    Case("upsampled_gate_skip", _upsampled(True, True)),
    # conv2d_padded
    Case("padded_sink", _padded()),
    Case("padded_nosink", _padded(sink=False)),
    Case("padded_sink_queued", _padded(fan=True), pooled=True),
    Case("padded_fanout", _padded(fan=True)),
    Case("padded_fanout_no_input_grad", _padded(fan=True, xgrad=False)),
    # layer_norm
    Case("ln_gelu_sink", _ln(gelu=True)),
    Case("ln_residual_nosink", _ln(sink=False, res=True)),
    Case("ln_fanout", _ln(fan=True)),
    Case("ln_fanout_declined", _ln(fan=True), script={"layernorm_backward": [False]}),
    Case("ln_elu_gate", _ln(elu=True)),
    Case("ln_elu_gate_declined", _ln(elu=True), script={"layernorm_backward": [False]}),
    Case("ln_elu_gate_fanout_declined", _ln(elu=True, fan=True, sink=False), script={"layernorm_backward": [False]}),
    Case("ln_pitch", _ln(C_aff=6)),
    Case("ln_no_affine", _ln(affine=False)),
    # conv_ln
    Case("conv_ln_fused", _conv_ln()),
    Case("conv_ln_declined", _conv_ln(gelu=True), script={"conv_forward": [False]}),
    Case("conv_ln_nosink_residual", _conv_ln(sink=False, res=True)),
    Case("conv_ln_fanout_queued", _conv_ln(fan=True), queued=True),
    Case("conv_ln_geom_sink", _conv_ln(geom=GEOM, gelu=True)),
    Case("conv_ln_geom_nosink_declined", _conv_ln(geom=GEOM, sink=False), script={"conv_forward": [False]}),
    Case("conv_ln_geom_fanout_queued", _conv_ln(geom=GEOM, fan=True, res=True), pooled=True),
    Case("conv_ln_inference", _conv_ln(infer=True)),
    Case("conv_ln_inference_declined", _conv_ln(infer=True, geom=GEOM), script={"conv_forward": [False]}),
    # pyramid_tail
    Case("tail_nlow1_sink", _tail(1)),
    Case("tail_nlow1_sep_declined", _tail(1), script={"resample_backward_sep": [False]}),
    Case("tail_nlow2_nosink", _tail(2, sink=False)),
    Case("tail_nlow1_queued", _tail(1), pooled=True),
    Case("tail_nlow2_queued", _tail(2), pooled=True),
    # gpu only
    Case("gpu_up2x_bf16", _up2x_bf16, gpu_only=True, dtype=BF16),
    Case("gpu_up2x_bf16_queued", _up2x_bf16, pooled=True, gpu_only=True, dtype=BF16),
    Case("gpu_up2x_bf16_gate_skip", _upsampled(True, True), gpu_only=True, dtype=BF16),
    Case("gpu_bias_in_wgrad_bf16", _bias_in_wgrad, gpu_only=True, dtype=BF16),
    Case("gpu_bias_in_wgrad_bf16_queued", _bias_in_wgrad, queued=True, gpu_only=True, dtype=BF16),
    Case("gpu_bias_not_in_wgrad_fp32", _bias_in_wgrad, gpu_only=True),
    Case("gpu_cout6_bf16_colsum_declines", _cout6_bf16, gpu_only=True, dtype=BF16),
    Case("gpu_ln6_bf16_skip_declines", _ln6_bf16, gpu_only=True, dtype=BF16),
    # window attention
    Case("win_packed_sink", _win_packed()),
    Case("win_packed_nosink", _win_packed(sink=False)),
    Case("win_packed_region", _win_packed(region=True)),
    Case("win_packed_queued", _win_packed(), pooled=True),
    Case("win_separate_sink", _win_separate()),
    Case("win_separate_nosink_region", _win_separate(sink=False, region=True)),
    Case("win_separate_strided_q", _win_separate(strided=True)),
    Case("win_separate_queued", _win_separate(), pooled=True),
    Case("win_query_sink", _win_query()),
    Case("win_query_nosink", _win_query(sink=False)),
    Case("win_query_region", _win_query(region=True)),
    Case("win_query_queued", _win_query(), pooled=True),
    Case("win_block_sink", _win_block()),
    Case("win_block_nosink_region", _win_block(sink=False, region=True)),
    Case("win_block_queued", _win_block(), pooled=True),
    Case("ref_scores_mix_alone", _ref_alone),
    Case("gpu_win_packed_bf16", _win_packed(), gpu_only=True, dtype=BF16),
    Case("gpu_win_packed_bf16_nosink_queued", _win_packed(sink=False), pooled=True, gpu_only=True, dtype=BF16),
    Case("gpu_win_query_bf16", _win_query(), gpu_only=True, dtype=BF16),
    Case("gpu_win_query_bf16_nosink_queued", _win_query(sink=False), pooled=True, gpu_only=True, dtype=BF16),
    Case("gpu_win_block_bf16_queued", _win_block(), pooled=True, gpu_only=True, dtype=BF16),
    # token attention
    Case("tok_single", _tok_single),
    Case("tok_pair_taken", _tok_pair, dtype=BF16),
    Case("tok_pair_forward_declined", _tok_pair, script={"tokattn_pair_forward": [False]}, dtype=BF16),
    Case("tok_pair_backward_declined", _tok_pair, script={"tokattn_pair_backward": [False]}, dtype=BF16),
    Case("tok_pair_fp32_two_singles", _tok_pair),
    Case("gpu_tok_pair_misaligned_q_declines", _tok_pair_misaligned, gpu_only=True, dtype=BF16),
    # window maps
    Case("map_single", _map_single(0, False)),
    Case("map_single_shift_residual", _map_single(3, True)),
    Case("map_multi_taken", _map_multi(3)),
    Case("map_multi_declined", _map_multi(0), script={"window_map_multi": [False, False, False, False]}),
    Case("map_multi_one_residual_none", _map_multi(3, res=(True, False, True))),
    Case("gpu_map_multi_fp32_width6_declines", _map_multi(3, Cs=(16, 6, 6), res=(True, False, True)), gpu_only=True),
]
ARMS = """Which case takes which arm (dry mode unless the name starts with gpu_).

_ConvFn.forward     no virt / upsample_to: conv_plain_* / upsampled_*;  bias, shift_const, both: conv_relu_bias_sink,
                    conv_row_scale_shift_*, -;  z for GELU: conv_gelu_bias_nosink;  residual, mult: conv_bias_residual, conv_mult_*;
                    defer GELU returns (y, z): gelu_mlp_*;  z = y where no gradient is wanted: -;  fanout: conv_fanout_*
_ConvFn.backward    gy None: gelu_producer_unconsumed
  fan-in            g_in given: conv_fanout_g_in;  none: conv_fanout_alone (autograd materialises zeros) and every case without fanout
  activation, dropout, bias
                    mult + bias sink, one pass taken: conv_mult_relu_bias_sink, conv_mult_residual_bias_sink
                    declined -> gy * mult -> second attempt taken / declined -> act_backward: conv_mult_relu_declined_then_taken / _twice
                    declined, no activation behind it (no second attempt): conv_mult_residual_declined
                    mult without bias sink: conv_mult_nobias, conv_mult_bias_nosink
                    defer (dv = gy): relu_defer_in_gate, gelu_mlp_*
                    colsum pass taken / declined: conv_relu_bias_sink / conv_relu_bias_sink_declined(_queued)
                    activation without a bias sink: conv_gelu_bias_nosink, conv_act_scale;  dv = gy: conv_plain_*
  data gradient     4x4 / stride 2 (x.is_cuda, bf16): gpu_up2x_bf16(_queued);  with gate and skip it is not taken: gpu_up2x_bf16_gate_skip
                    up-sampled general: upsampled_general, upsampled_2x;  gate on the footprint sum taken / declined: upsampled_gate /
                    upsampled_gate_declined;  skip: upsampled_2x_skip;  gate behind the skip: upsampled_gate_skip
                    1x1 stride s placed / declined: conv_1x1_stride2(_fanout) / conv_1x1_stride2_declined
                    transposed gather: conv_plain_*;  ReLU gate: relu_defer_in_gate;  GELU gate taken / declined: gelu_mlp_gated /
                    gelu_mlp_gate_declined;  no input gradient, g_in or none: conv_fanout_g_in_no_input_grad / conv_w_only
  weight, bias      4x4 form + fold hook: gpu_up2x_bf16(_queued);  sink: conv_plain_sink;  bias rides, _both hooks:
                    gpu_bias_in_wgrad_bf16(_queued);  refused: gpu_bias_not_in_wgrad_fp32;  no sink: conv_plain_nosink
                    COLSUMS.add direct / queued: conv_bias_residual / conv_plain_sink_queued;  colsum without sink: conv_gelu_bias_nosink
                    residual gradient dv / g_skip: conv_bias_residual / conv_mult_residual_*
                    real decline of gwd_act_backward_colsum (Cout = 6, bf16): gpu_cout6_bf16_colsum_declines
                    rows= slices of the sinks: linear_rows;  row_scale: conv_row_scale_shift_*
_PadConvFn          sink / none: padded_sink / padded_nosink;  fanout: padded_fanout;  pooled scratch: padded_sink_queued;
                    no input gradient but g_in: padded_fanout_no_input_grad
_LayerNormFn        gelu: ln_gelu_sink;  residual, no sinks: ln_residual_nosink;  fanout taken / declined: ln_fanout / ln_fanout_declined;
                    ELU gate taken / declined / declined behind a skip: ln_elu_gate / ln_elu_gate_declined / ln_elu_gate_fanout_declined;
                    pitch: ln_pitch;  no affine: ln_no_affine;  real decline (C = 6, bf16, skip): gpu_ln6_bf16_skip_declines
_ConvLnFn           fused / declined forward: conv_ln_fused / conv_ln_declined;  geom: conv_ln_geom_*;  sinks absent:
                    conv_ln_nosink_residual, conv_ln_geom_nosink_declined;  residual, fanout: conv_ln_nosink_residual,
                    conv_ln_fanout_queued, conv_ln_geom_fanout_queued;  inference (z not written / written by the fallback):
                    conv_ln_inference / conv_ln_inference_declined
_PyramidTailFn      nlow < branches (concat forward / backward, separable resample taken / declined): tail_nlow1_sink /
                    tail_nlow1_sep_declined;  nlow == branches, no sinks: tail_nlow2_nosink;  pooled scratch: tail_nlow*_queued
_WinAttnFn          q / k / v all slots of qkv: win_packed_*;  all given: win_separate_*;  q given, k / v slots: win_query_*, win_block_*
                    operand without a unit channel stride copied: win_separate_strided_q;  region table (2 windows per image): *_region
                    free q slot of the packed gradient zero-filled: win_query_*;  left to ref_scores' backward: win_block_*
  table gradient    sink / fresh zeros (dry: straight into either): *_sink / *_nosink;  head-major scratch, transposed add into the sink /
                    transposed copy (tb.is_cuda): gpu_win_packed_bf16, gpu_win_query_bf16 / gpu_win_*_bf16_nosink_queued and the gpu
                    sections of every win_* case;  pooled scratch offsets: *_queued
_RefScoresFn        packed gradient arrives on the handle's edge, q slot written into it: win_block_* (gpu_win_block_bf16_queued);
                    no handle, zeros_like: ref_scores_mix_alone;  ra without a gradient (q slot zeroed): tests/test_qkv_handle.py
_RefMixFn           win_block_*, ref_scores_mix_alone
_TokAttnFn          one query: tok_single, tok_pair_fp32_two_singles (two nodes, autograd adds gk / gv);  pair taken both ways:
                    tok_pair_taken;  forward declined / backward declined (singles, gk / gv summed in the node): tok_pair_forward_declined
                    / tok_pair_backward_declined;  real decline both ways (q 4 bytes past an 8-byte boundary): gpu_tok_pair_misaligned_q_declines
_WindowMapFn        one map (window_map, window_map_multi never asked), without / with residual, shift 0 / 3: map_single /
                    map_single_shift_residual;  several maps joint / declined four times (per map): map_multi_taken / map_multi_declined;
                    a residual None: map_multi_one_residual_none;  real decline (fp32 rows of 6 channels): gpu_map_multi_fp32_width6_declines
"""


SAME_AS_CPU = "same as cpu"


def sections(text):
    """Golden file -> {section name: [lines]}; a section starts with `== <mode> <case>`; a gpu section that reads SAME_AS_CPU holds
    the lines of the case's cpu section."""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        elif cur is not None:
            cur.append(line)
    return {k: (out["cpu " + k[4:]] if v == [SAME_AS_CPU] else v) for k, v in out.items()}


def compare(name, fresh, golden):
    """Line by line; prints and reports the first differing line."""
    for i in range(max(len(fresh), len(golden))):
        a = fresh[i] if i < len(fresh) else "<end of trace>"
        b = golden[i] if i < len(golden) else "<end of trace>"
        if a != b:
            msg = "%s: line %d differs\n  fresh : %s\n  golden: %s" % (name, i + 1, a, b)
            print(msg)
            return msg
    return None

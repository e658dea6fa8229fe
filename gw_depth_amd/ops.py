"""torch.autograd.Function wrappers over the C ABI (include/gwdepth.h).

Layout conventions: feature maps are (B, H, W, C) contiguous ("pixel-major"), token tensors
(..., C) contiguous; conv weights are (Cout, KH, KW, Cin); Linear weights (out, in) as in torch.
Master parameters are fp32; with bf16 activations the kernels read a bf16 copy of the weights
(the flat shadow maintained by the fused optimizer when present, otherwise made on the fly).
"""
import bisect
import os

import torch
import torch.nn.functional as F

from . import hip
from .hip import (ACT_ELU, ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, GATHER_CONV, GATHER_TRANSPOSED,
                  GATHER_UPSAMPLED)

__all__ = ["conv2d", "linear", "layer_norm", "softmax_lastdim", "silog_loss", "seg_cross_entropy",
           "ACT_NONE", "ACT_RELU", "ACT_GELU", "ACT_ELU", "ACT_SIGMOID"]


def _lib():
    return hip.library()


class WeightCache:
    """bf16 kernel-side copies of the conv / linear weights (row-scaled forward copy for folded FrozenBN, transposed
    copy for the data gradient), refreshed by ONE gwd_weight_prep_batch launch per train step instead of one small
    launch per layer.  engine.TrainStep owns one and runs each forward/backward inside `with cache:` (begin_pass() / end_pass());
    outside such a pass (plain ops calls, fp32 runs) every copy is made on the fly as before.  A weight first seen inside a pass is
    prepared on the fly and joins the table for the next pass.

    frozen=True (infer.InferenceSession): the weights do not change between passes.  begin_pass() only activates the cache
    and launches nothing: a copy is made when its weight is first seen (the first pass) and stays as it is.  refresh() runs
    the one batch launch and rewrites every copy IN PLACE (a captured HIP graph reads them by address).  A frozen cache also
    answers for weights that carry a TrainStep's bf16 shadow (see _weight_for): the shadow follows every optimizer step, the
    frozen copies follow refresh() only."""

    def __init__(self, persistent=(), frozen=False):
        self.frozen = bool(frozen)
        self._derived = {}       # frozen mode: (parameter address, tag) -> (maker, tensor), see derived()
        # [start, end) address ranges of PARAMETER storage: only weights living there are cached - a temporary (e.g. a
        # zero-padded copy of a parameter) has a new address every step and must be prepared on the fly
        self.ranges = sorted((int(a), int(b)) for a, b in persistent)
        self._starts, self._ends, self._merged_from = [], [], -1
        self.jobs = {}           # key -> dict(w, rs, fwd, t)
        self.table = None
        self.n_jobs = self.blocks = 0
        self.dirty = False
        self.active = False
        self._retired = []

    @staticmethod
    def _key(w, rs, geom=None):
        return (w.data_ptr(), tuple(w.shape), 0 if rs is None else rs.data_ptr(), geom)

    def get(self, w, rs, kind, geom=None):
        """kind 'fwd' | 't' -> cached tensor, or None when the cache is not in a pass / not applicable.
        geom = (Np, Cg, Cgp): the zero-padded copies of padded_weight()."""
        if not self.active or not w.is_cuda or w.dtype != torch.float32:
            return None
        if not self._persistent(w.data_ptr()):
            return None
        job = self.jobs.get(self._key(w, rs, geom))
        if job is not None and job[kind] is not None:
            return job[kind]        # refreshed by this pass's batch launch, or made earlier in this very pass
        return self._add(w, rs, kind, geom)

    def _persistent(self, p):
        """p lies in one of the [start, end) ranges.  Bisection over the merged ranges: a session registers one range per
        parameter and buffer, and every weight of a forward asks."""
        if self._merged_from != len(self.ranges):
            merged = []
            for lo, hi in sorted(self.ranges):
                if merged and lo <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], hi)
                else:
                    merged.append([lo, hi])
            self._starts, self._ends, self._merged_from = [m[0] for m in merged], [m[1] for m in merged], len(self.ranges)
        i = bisect.bisect_right(self._starts, p) - 1
        return i >= 0 and p < self._ends[i]

    def _add(self, w, rs, kind, geom=None):
        key = self._key(w, rs, geom)
        job = self.jobs.get(key)
        if job is None:
            job = self.jobs[key] = {"w": w.detach(), "rs": rs, "fwd": None, "t": None, "geom": geom}
        N, C = w.shape[0], w.shape[-1]
        taps = w.numel() // (N * C)
        if geom is not None:
            # the padding is written here, once; the per-step batch launch refreshes the real entries only
            job[kind] = padded_weight(w.detach(), geom, kind, torch.bfloat16)
            self.dirty = True
            return job[kind]
        if kind == "fwd":
            out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
            _lib().weight_prep(w.detach(), rs, out, None, N, taps, C, hip.BF16)
        else:
            out = torch.empty((C,) + tuple(w.shape[1:-1]) + (N,), dtype=torch.bfloat16, device=w.device)
            _lib().weight_prep(w.detach(), rs, None, out, N, taps, C, hip.BF16)
        job[kind] = out
        self.dirty = True
        return out

    def _build_table(self):
        if self.dirty and self.jobs:
            recs = (hip.PrepJob * len(self.jobs))()
            b0 = 0
            owners = []
            for i, job in enumerate(self.jobs.values()):
                w = job["w"]
                N, C = w.shape[0], w.shape[-1]
                r = recs[i]
                r.w, r.row_scale = w.data_ptr(), (0 if job["rs"] is None else job["rs"].data_ptr())
                r.w_fwd = 0 if job["fwd"] is None else job["fwd"].data_ptr()
                r.w_dgrad = 0 if job["t"] is None else job["t"].data_ptr()
                r.N, r.taps, r.C, r.block0 = N, w.numel() // (N * C), C, b0
                r.Np, r.Cg, r.Cgp = job["geom"] if job.get("geom") is not None else (0, 0, 0)
                nblk = (w.numel() // (N * C)) * ((N + 31) // 32) * ((C + 31) // 32)
                owners.append(torch.full((nblk,), i, dtype=torch.int32))
                b0 += nblk
            raw = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)
            dev = next(iter(self.jobs.values()))["w"].device
            self._retired.append((self.table, getattr(self, "block_job", None)))      # a captured HIP graph may still launch with the old tables
            self.table = raw.to(dev)
            self.block_job = torch.cat(owners).to(dev)
            self.n_jobs, self.blocks = len(self.jobs), b0
            self.dirty = False

    def _prepare_all(self):
        if self.table is not None:
            _lib().weight_prep_batch(self.table, self.n_jobs, self.blocks, getattr(self, "block_job", None))

    def begin_pass(self):
        if not self.frozen:
            self._build_table()
            self._prepare_all()
        self.active = True
        global _ACTIVE_WEIGHTS
        _ACTIVE_WEIGHTS = self

    def end_pass(self):
        global _ACTIVE_WEIGHTS
        self.active = False
        _ACTIVE_WEIGHTS = None

    def __enter__(self):
        self.begin_pass()
        return self

    def __exit__(self, *exc):
        self.end_pass()
        return False

    def derived(self, w, tag, make):
        """Frozen mode: a weight-shaped tensor the forward derives from parameter w on every call (its zero-padded form), made
        once and kept at one address, so its kernel-side copy is cached like a parameter's; refresh() remakes it in place."""
        key = (w.data_ptr(), tag)
        ent = self._derived.get(key)
        if ent is None:
            t = make().detach().contiguous()
            ent = self._derived[key] = (make, t)
            self.ranges.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
        return ent[1]

    def refresh(self):
        """Frozen mode: the weights changed (load_state_dict, optimizer steps) - ONE batch launch on the current stream rewrites
        every copy made so far, in place."""
        for make, t in self._derived.values():
            t.copy_(make())
        self._build_table()
        self._prepare_all()


class ColsumQueue:
    """Bias gradients of a backward pass, batched: the column sums of up to hip.COLSUM_BATCH layers run as ONE launch
    (gwd_colsum_batch) instead of one 6-25 us launch each.  engine.TrainStep opens the queue around backward and
    flushes it at the end; outside (plain ops calls) every column sum runs at once, as before.  A queued job keeps its
    gradient tensor alive until the flush; the hooks of the DDP bucket plan fire after the sums have been enqueued."""

    def __init__(self):
        self.jobs, self.active = [], False

    def add(self, g, out, rows, C, hook=None):
        lib = _lib()
        if not self.active or rows <= 0 or not lib.colsum_batchable(g, C) or (self.jobs and self.jobs[0][0].dtype != g.dtype):
            if self.jobs and self.active:
                self.flush()                        # keep program order between jobs that may share `out`
            lib.colsum(g, out, rows, C)
            if hook is not None:
                hook()
            return
        self.jobs.append((g, out, rows, C, hook))
        if len(self.jobs) == hip.COLSUM_BATCH:
            self.flush()

    def flush(self):
        if not self.jobs:
            return
        jobs, self.jobs = self.jobs, []
        _lib().colsum_batch([j[:4] for j in jobs])
        for j in jobs:
            if j[4] is not None:
                j[4]()

    def __enter__(self):
        self.active = True
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.flush()
        finally:
            self.jobs, self.active = [], False
        return False


COLSUMS = ColsumQueue()


def _both(first, second):
    """One hook out of two (either may be None): a weight-gradient job that carries the layer's bias gradient fires both."""
    def fire():
        if first is not None:
            first()
        second()
    return fire


class WgradQueue:
    """Weight gradients that accumulate into the flat gradient buffer, handed to the library WGRAD_BATCH at a time
    (gwd_conv_wgrad_batch runs the small plain-GEMM ones of a batch as one grouped launch).  Same life cycle as
    ColsumQueue: open around backward, flushed at its end; a queued job keeps its activation and gradient alive."""
    BATCH = 32

    def __init__(self):
        self.jobs, self.active = [], False
        self._pool, self._used, self._want, self._dev = None, 0, 0, None
        self._retired = []

    def scratch(self, shape, device):
        """Zeroed fp32 scratch for a weight gradient formed in a padded shape.  Inside a backward pass the pieces come from ONE
        buffer zeroed by one fill when the pass opens (sized by the previous pass; a piece that does not fit gets its own zeros)."""
        n = 1
        for v in shape:
            n *= int(v)
        n16 = (n + 15) // 16 * 16
        self._want += n16
        self._dev = device
        if self.active and self._pool is not None and self._pool.device == device and self._used + n16 <= self._pool.numel():
            out = self._pool[self._used:self._used + n].view(shape)
            self._used += n16
            return out
        return torch.zeros(shape, dtype=torch.float32, device=device)

    def add(self, x, dv, dw, dims, kw, hook=None, unpad=None):
        """unpad = (dst, N, taps, G, Cg, Cgp): dw is a zeroed scratch tensor in the PADDED weight shape; after the launch its real
        entries are added to dst (the parameter's slot of the flat gradient buffer) by gwd_unpad_add_batch, then the hook fires."""
        if not self.active:
            _lib().conv_wgrad(x, dv, dw, dims, **kw)
            if unpad is not None:
                _lib().unpad_add_batch([(dw,) + tuple(unpad)])
            if hook is not None:
                hook()
            return
        self.jobs.append((x, dv, dw, dims, kw, hook, unpad))
        if len(self.jobs) == self.BATCH:
            self.flush()

    def flush(self):
        if not self.jobs:
            return
        jobs, self.jobs = self.jobs, []
        _lib().conv_wgrad_batch([j[:5] for j in jobs])
        folds = [(j[2],) + tuple(j[6]) for j in jobs if j[6] is not None]
        if folds:
            _lib().unpad_add_batch(folds)
        for j in jobs:
            if j[5] is not None:
                j[5]()

    def __enter__(self):
        self.active = True
        if self._pool is not None:
            self._pool.zero_()
        self._used = self._want = 0
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.flush()
        finally:
            self.jobs, self.active = [], False
            if self._want and self._dev is not None and (self._pool is None or self._pool.numel() < self._want) \
                    and not torch.cuda.is_current_stream_capturing():
                if self._pool is not None:
                    self._retired.append(self._pool)          # a captured HIP graph may still zero / write the old buffer: never freed
                self._pool = torch.empty(self._want, dtype=torch.float32, device=self._dev)     # for the next pass
        return False


WGRADS = WgradQueue()


_ACTIVE_WEIGHTS = None


def _weight_for(w, row_scale, dtype, shadow=None):
    """Kernel-ready forward weights in the activation dtype (fp32 master -> as is)."""
    if row_scale is None:
        if dtype == torch.float32:
            return w.detach()
        if shadow is not None and shadow.dtype == dtype and not (_ACTIVE_WEIGHTS is not None and _ACTIVE_WEIGHTS.frozen):
            return shadow           # a frozen cache answers itself: its copies change at refresh() only, the shadow at every step
    if dtype == torch.bfloat16 and _ACTIVE_WEIGHTS is not None:
        cached = _ACTIVE_WEIGHTS.get(w, row_scale, "fwd")
        if cached is not None:
            return cached
    out = torch.empty(w.shape, dtype=dtype, device=w.device)
    N, C = w.shape[0], w.shape[-1]
    _lib().weight_prep(w.detach(), row_scale, out, None, N, w.numel() // (N * C), C, hip.F32 if dtype == torch.float32 else hip.BF16)
    return out


def derived_weight(w, tag, make):
    """make(): a weight derived from parameter w inside a forward.  Under a frozen WeightCache (inference) it is made once and
    kept (WeightCache.derived); otherwise it is made now, as before."""
    if _ACTIVE_WEIGHTS is not None and _ACTIVE_WEIGHTS.frozen and w.is_cuda and not torch.is_grad_enabled():
        return _ACTIVE_WEIGHTS.derived(w, tag, make)
    return make()


def _weight_transposed(w, row_scale, dtype):
    """[Cin][taps][Cout] copy for the data gradient."""
    if dtype == torch.bfloat16 and _ACTIVE_WEIGHTS is not None:
        cached = _ACTIVE_WEIGHTS.get(w, row_scale, "t")
        if cached is not None:
            return cached
    N, C = w.shape[0], w.shape[-1]
    taps = w.numel() // (N * C)
    out = torch.empty((C,) + tuple(w.shape[1:-1]) + (N,), dtype=dtype, device=w.device)
    _lib().weight_prep(w.detach(), row_scale, None, out, N, taps, C, hip.F32 if dtype == torch.float32 else hip.BF16)
    return out


_DIM_T = {}


def _upsampled_dgrad_weight(w, dtype):
    """Data gradient of `3x3 conv over a 2x nearest-upsampled map` onto the LOW-resolution input, as ONE 4x4 / stride 2 / pad 1
    convolution of the output gradient: summing the 2 x 2 children of a low-res pixel commutes into the taps,
        gx[y', x'] = sum_{t, s = 0..3} gy[2 y' - 1 + t, 2 x' - 1 + s] . Wk[t][s],   Wk[t][s] = sum_{kh in G(t), kw in G(s)} W[kh][kw],
        G(0) = {2}, G(1) = {1, 2}, G(2) = {0, 1}, G(3) = {0}
    - 16 taps per low-res pixel = 4 per high-res one instead of 9, and no high-resolution gradient map in memory (the transposed
    gather wrote it, 314 MB for the last decoder stage, and the footprint sum read it back).  w (Cout, 3, 3, Cin) fp32 master ->
    (Cin, 4, 4, Cout) in `dtype`: the weight operand of gwd_conv_forward with x = gy."""
    Cout, _, _, Cin = w.shape
    wk = torch.empty((Cin, 4, 4, Cout), dtype=dtype, device=w.device)
    _lib().upsample_taps_collapse(w.detach().float().contiguous(), wk)       # one launch (was ~8 element-wise ones; an einsum would be a library GEMM)
    return wk




def mask_levels(pad_mask, sizes):
    """Padding masks of the feature levels (F.interpolate(mask[None].float(), size).to(bool), backbone.py:81-88) with the cumulative
    counts of their un-masked pixels attached (`_gwd_counts`, what pos_sine needs): one launch per level."""
    lib = _lib()
    B = pad_mask.shape[0]
    full = pad_mask.contiguous().view(torch.uint8) if pad_mask.dtype == torch.bool else pad_mask.contiguous()
    out = []
    for h, w in sizes:
        lvl = torch.empty((B, h, w), dtype=torch.uint8, device=pad_mask.device)
        counts = torch.empty((B, h, w, 2), dtype=torch.int16, device=pad_mask.device)
        lib.pos_counts(full, lvl, counts)
        m = lvl.view(torch.bool)
        m._gwd_counts = counts
        out.append(m)
    return out


def pos_sine(mask, num_pos_feats, normalize, temperature=10000.0):
    """PositionEmbeddingSine (position_encoding.py:28-48) of a level mask from mask_levels(): (B,h,w,2F) fp32, one launch."""
    counts = mask._gwd_counts
    key = (num_pos_feats, float(temperature), str(mask.device))
    dim_t = _DIM_T.get(key)
    if dim_t is None:
        t = torch.arange(num_pos_feats, dtype=torch.float32, device=mask.device)
        dim_t = _DIM_T[key] = temperature ** (2 * torch.div(t, 2, rounding_mode="floor") / num_pos_feats)
    B, h, w, _ = counts.shape
    out = torch.empty((B, h, w, 2 * num_pos_feats), dtype=torch.float32, device=mask.device)
    _lib().pos_emit(counts, dim_t, out, normalize)
    return out


_STEM_PACKED = {}
_STEM_RETIRED = []


def stem(x, w, scale, shift):
    """ResNet stem (conv 7x7 s2 p3, 3 -> 64, folded FrozenBN, ReLU, max-pool 3x3 s2 p1) as ONE forward-only kernel
    (gwd_stem_forward); x bf16 (B,H,W,3) -> (B,Hp,Wp,64).  The stem is frozen on this path (backbone.py:62-64): no gradient.
    The operand-order copy of the weights is rebuilt when the weight or the scale changes (load_state_dict)."""
    lib = _lib()
    key = (w.data_ptr(), w._version, scale.data_ptr(), scale._version, str(w.device))
    ent = _STEM_PACKED.get(w.data_ptr())
    if ent is None or ent[0] != key:
        packed = torch.empty(hip.STEM_PACKED_ELEMS, dtype=torch.bfloat16, device=w.device)
        lib.stem_pack(w.detach(), scale.detach().float().contiguous(), packed)
        if ent is not None:
            _STEM_RETIRED.append(ent[1])                      # a captured graph may still read the previous copy
        ent = _STEM_PACKED[w.data_ptr()] = (key, packed)
    B, H, W, _ = x.shape
    y = torch.empty((B, hip.stem_out(H), hip.stem_out(W), 64), dtype=x.dtype, device=x.device)
    lib.stem_forward(x.detach().contiguous(), ent[1], shift.detach().float().contiguous(), y)
    return y


def padded_weight(w, geom, kind, dtype):
    """Zero-padded kernel-side copy of w (N, KH, KW, C), geom = (Np, Cg, Cgp): rows N -> Np and each of the G = C / Cg groups of
    input channels Cg -> Cgp.  kind 'fwd': (Np, KH, KW, G*Cgp); 't' (data gradient): (G*Cgp, KH, KW, Np)."""
    Np, Cg, Cgp = geom
    N, KH, KW, C = w.shape
    G = C // Cg
    if G * Cg != C or Np < N or Cgp < Cg:
        raise ValueError("padded_weight: geometry %r does not fit a weight of shape %r" % (geom, tuple(w.shape)))
    src = w.view(N, KH * KW, G, Cg)
    if kind == "fwd":
        out = torch.zeros((Np, KH, KW, G * Cgp), dtype=dtype, device=w.device)
        out.view(Np, KH * KW, G, Cgp)[:N, :, :, :Cg] = src
    else:
        out = torch.zeros((G * Cgp, KH, KW, Np), dtype=dtype, device=w.device)
        out.view(G, Cgp, KH * KW, Np)[:, :Cg, :, :N] = src.permute(2, 3, 1, 0)
    return out


def _padded_weight_for(w, geom, kind, dtype):
    if dtype == torch.bfloat16 and _ACTIVE_WEIGHTS is not None:
        cached = _ACTIVE_WEIGHTS.get(w, None, kind, geom)
        if cached is not None:
            return cached
    return padded_weight(w.detach(), geom, kind, dtype)


def _fan_in(ctx, g_fan):
    """The second gradient of a fan-out node (the one of its `x again` output, see _ConvFn.forward), contiguous; None where the node
    has no such output or nothing arrived for it."""
    return g_fan[0].contiguous() if (ctx.fan and g_fan and g_fan[0] is not None) else None


def _dgrad_dims(dims):
    """dims of a convolution -> dims of its data gradient: the same problem with the input and the output side swapped."""
    B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW = dims
    return (B, Ho, Wo, Cout, Hi, Wi, Cin, KH, KW)


def _dgrad_stride1(dv, wt, x, dims, pad, g_in=None):
    """Data gradient of a stride-1 convolution of x (dims): the transposed gather of dv over the [Cin][taps][Cout] weights wt; g_in, the
    input's second gradient (fan-out), joins in the kernel epilogue."""
    gx = torch.empty_like(x)
    _lib().conv_forward(dv, wt, gx, _dgrad_dims(dims), stride=1, pad=pad, gather=GATHER_TRANSPOSED, residual=g_in)
    return gx


def _conv_wgrad(x, dv, w, dims, kw, sink, geom=None):
    """Weight gradient of a convolution (kw: its descriptor keywords).  With a sink the kernel ACCUMULATES (fp32 atomics) straight into
    the flat gradient buffer, no temporary: the job joins WGRADS, sink[1] fires once it has been issued, and autograd gets None; without
    one the gradient is formed in fresh zeros and returned.  geom = (Np, Cg, Cgp) (_PadConvFn): the gradient is formed in the padded
    shape, in zeroed scratch, and its real entries are added to the parameter's own shape by gwd_unpad_add_batch."""
    lib = _lib()
    if geom is None:
        if sink is not None:
            WGRADS.add(x, dv, sink[0], dims, kw, sink[1])
            return None
        gw = torch.zeros(w.shape, dtype=torch.float32, device=w.device)
        lib.conv_wgrad(x, dv, gw, dims, **kw)
        return gw
    Np, Cg, Cgp = geom
    N, KH, KW, C = w.shape
    tmp = WGRADS.scratch((Np, KH, KW, dims[3]), x.device)
    fold = (N, KH * KW, C // Cg, Cg, Cgp)
    if sink is not None:
        WGRADS.add(x, dv, tmp, dims, kw, sink[1], unpad=(sink[0].view(-1),) + fold)
        return None
    lib.conv_wgrad(x, dv, tmp, dims, **kw)
    gw = torch.zeros(w.shape, dtype=torch.float32, device=w.device)
    lib.unpad_add_batch([(tmp, gw.view(-1)) + fold])
    return gw


def _conv_backward_stride1(need_gx, need_gw, x, w, dv, g_in, dims, pad, geom, sink):
    """Backward of a stride-1 convolution without bias or activation (_PadConvFn, the convolution inside _ConvLnFn) -> (gx, gw)."""
    gx = gw = None
    if need_gx:
        wt = _weight_transposed(w, None, x.dtype) if geom is None else _padded_weight_for(w, geom, "t", x.dtype)
        gx = _dgrad_stride1(dv, wt, x, dims, pad, g_in)
    elif g_in is not None:
        gx = g_in
    if need_gw:
        gw = _conv_wgrad(x, dv, w, dims, dict(stride=1, pad=pad), sink, geom)
    return gx, gw


class _PadConvFn(torch.autograd.Function):
    """Stride-1 convolution (no bias, no activation) of a layer whose channel counts are not multiples of the MFMA / LDS-DMA
    granule, run on ZERO-PADDED channel counts: x (B, H, W, G*Cgp) holds G groups of Cg real channels each padded to Cgp with zeros,
    the result (B, Ho, Wo, Np) has its Cout real channels followed by zeros.  The kernels see an ordinary (G*Cgp -> Np) layer (the
    padding lives in the kernel-side weight copies: WeightCache / gwd_weight_prep_batch write the real entries into zeroed
    copies), the parameter and its gradient keep their own shape: the weight gradient is formed in the padded shape and folded
    back by gwd_unpad_add_batch.  User: the 30 / 60 / 300-channel pyramid of points_sample.py:45-125 (32 / 64 / 320 here)."""

    @staticmethod
    def forward(ctx, x, w, pad, geom, sink, fanout=False):
        lib = _lib()
        ctx.fan = bool(fanout)
        Np, Cg, Cgp = geom
        B, Hi, Wi, Cin = x.shape
        N, KH, KW, C = w.shape
        G = C // Cg
        if Cin != G * Cgp:
            raise ValueError("conv2d_padded: input has %d channels, the padded weight expects %d" % (Cin, G * Cgp))
        Ho, Wo = Hi + 2 * pad - KH + 1, Wi + 2 * pad - KW + 1
        x = x.contiguous()
        y = torch.empty((B, Ho, Wo, Np), dtype=x.dtype, device=x.device)
        dims = (B, Hi, Wi, Cin, Ho, Wo, Np, KH, KW)
        lib.conv_forward(x, _padded_weight_for(w, geom, "fwd", x.dtype), y, dims, stride=1, pad=pad)
        ctx.save_for_backward(x, w)
        ctx.cfg = (dims, pad, geom, sink)
        if fanout:
            return y, x.view_as(x)                   # as _ConvFn: the input again, for its second consumer
        return y

    @staticmethod
    def backward(ctx, gy, *g_fan):
        g_in = _fan_in(ctx, g_fan)
        x, w = ctx.saved_tensors
        dims, pad, geom, sink = ctx.cfg
        gx, gw = _conv_backward_stride1(ctx.needs_input_grad[0], ctx.needs_input_grad[1], x, w, gy.contiguous(), g_in, dims, pad, geom, sink)
        return gx, gw, None, None, None, None


def conv2d_padded(x, w, pad, geom, fanout=False):
    """See _PadConvFn.  x (B, H, W, G*Cgp) zero-padded, w (Cout, KH, KW, G*Cg) fp32 master, geom = (Np, Cg, Cgp)."""
    return _PadConvFn.apply(x, w, int(pad), tuple(int(v) for v in geom), _sink(w), bool(fanout))


class _ConvFn(torch.autograd.Function):
    """y = act_scale * act(conv(x, w * row_scale) + shift + residual), all in one kernel launch; with `mult` (an element-wise
    dropout multiplier) y = act_scale * act(conv + shift) * mult + residual: the skip is added after the dropout."""

    @staticmethod
    def forward(ctx, x, w, bias, residual, row_scale, shift_const, stride, pad, act, act_scale, virt, shadow, sinks, mult=None, fanout=False,
                in_gate=ACT_NONE, defer=False, gate_src=None):
        lib = _lib()
        ctx.fan = bool(fanout)
        # in_gate / defer: the activation backward of a ReLU / ELU layer moves into the data-gradient epilogue of its ONLY consumer
        # (gwd_conv_desc.gate = the consumer's saved input): the producer (defer) passes the incoming gradient on unchanged, the
        # consumer (in_gate = the producer's activation) returns the gradient w.r.t. the producer's PRE-activation value
        # GELU (the MLPs): its derivative needs the producer's PRE-activation value, so the producer (defer) returns it as a second
        # output and the consumer gets it as gate_src (in_gate = ACT_GELU); ReLU / ELU gates are rebuilt from the consumer's own input
        ctx.in_gate, ctx.defer = int(in_gate), bool(defer)
        if defer and (act not in (ACT_RELU, ACT_ELU, ACT_GELU) or act_scale != 1.0 or mult is not None or (act == ACT_GELU and fanout)):
            raise ValueError("conv2d: defer needs ReLU / ELU / GELU with act_scale 1 and no dropout multiplier")
        if in_gate not in (ACT_NONE, ACT_RELU, ACT_ELU, ACT_GELU) or (in_gate == ACT_GELU) != (gate_src is not None):
            raise ValueError("conv2d: in_gate is ReLU or ELU, or GELU with the producer's pre-activation tensor as gate_src")
        B, Hi, Wi, Cin = x.shape
        Cout, KH, KW, Cw = w.shape
        if Cw != Cin:
            raise ValueError("conv2d: weight expects %d input channels, input has %d" % (Cw, Cin))
        if virt is None:
            Ho = (Hi + 2 * pad - KH) // stride + 1
            Wo = (Wi + 2 * pad - KW) // stride + 1
            gather, vv = GATHER_CONV, (0, 0)
        else:
            Ho, Wo = virt[0] + 2 * pad - KH + 1, virt[1] + 2 * pad - KW + 1
            gather, vv = GATHER_UPSAMPLED, tuple(virt)
        x = x.contiguous()
        wk = _weight_for(w, row_scale, x.dtype, shadow)
        shift = shift_const if bias is None else (bias.detach().float() if shift_const is None else shift_const + bias.detach().float())
        y = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
        need_grad = any(ctx.needs_input_grad[:4])
        z = torch.empty_like(y) if (act == ACT_GELU and need_grad) else None
        if residual is not None:
            residual = residual.contiguous()
        dims = (B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW)
        if mult is not None:
            mult = mult.contiguous()
        lib.conv_forward(x, wk, y, dims, z=z, shift=shift, residual=residual, stride=stride, pad=pad, gather=gather,
                         virt=vv, act=act, act_scale=act_scale, mult=mult)
        ctx.cfg = (dims, stride, pad, act, act_scale, gather, vv, bias is not None, residual is not None)
        ctx.sinks = sinks
        if mult is not None and (act not in (ACT_NONE, ACT_RELU) or (act == ACT_RELU and residual is not None)):
            raise ValueError("conv2d: a dropout multiplier is supported behind no activation (+ skip) or behind ReLU (no skip) only")
        # ReLU's backward needs only the sign of the output: y * mult has the sign of relu(v) wherever mult > 0, and where
        # mult == 0 the incoming gradient is multiplied by zero anyway
        ctx.save_for_backward(x, w, row_scale, z if act == ACT_GELU else (y if act != ACT_NONE else None), mult, gate_src)
        if defer and act == ACT_GELU:
            if z is None:                               # no gradient wanted anywhere: nobody will read it
                z = y
            ctx.mark_non_differentiable(z)
            ctx.set_materialize_grads(False)            # or every backward starts with a zero fill the size of z for "its" gradient
            return y, z
        if fanout:
            # second output: x again, for a second consumer of the layer's input (a skip connection).  With it this node is x's only
            # consumer, both gradients arrive in ONE backward call and the skip's joins the data gradient in the kernel epilogue -
            # no accumulation pass over the map (PyrBlock, Bottleneck)
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, gy, *g_fan):
        if gy is None:                                 # (only where materialize_grads is off: a GELU producer nobody consumed)
            return (None,) * 18
        g_in = _fan_in(ctx, g_fan)
        x, w, row_scale, ref, mult, gate_src = ctx.saved_tensors
        dims, stride, pad, act, act_scale, gather, vv, has_bias, has_res = ctx.cfg
        gy = gy.contiguous()
        w_sink, b_sink = ctx.sinks if ctx.sinks is not None else (None, None)
        want_b = has_bias and ctx.needs_input_grad[2]
        dv, bias_done = _conv_act_backward(gy, ref, mult, act, act_scale, ctx.defer, b_sink if want_b else None, dims)
        gx = g_in
        if ctx.needs_input_grad[0]:
            gx = _conv_dgrad(x, w, row_scale, dv, g_in, dims, stride, pad, gather, vv, ctx.in_gate, gate_src)
        gw, gb = _conv_param_grads(x, w, row_scale, dv, dims, stride, pad, gather, vv, ctx.needs_input_grad[1], want_b and not bias_done,
                                   w_sink, b_sink)
        # the post-dropout skip connection gets the incoming gradient as is
        gres = (gy if mult is not None else dv) if (has_res and ctx.needs_input_grad[3]) else None
        return gx, gw, gb, gres, None, None, None, None, None, None, None, None, None, None, None, None, None, None


def _conv_act_backward(gy, ref, mult, act, act_scale, defer, b_sink, dims):
    """First step of _ConvFn.backward: dropout multiplier, activation backward and, where it comes for free, the bias gradient.
    b_sink: the bias' sink where the layer has a bias whose gradient is wanted in one, else None.  -> (dv, the gradient w.r.t. the
    convolution's own output; whether the bias gradient has been summed into b_sink here)."""
    lib = _lib()
    rows, Cout = dims[0] * dims[4] * dims[5], dims[6]

    def with_colsum(g, dv, m):
        # [dropout multiplier,] activation backward and the bias gradient (column sums of dv) in ONE pass, straight into the flat
        # gradient; False: no kernel for the shape, nothing was launched
        done = lib.act_backward_colsum(g, ref, dv, b_sink[0], rows, Cout, act, act_scale, mult=m)
        if done and b_sink[1] is not None:
            b_sink[1]()
        return done

    if defer:
        return gy, False                               # the consumer's data-gradient epilogue has applied act'(.) already
    if mult is not None:
        if b_sink is not None:
            dv = torch.empty_like(gy)
            if with_colsum(gy, dv, mult):              # (was: an ATen multiply, then the rest)
                return dv, True
        gy = gy * mult
    if act == ACT_NONE and act_scale == 1.0:
        return gy, False
    dv = torch.empty_like(gy)
    bias_done = b_sink is not None and with_colsum(gy, dv, None)
    if not bias_done:
        lib.act_backward(gy, ref, dv, None, rows, Cout, act, act_scale)
    return dv, bias_done


def _conv_dgrad(x, w, row_scale, dv, g_in, dims, stride, pad, gather, vv, in_gate, gate_src):
    """Second step of _ConvFn.backward: the gradient w.r.t. the input x, with g_in (the input's second gradient, fan-out) added and
    the backward of the producer's activation applied where the layer is that producer's gated consumer (in_gate)."""
    lib = _lib()
    B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW = dims
    wt = _weight_transposed(w, row_scale, x.dtype)
    gate = dict(gate=(x if gate_src is None else gate_src), gate_act=in_gate) if in_gate != ACT_NONE else {}
    if (gather == GATHER_UPSAMPLED and x.is_cuda and x.dtype == torch.bfloat16 and KH == 3 and KW == 3
            and pad == 1 and vv == (2 * Hi, 2 * Wi) and row_scale is None and (g_in is None or not gate)):
        # one strided convolution of the gradient with the 4x4 collapse of the weights (see _upsampled_dgrad_weight)
        gx = torch.empty_like(x)
        lib.conv_forward(dv, _upsampled_dgrad_weight(w, x.dtype), gx, (B, Ho, Wo, Cout, Hi, Wi, Cin, 4, 4), stride=2, pad=1,
                         residual=g_in, **gate)
        return gx
    if gather == GATHER_UPSAMPLED:
        gxv = torch.empty((B, vv[0], vv[1], Cin), dtype=x.dtype, device=x.device)
        lib.conv_forward(dv, wt, gxv, (B, Ho, Wo, Cout, vv[0], vv[1], Cin, KH, KW), stride=1, pad=pad, gather=GATHER_TRANSPOSED)
        if gate and g_in is None:                      # the gate rides on the footprint sum
            return _nearest_upsample_backward(gxv, Hi, Wi, gate=x, gate_act=in_gate)
        gx = _nearest_upsample_backward(gxv, Hi, Wi)
        if g_in is not None:
            gx = gx + g_in
        if gate:                                       # behind the skip gradient: a pass of its own
            gated = torch.empty_like(gx)
            lib.act_backward(gx, x, gated, None, B * Hi * Wi, Cin, in_gate, 1.0)
            gx = gated
        return gx
    gx = torch.empty_like(x)
    if KH == 1 and KW == 1 and stride > 1 and pad == 0 and not gate:
        # 1x1 / stride s: only the pixels (s i, s j) get a gradient - a plain GEMM over the OUTPUT pixels, then placement
        # (+ the skip gradient) in one pass; the transposed gather spent 3/4 of its work on zero-page products
        q = torch.empty((B, Ho, Wo, Cin), dtype=x.dtype, device=x.device)
        lib.conv_forward(dv, wt, q, (B, Ho, Wo, Cout, Ho, Wo, Cin, 1, 1), stride=1, pad=0, gather=GATHER_TRANSPOSED)
        if lib.stride_place(q, g_in, gx, stride):
            return gx
    if lib.conv_forward(dv, wt, gx, _dgrad_dims(dims), stride=stride, pad=pad, gather=GATHER_TRANSPOSED, residual=g_in, **gate) is False:
        # no kernel with the GELU gate for this shape: the data gradient, then the gate as a pass of its own
        lib.conv_forward(dv, wt, gx, _dgrad_dims(dims), stride=stride, pad=pad, gather=GATHER_TRANSPOSED, residual=g_in)
        gated = torch.empty_like(gx)
        lib.act_backward(gx, gate["gate"], gated, None, B * Hi * Wi, Cin, in_gate, 1.0)
        gx = gated
    return gx


def _conv_param_grads(x, w, row_scale, dv, dims, stride, pad, gather, vv, want_w, want_b, w_sink, b_sink):
    """Third step of _ConvFn.backward: weight and bias gradient -> (gw, gb) as autograd gets them (None for what went into a sink).
    want_b: the layer has a bias whose gradient is wanted and the activation pass has not summed it.  This is the one place that decides
    who sums it then: the weight-gradient kernel, or a column-sum pass."""
    lib = _lib()
    B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW = dims
    gw = gb = None
    if want_w:
        # row_scale (folded FrozenBN: the layer ran with w * scale) multiplies the gradient inside the kernel's epilogue
        if (w_sink is not None and gather == GATHER_UPSAMPLED and x.is_cuda and x.dtype == torch.bfloat16
                and KH == 3 and KW == 3 and pad == 1 and vv == (2 * Hi, 2 * Wi) and row_scale is None):
            # the weight gradient through the same 4x4 / stride 2 form: D[ci][t][s][co] = sum_{y', x'} x[y', x', ci] gy[2 y' - 1 + t, 2 x' - 1 + s, co]
            # is the ordinary weight gradient of that strided convolution (operands swapped: its input is gy, its output side x) - 16 taps per
            # low-res pixel instead of 36, on the grouped GEMM kernels - and dW[co][kh][kw][ci] = sum_{t in T(kh), s in T(kw)} D[ci][t][s][co],
            # T(0) = {2, 3}, T(1) = {1, 2}, T(2) = {0, 1}, added to the flat gradient when the batch has been issued
            D = WGRADS.scratch((Cin, 4, 4, Cout), x.device)

            def fold(D=D, sink=w_sink, shape=(Cout, KH, KW, Cin)):
                lib.upsample_taps_fold(D, sink[0].view(shape))
                if sink[1] is not None:
                    sink[1]()

            WGRADS.add(dv, x, D, (B, Ho, Wo, Cout, Hi, Wi, Cin, 4, 4), dict(stride=2, pad=1), fold)
        else:
            kw, sink = dict(stride=stride, pad=pad, gather=gather, virt=vv, scale=row_scale), w_sink
            if (w_sink is not None and want_b and b_sink is not None and x.is_cuda
                    and lib.conv_wgrad_takes_bias(x, dv, dims, WGRADS.active, **kw)):
                # the weight-gradient kernel stages every element of dv anyway: it sums the bias gradient from its dY tiles, and the
                # column-sum pass over the same map below is not run; both hooks fire once the job has been issued
                kw["dbias"], want_b = b_sink[0], False
                if b_sink[1] is not None:
                    sink = (w_sink[0], _both(w_sink[1], b_sink[1]))
            gw = _conv_wgrad(x, dv, w, dims, kw, sink)
    if want_b:
        rows = B * Ho * Wo
        if b_sink is not None:
            COLSUMS.add(dv, b_sink[0], rows, Cout, b_sink[1])
        else:
            gb = torch.zeros(Cout, dtype=torch.float32, device=dv.device)
            lib.colsum(dv, gb, rows, Cout)
    return gw, gb


def _nearest_upsample_backward(gv, Hi, Wi, gate=None, gate_act=ACT_NONE):
    """Sum the gradient of a nearest-upsampled view back onto its source pixels: one gather pass of gwd_resample_backward
    (each source pixel sums its own footprint; was a strided aten::sum at 1.5 TB/s).  gate: the source map when it is the output of
    an activation whose backward is applied to the sums in the same pass (conv2d defer / in_gate)."""
    B, Hv, Wv, C = gv.shape
    gx = torch.empty((B, Hi, Wi, C), dtype=gv.dtype, device=gv.device)
    lib = _lib()
    done = lib.resample_backward(gv.contiguous(), gx, B, Hi, Wi, Hv, Wv, C, hip.RESAMPLE_NEAREST, gate=gate, gate_act=gate_act)
    if gate is not None and done is False:
        gated = torch.empty_like(gx)
        lib.act_backward(gx, gate, gated, None, B * Hi * Wi, C, gate_act, 1.0)
        gx = gated
    return gx


def _sink(p, shape=None):
    """(flat-gradient view, hook) of a parameter managed by engine.TrainStep, else None."""
    g = getattr(p, "_gwd_grad", None)
    if g is None:
        return None
    return (g if shape is None else g.view(shape), getattr(p, "_gwd_hook", None))


def conv2d(x, w, bias=None, *, stride=1, pad=0, act=ACT_NONE, act_scale=1.0, residual=None, row_scale=None,
           shift=None, upsample_to=None, mult=None, fanout=False, in_gate=ACT_NONE, defer=False):
    """x (B,H,W,Cin); w (Cout,KH,KW,Cin) fp32 master; bias fp32 parameter or None.
    row_scale / shift: constant per-Cout tensors of a folded FrozenBatchNorm.
    upsample_to=(Hv,Wv): convolve a nearest-upsampled view of x without materialising it.
    fanout: return (y, x'), x' = x for the OTHER consumer of the input (use x' instead of x there): see _ConvFn.forward.
    defer / in_gate: a ReLU / ELU layer whose output has exactly ONE consumer (this function again, or the fan-out chain that starts
    with it) is called with defer=True and that consumer with in_gate=<the producer's activation>: the activation's backward then
    runs in the consumer's data-gradient epilogue instead of as a pass of its own (both or neither)."""
    sinks = (_sink(w), _sink(bias) if bias is not None else None)
    return _ConvFn.apply(x, w, bias, residual, row_scale, shift, stride, pad, act, float(act_scale), upsample_to,
                         getattr(w, "_gwd_bf16", None), sinks if (sinks[0] or sinks[1]) else None, mult, bool(fanout), in_gate, defer)


def linear(x, w, bias=None, act=ACT_NONE, rows=None, residual=None, mult=None, fanout=False, defer=False, in_gate=ACT_NONE, gate_src=None):
    """x (..., K) @ w(N, K)^T + bias, optional fused activation; same kernel as conv2d (1x1, one pixel per row).
    rows=(r0, r1): use only that row range of a packed parameter (the q/k/v blocks of an attention in-projection);
    the gradient then goes straight into that slice of the parameter's flat gradient instead of through a
    zero-filled full-size SliceBackward temporary."""
    K = x.shape[-1]
    lead = x.shape[:-1]
    x2 = x.reshape(-1, 1, 1, K)
    shadow = getattr(w, "_gwd_bf16", None)
    ws, bs = _sink(w), (_sink(bias) if bias is not None else None)
    if rows is not None:
        r0, r1 = rows
        if ws is not None:
            ws = (ws[0][r0:r1], ws[1])
        if bs is not None:
            bs = (bs[0][r0:r1], bs[1])
        shadow = None if shadow is None else shadow[r0:r1]
        w = w[r0:r1]
        bias = None if bias is None else bias[r0:r1]
    n = w.shape[0]
    sinks = (None if ws is None else (ws[0].view(n, 1, 1, K), ws[1]), bs)
    res = None if residual is None else residual.reshape(-1, 1, 1, n)
    mul = None if mult is None else mult.reshape(-1, 1, 1, n)
    fan = bool(fanout)
    # defer (act = GELU): the activation's backward runs in the data-gradient epilogue of the layer's ONLY consumer; returns (y, z), z the
    # pre-activation tensor that consumer takes as gate_src (with in_gate = ACT_GELU) - the fc1 / fc2 pair of an MLP (layers.Mlp)
    gs = None if gate_src is None else gate_src.reshape(-1, 1, 1, K)
    y = _ConvFn.apply(x2, w.view(n, 1, 1, K), bias, res, None, None, 1, 0, act, 1.0, None,
                      None if shadow is None else shadow.view(n, 1, 1, K),
                      sinks if (sinks[0] or sinks[1]) else None, mul, fan, int(in_gate), bool(defer), gs)
    if defer and act == ACT_GELU:
        return y[0].view(*lead, n), y[1].view(*lead, n)
    if fanout:                              # (y, x again for the input's second consumer): see _ConvFn.forward
        return (y[0].view(*lead, n), y[1].view(x.shape)) if fan else (y.view(*lead, n), x)
    return y.view(*lead, n)


def _ln_backward(gy, x, g, b, mean, rstd, gelu, sinks, g_in=None, in_gate=ACT_NONE):
    """Backward of y = [GELU](LayerNorm(x)) over the first C = len(g) channels of rows of pitch x.shape[-1] (more channels than affine
    entries: the rest is zero padding, _PadConvFn): gwd_layernorm_backward, with d gamma / d beta into their sinks (sinks =
    ((dgamma, hook), (dbeta, hook))) or into fresh zeros.  g_in: a second gradient of x (fan-out), added in the kernel; in_gate = ACT_ELU:
    x is an ELU output whose backward is applied as well.  -> (gx, what autograd gets for gamma, for beta)."""
    lib = _lib()
    ld = x.shape[-1]
    C = g.shape[0] if g is not None else ld
    rows = x.numel() // ld
    gx = torch.empty_like(x)
    dg = db = None
    if sinks is not None:
        (dg, h1), (db, h2) = sinks
    elif g is not None:
        dg = torch.zeros(C, dtype=torch.float32, device=x.device)
        db = torch.zeros(C, dtype=torch.float32, device=x.device)
    fused = lib.layernorm_backward(gy, x, g, b, mean, rstd, gx, dg, db, rows, C, gelu, ld=0 if ld == C else ld, gskip=g_in,
                                   elu_input=in_gate == ACT_ELU)
    if fused is False:                                 # no vector kernel for this width: the skip gradient / the gate as passes
        if g_in is not None:
            gx = gx + g_in
        if in_gate != ACT_NONE:
            gated = torch.empty_like(gx)
            lib.act_backward(gx, x, gated, None, rows, ld, in_gate, 1.0)
            gx = gated
    if sinks is None:
        return gx, dg, db
    for h in (h1, h2):
        if h is not None:
            h()
    return gx, None, None


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, gelu, sinks, residual, fanout=False, in_gate=ACT_NONE):
        lib = _lib()
        ctx.sinks = sinks
        ctx.fan = bool(fanout)
        if in_gate not in (ACT_NONE, ACT_ELU):
            raise ValueError("layer_norm: in_gate is ELU (the gate is rebuilt from the normalised value: continuous derivatives only)")
        ctx.in_gate = int(in_gate)                  # x is the output of a conv2d(..., act=ELU, defer=True): its backward runs in ours
        ctx.has_res = residual is not None
        x = x.contiguous()
        ld = x.shape[-1]
        C = gamma.shape[0] if gamma is not None else ld       # fewer affine entries than channels: the rest is zero padding (_PadConvFn)
        rows = x.numel() // ld
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        g = gamma.detach() if gamma is not None else None
        b = beta.detach() if beta is not None else None
        lib.layernorm_forward(x, g, b, y, mean, rstd, rows, C, gelu, residual=None if residual is None else residual.contiguous(),
                              ld=0 if ld == C else ld)
        ctx.save_for_backward(x, g, b, mean, rstd)
        ctx.gelu = gelu
        if fanout:
            return y, x.view_as(x)        # x again for its second consumer (the block's skip): see _ConvFn.forward
        return y

    @staticmethod
    def backward(ctx, gy, *g_fan):
        g_in = _fan_in(ctx, g_fan)
        x, g, b, mean, rstd = ctx.saved_tensors
        gy = gy.contiguous()
        gx, dg, db = _ln_backward(gy, x, g, b, mean, rstd, ctx.gelu, ctx.sinks, g_in, ctx.in_gate)
        gres = gy if ctx.has_res else None                # y = LN(x) + residual: the skip gets the incoming gradient as is
        return gx, dg, db, None, None, gres, None, None


def layer_norm(x, gamma, beta, gelu=False, residual=None, fanout=False, in_gate=ACT_NONE):
    """LayerNorm over the last dim (eps 1e-5) with optional fused exact GELU; residual (same shape) is added afterwards.
    fanout: return (y, x') with x' = x for the OTHER consumer of the input (the skip of a pre-norm block): x's two gradients then
    meet inside the LayerNorm backward kernel instead of an accumulation pass."""
    sinks = None
    if gamma is not None:
        sg, sb = _sink(gamma), _sink(beta)
        sinks = (sg, sb) if (sg is not None and sb is not None) else None
    return _LayerNormFn.apply(x, gamma, beta, bool(gelu), sinks, residual, bool(fanout), in_gate)


class _ConvLnFn(torch.autograd.Function):
    """ConvLn (points_sample.py:12-25): stride-1 convolution without bias -> LayerNorm over channels [-> GELU] [+ residual] as ONE
    forward launch - the LayerNorm runs in the implicit GEMM's epilogue on the fp32 accumulators (gwd_conv_desc.ln_*), so the
    normalisation pass and its read of the convolution's output disappear.  The kernel leaves what the unfused pair left: the
    convolution's output z and the row statistics, so the backward is the unfused one (gwd_layernorm_backward, then data / weight
    gradient of the convolution).  geom = None, or (Np, Cg, Cgp) for a layer on zero-padded channel counts (_PadConvFn).  Where the
    library has no fused kernel for the shape the two forward kernels run here instead - same results, same saved tensors."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, residual, pad, gelu, geom, w_sink, ln_sinks, fanout):
        lib = _lib()
        ctx.fan = bool(fanout)
        B, Hi, Wi, Cin = x.shape
        N, KH, KW, Cw = w.shape
        if geom is None:
            Np = N
            if Cw != Cin:
                raise ValueError("conv_ln: weight expects %d input channels, input has %d" % (Cw, Cin))
            wk = _weight_for(w, None, x.dtype, getattr(w, "_gwd_bf16", None))
        else:
            Np, Cg, Cgp = geom
            if Cin != (Cw // Cg) * Cgp:
                raise ValueError("conv_ln: input has %d channels, the padded weight expects %d" % (Cin, (Cw // Cg) * Cgp))
            wk = _padded_weight_for(w, geom, "fwd", x.dtype)
        Ho, Wo = Hi + 2 * pad - KH + 1, Wi + 2 * pad - KW + 1
        x = x.contiguous()
        rows = B * Ho * Wo
        y = torch.empty((B, Ho, Wo, Np), dtype=x.dtype, device=x.device)
        need_grad = any(ctx.needs_input_grad)
        z = torch.empty_like(y) if need_grad else None      # inference: the convolution's own output is never written
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        g, b = gamma.detach(), beta.detach()
        res = None if residual is None else residual.contiguous()
        dims = (B, Hi, Wi, Cin, Ho, Wo, Np, KH, KW)
        fused = lib.conv_forward(x, wk, y, dims, z=z, scale=g, shift=b, residual=res, stride=1, pad=pad,
                                 act=ACT_GELU if gelu else ACT_NONE, ln=(mean, rstd, N))
        if fused is False:
            z = torch.empty_like(y) if z is None else z
            lib.conv_forward(x, wk, z, dims, stride=1, pad=pad)
            lib.layernorm_forward(z, g, b, y, mean, rstd, rows, N, gelu, residual=res, ld=0 if Np == N else Np)
        if need_grad:
            ctx.save_for_backward(x, w, z, g, b, mean, rstd)
        ctx.cfg = (dims, pad, bool(gelu), geom, w_sink, ln_sinks, residual is not None)
        if fanout:
            return y, x.view_as(x)                   # the input again, for its second consumer (the block's skip): see _ConvFn
        return y

    @staticmethod
    def backward(ctx, gy, *g_fan):
        g_in = _fan_in(ctx, g_fan)
        x, w, z, g, b, mean, rstd = ctx.saved_tensors
        dims, pad, gelu, geom, w_sink, ln_sinks, has_res = ctx.cfg
        gy = gy.contiguous()
        # the gradient w.r.t. the convolution's output, d gamma / d beta; then the convolution's own backward
        gz, dg, db = _ln_backward(gy, z, g, b, mean, rstd, gelu, ln_sinks)
        gx, gw = _conv_backward_stride1(ctx.needs_input_grad[0], ctx.needs_input_grad[1], x, w, gz, g_in, dims, pad, geom, w_sink)
        gres = gy if has_res else None                      # y = ... + residual: the skip gets the incoming gradient as is
        return gx, gw, dg, db, gres, None, None, None, None, None, None


def conv_ln(x, w, gamma, beta, pad, gelu=False, residual=None, geom=None, fanout=False):
    """See _ConvLnFn.  x (B,H,W,Cin) bf16 on the device; w (Cout,KH,KW,Cin') fp32 master; gamma / beta (Cout,) fp32."""
    sg, sb = _sink(gamma), _sink(beta)
    ln_sinks = (sg, sb) if (sg is not None and sb is not None) else None
    return _ConvLnFn.apply(x, w, gamma, beta, residual, int(pad), bool(gelu), None if geom is None else tuple(int(v) for v in geom),
                           _sink(w), ln_sinks, bool(fanout))


def _as4(t):
    """(..., rows, cols) tensor -> a 4-D (b0, b1, rows, cols) view with unit inner stride (a copy only when the inner stride is not 1)."""
    if t.stride(-1) != 1:
        t = t.contiguous()
    while t.dim() < 4:
        t = t.unsqueeze(0)
    if t.dim() > 4:
        t = t.reshape(-1, *t.shape[-3:])
    return t


def _bmm_raw(a, a_km, b, b_km, M, N, K, alpha=1.0, out_dtype=None, splits=1):
    """alpha * A @ B^T with A (M x K), B (N x K) given as 4-D views, either possibly k-major; batch dims broadcast from size 1."""
    nb0, nb1 = max(a.shape[0], b.shape[0]), max(a.shape[1], b.shape[1])
    acc = splits > 1
    c = (torch.zeros if acc else torch.empty)((nb0, nb1, M, N), dtype=torch.float32 if acc else a.dtype, device=a.device)
    _lib().bmm(a, b, c, M, N, K, a_kmajor=a_km, b_kmajor=b_km, alpha=alpha, accumulate=acc, splits=splits)
    return c if (out_dtype is None or c.dtype == out_dtype) else c.to(out_dtype)


def _bmm_splits(M, N, K, batches):
    """Workgroups along the reduction when the tiles alone leave the chip idle (d refer = d rg^T @ xg: 19 200 pixels onto 80 x 64)."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * batches
    if tiles >= 256 or K < 2048:
        return 1
    return max(1, min(K // 512, 512 // tiles))


class _MatmulFn(torch.autograd.Function):
    """alpha * a @ b^T (trans_b) or alpha * a @ b over leading batch dims, forward and both gradients on gwd_bmm - strided operands,
    no transposed copies.  a (..., M, K); b (..., N, K) when trans_b else (..., K, N); batch dims of a and b equal (or 1: broadcast)."""

    @staticmethod
    def forward(ctx, a, b, trans_b, alpha):
        a4, b4 = _as4(a), _as4(b)
        M, K = a4.shape[-2:]
        N = b4.shape[-2] if trans_b else b4.shape[-1]
        c = _bmm_raw(a4, False, b4, not trans_b, M, N, K, alpha)
        ctx.save_for_backward(a4, b4)
        ctx.cfg = (trans_b, alpha, a.shape, b.shape, M, N, K)
        lead = torch.broadcast_shapes(a.shape[:-2], b.shape[:-2])
        return c.reshape(*lead, M, N)

    @staticmethod
    def backward(ctx, gc):
        a4, b4 = ctx.saved_tensors
        trans_b, alpha, ashape, bshape, M, N, K = ctx.cfg
        g4 = _as4(gc)
        ga = gb = None
        batches = g4.shape[0] * g4.shape[1]
        if ctx.needs_input_grad[0]:
            # d a (M x K) = alpha * gc (M x N) @ B'^T, B' (K x N): b (N x K) is k-major for it, b (K x N) is not
            ga = _bmm_raw(g4, False, b4, trans_b, M, K, N, alpha)
            if a4.shape[0] != g4.shape[0] or a4.shape[1] != g4.shape[1]:
                ga = ga.sum(dim=[i for i in (0, 1) if a4.shape[i] != g4.shape[i]], keepdim=True)
            ga = ga.reshape(ashape)
        if ctx.needs_input_grad[1]:
            sp = _bmm_splits(N if trans_b else K, K if trans_b else N, M, batches)
            if trans_b:       # d b (N x K) = alpha * gc^T (N x M) @ a'^T with a' (K x M): both k-major (the reduction runs over M)
                gb = _bmm_raw(g4, True, a4, True, N, K, M, alpha, out_dtype=b4.dtype, splits=sp)
            else:             # d b (K x N) = alpha * a^T (K x M) @ gc'^T with gc' (N x M): both k-major
                gb = _bmm_raw(a4, True, g4, True, K, N, M, alpha, out_dtype=b4.dtype, splits=sp)
            if b4.shape[0] != g4.shape[0] or b4.shape[1] != g4.shape[1]:
                gb = gb.sum(dim=[i for i in (0, 1) if b4.shape[i] != g4.shape[i]], keepdim=True)
            gb = gb.reshape(bshape)
        return ga, gb, None, None


def matmul_nt(a, b, alpha=1.0):
    """alpha * a @ b.transpose(-1, -2) on the library's own batched GEMM (gwd_bmm)."""
    return _MatmulFn.apply(a, b, True, float(alpha))


def matmul_nn(a, b, alpha=1.0):
    """alpha * a @ b on the library's own batched GEMM (gwd_bmm)."""
    return _MatmulFn.apply(a, b, False, float(alpha))


class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        L = x.shape[-1]
        y = torch.empty_like(x)
        _lib().softmax_forward(x, y, x.numel() // L, L)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        L = y.shape[-1]
        gx = torch.empty_like(y)
        _lib().softmax_backward(gy.contiguous(), y, gx, y.numel() // L, L)
        return gx


def softmax_lastdim(x):
    return _SoftmaxFn.apply(x)


class _AttnSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, key_mask, scale):
        x = x.contiguous()
        L = x.shape[-1]
        rows = x.numel() // L
        y = torch.empty_like(x)
        if key_mask is not None:
            key_mask = key_mask.contiguous().view(torch.uint8) if key_mask.dtype == torch.bool else key_mask.contiguous()
            rpm = rows // (key_mask.numel() // L)
        else:
            rpm = 1
        _lib().softmax_masked_forward(x, key_mask, y, rows, L, rpm, scale)
        ctx.save_for_backward(y)
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        L = y.shape[-1]
        gx = torch.empty_like(y)
        _lib().softmax_scaled_backward(gy.contiguous(), y, gx, y.numel() // L, L, ctx.scale)
        return gx, None, None


def attention_softmax(scores, key_padding_mask=None, scale=1.0):
    """softmax(scale * scores + key-padding mask) over the last dim; scores (B, H, L, S), mask (B, S) bool (True = pad)."""
    return _AttnSoftmaxFn.apply(scores, key_padding_mask, float(scale))


class _MhaFlashFn(torch.autograd.Function):
    """dropout(softmax(scale q k^T + key mask)) v with the heads merged, on the matrix cores (gwd_mha_flash_forward /
    _backward, csrc/mfattn.hip): only the merged output and one log-sum-exp per (image, head, query) are saved.
    `qk` is either one packed (B, L, 2E) projection (self-attention: q = [..., :E], k = [..., E:], ONE gradient tensor, no
    slice-backward zero-fill + add) or a (q, k) pair."""

    @staticmethod
    def forward(ctx, qk, k_sep, v, H, key_padding_mask, mult, scale):
        lib = _lib()
        packed = k_sep is None
        E = v.shape[-1]
        q, k = (qk[..., :E], qk[..., E:]) if packed else (qk, k_sep)
        B, L, S = q.shape[0], q.shape[1], k.shape[1]
        out = torch.empty((B, L, E), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
        if key_padding_mask is not None:
            key_padding_mask = key_padding_mask.contiguous().view(torch.uint8) if key_padding_mask.dtype == torch.bool else key_padding_mask.contiguous()
        lib.mha_flash_forward(q, k, v, key_padding_mask, mult, out, lse, H, scale)
        ctx.save_for_backward(qk, k_sep, v, key_padding_mask, mult, out, lse)
        ctx.cfg = (H, scale, packed)
        return out

    @staticmethod
    def backward(ctx, go):
        qk, k_sep, v, kpm, mult, out, lse = ctx.saved_tensors
        H, scale, packed = ctx.cfg
        E = v.shape[-1]
        q, k = (qk[..., :E], qk[..., E:]) if packed else (qk, k_sep)
        go = go.contiguous()
        gqk = torch.empty_like(qk)
        gk_sep = None if packed else torch.empty_like(k_sep)
        gq, gk = (gqk[..., :E], gqk[..., E:]) if packed else (gqk, gk_sep)
        gv = torch.empty_like(v)
        delta = torch.empty_like(lse)
        _lib().mha_flash_backward(q, k, v, go, out, kpm, mult, lse, delta, gq, gk, gv, H, scale)
        return gqk, gk_sep, gv, None, None, None, None


def _dense_rows(t):
    """(B, tokens, C) view acceptable to the attention kernels: unit channel stride, dense token rows, 16-byte aligned rows."""
    ok = (t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1) and (t.stride(1) * t.element_size()) % 16 == 0
          and t.data_ptr() % 16 == 0)
    return t if ok else t.contiguous()


def mha_core(qk, k, v, heads, key_padding_mask, dropout_p, training, scale, mult=None):
    """Attention core of one MultiheadAttention call (multi_head_attention.py:329-375) as ONE kernel each way.  qk: the packed
    (B, L, 2E) q|k projection with k=None, or q with a separate k (B, S, E); v (B, S, E).  Returns the merged (B, L, E) output,
    or None when the kernels do not cover the call (not bf16 on a HIP device, head_dim != 32): the caller keeps the unfused
    path (the fp32 parity mode)."""
    E = v.shape[-1]
    if not v.is_cuda or v.dtype != torch.bfloat16 or E // heads != 32:
        return None
    B, L = qk.shape[0], qk.shape[1]
    S = v.shape[1]
    if mult is None and training and dropout_p > 0:      # no pool: ATen's graph-safe Philox stream decides which probabilities are dropped
        mult = F.dropout(torch.ones((B, heads, L, S), dtype=v.dtype, device=v.device), dropout_p, True)
    return _MhaFlashFn.apply(_dense_rows(qk), None if k is None else _dense_rows(k), _dense_rows(v), int(heads), key_padding_mask,
                             mult, float(scale))


class _SilogFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, weight, lam, log_err):
        lib = _lib()
        pred = pred.contiguous()
        B = pred.shape[0]
        # accepted layouts: (B,h,w,1) pixel-major or (B,1,h,w); both are the same bytes
        if pred.dim() == 4 and pred.shape[-1] == 1:
            h, w = pred.shape[1], pred.shape[2]
        elif pred.dim() == 4 and pred.shape[1] == 1:
            h, w = pred.shape[2], pred.shape[3]
        else:
            h, w = pred.shape[-2], pred.shape[-1]
        H, W = gt.shape[-2], gt.shape[-1]
        sums = torch.zeros(3, dtype=torch.float64, device=pred.device)
        lib.silog_sums(pred, gt, sums, B, h, w, H, W, log_err)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        lib.silog_finalize(sums, lam, 10.0 * weight, loss)       # 10 w sqrt(E[d^2] - lam E[d]^2), one launch
        ctx.save_for_backward(pred, gt, sums)
        ctx.cfg = (B, h, w, H, W, weight, lam, log_err)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred, gt, sums = ctx.saved_tensors
        B, h, w, H, W, weight, lam, log_err = ctx.cfg
        gp = torch.empty_like(pred)
        _lib().silog_backward(pred, gt, sums, gloss.contiguous().float(), weight, lam, gp, B, h, w, H, W, log_err)
        return gp, None, None, None, None


def silog_loss(pred, gt_full, weight=1.0, variance_focus=0.85, log_depth_error=True):
    """weight * SiLog(pred, nearest_resize(gt), nearest_resize(0.2 <= gt < 10)); gt_full (B,1,H,W)/(B,H,W) fp32."""
    return _SilogFn.apply(pred, gt_full.contiguous(), float(weight), float(variance_focus), bool(log_depth_error))


class _SegCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, scale):
        logits = logits.contiguous()
        P = logits.numel() // 2
        s = torch.zeros(1, dtype=torch.float64, device=logits.device)
        _lib().seg_ce_sum(logits, target, s, P)
        ctx.save_for_backward(logits, target)
        ctx.cfg = (P, scale)
        return (s[0] * (scale / P)).float()

    @staticmethod
    def backward(ctx, gloss):
        logits, target = ctx.saved_tensors
        P, scale = ctx.cfg
        gl = torch.empty_like(logits)
        _lib().seg_ce_backward(logits, target, gloss.contiguous().float(), scale, gl, P)
        return gl, None, None


def seg_cross_entropy(logits_pixel_major, target, scale=1.0):
    """scale * mean CE of (B,H,W,2) logits against (B,H,W) int64 targets."""
    return _SegCEFn.apply(logits_pixel_major, target.contiguous(), float(scale))


class _ResampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, mode):
        x = x.contiguous()
        B, Hs, Ws, C = x.shape
        y = torch.empty((B, size[0], size[1], C), dtype=x.dtype, device=x.device)
        _lib().resample_forward(x, y, B, Hs, Ws, size[0], size[1], C, mode)
        ctx.cfg = (B, Hs, Ws, size[0], size[1], C, mode)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, Hs, Ws, Ho, Wo, C, mode = ctx.cfg
        gy = gy.contiguous()
        gx = torch.empty((B, Hs, Ws, C), dtype=gy.dtype, device=gy.device)
        lib = _lib()
        done = False
        if C % 4 == 0 and (Ho > Hs or Wo > Ws):
            tmp = torch.empty(lib.workspace_bytes(hip.WS_RESAMPLE_BWD, B, Ho, Ws, C) // 4, dtype=torch.float32, device=gy.device)   # x pass -> y pass scratch
            done = lib.resample_backward_sep(gy, tmp, gx, B, Hs, Ws, Ho, Wo, C, mode)
        if not done:
            lib.resample_backward(gy, gx, B, Hs, Ws, Ho, Wo, C, mode)
        return gx, None, None


class _PspPoolFn(torch.autograd.Function):
    """x -> (x itself, avg_pool 16, 8, 4, 2 of x): the pooling side of the PSP module (points_sample.py:107-113) as one pass forward
    and one pass backward.  The first output is x again, for the consumer that takes the map itself (the concat): with it this node
    is x's ONLY consumer, so the five gradients arrive together and leave as one tensor (was four pool backward kernels and four
    accumulation passes over the full map)."""

    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        outs = [torch.empty((B, H // k, W // k, C), dtype=x.dtype, device=x.device) for k in (16, 8, 4, 2)]
        if not _lib().psp_pool_forward(x, *outs):
            raise ValueError("psp_pools: unsupported shape %r" % (tuple(x.shape),))
        ctx.shape = tuple(x.shape)
        return (x.view_as(x),) + tuple(outs)

    @staticmethod
    def backward(ctx, g_pass, g16, g8, g4, g2):
        B, H, W, C = ctx.shape
        like = next(g for g in (g_pass, g16, g8, g4, g2) if g is not None)
        gx = torch.empty((B, H, W, C), dtype=like.dtype, device=like.device)
        con = lambda g: None if g is None else g.contiguous()
        _lib().psp_pool_backward(g_pass, con(g16), con(g8), con(g4), con(g2), gx)
        return gx


def psp_pools(x, pools):
    """(x, [avg_pool(x, k) for k in pools]); fused into one pass each way for the reference's pools (16, 8, 4, 2)."""
    B, H, W, C = x.shape
    vec = 8 if x.dtype == torch.bfloat16 else 4
    if tuple(pools) == (16, 8, 4, 2) and H >= 16 and W >= 16 and C % vec == 0 and x.is_contiguous():
        outs = _PspPoolFn.apply(x)
        return outs[0], list(outs[1:])
    return x, [avg_pool(x, k) for k in pools]


def _pyramid_cat_forward(x, ys):
    """-> ([x | up(y_1) | ... | up(y_n)], cfg for _pyramid_cat_backward): see _PyramidCatFn."""
    lib = _lib()
    x = x.contiguous()
    B, H, W, C = x.shape
    n = len(ys)
    out = torch.empty((B, H, W, (n + 1) * C), dtype=x.dtype, device=x.device)
    out[..., :C].copy_(x)
    shapes = []
    for k, y in enumerate(ys):
        y = y.contiguous()
        if y.shape[0] != B or y.shape[3] != C:
            raise ValueError("pyramid_concat: branch %d has shape %r" % (k, tuple(y.shape)))
        lib.resample_forward(y, out[..., (k + 1) * C:(k + 2) * C], B, y.shape[1], y.shape[2], H, W, C, hip.RESAMPLE_BILINEAR_AC)
        shapes.append((y.shape[1], y.shape[2]))
    return out, (B, H, W, C, shapes)


def _pyramid_cat_backward(cfg, g):
    """g, the gradient of _pyramid_cat_forward's result -> [the gradient of x (a view of g), of y_1, ..., of y_n]."""
    lib = _lib()
    B, H, W, C, shapes = cfg
    g = g.contiguous()
    grads = [g[..., :C]]
    for k, (h, w) in enumerate(shapes):
        gk = g[..., (k + 1) * C:(k + 2) * C]
        gy = torch.empty((B, h, w, C), dtype=g.dtype, device=g.device)
        tmp = torch.empty(lib.workspace_bytes(hip.WS_RESAMPLE_BWD, B, H, w, C) // 4, dtype=torch.float32, device=g.device)
        if not lib.resample_backward_sep(gk, tmp, gy, B, h, w, H, W, C, hip.RESAMPLE_BILINEAR_AC):
            lib.resample_backward(gk.contiguous(), gy, B, h, w, H, W, C, hip.RESAMPLE_BILINEAR_AC)
        grads.append(gy)
    return grads


class _PyramidCatFn(torch.autograd.Function):
    """cat([x, up(y_1), ..., up(y_n)], channels) with up = bilinear(align_corners) to x's size (the PSP tail of
    points_sample.py:114-122) WITHOUT the concat pass: the up-sampling kernels write their channel slice of the result directly
    (pixel pitch = (n + 1) C), only x itself is copied; backward reads the slices in place (no .contiguous() copies) and hands
    x its slice of the gradient as a view."""

    @staticmethod
    def forward(ctx, x, *ys):
        out, ctx.cfg = _pyramid_cat_forward(x, ys)
        return out

    @staticmethod
    def backward(ctx, g):
        return tuple(_pyramid_cat_backward(ctx.cfg, g))


def pyramid_concat(x, ys):
    """x (B,H,W,C) and low-resolution maps ys[k] (B,h_k,w_k,C) -> (B,H,W,(1+len(ys)) C) = [x | bilinear_ac(ys[k] -> H,W) ...]."""
    C = x.shape[-1]
    if C % 8 or not ys:
        return torch.cat([x] + [upsample_bilinear_ac(y, x.shape[1:3]) for y in ys], dim=-1)
    return _PyramidCatFn.apply(x, *ys)


PYRAMID_TAIL_LOWRES = True       # PyramidLayer's last ConvLn: convolve the coarse PSP branches at their own resolution (pyramid_tail)
PYRAMID_TAIL_NLOW = 3            # how many of the branches (coarsest first) go that way; the rest stay in the high-resolution concat


class _PyramidTailFn(torch.autograd.Function):
    """[GELU](LayerNorm(conv3x3([x | up(y_1) | ... | up(y_n)], w))) without convolving the up-sampled coarse branches at full
    resolution.  conv and the bilinear resize are linear and the channel mixing commutes with the resize:
        conv3x3(up(y))(p) = sum_tap [p + tap inside] up(W_tap . y)(p + tap),
    so the first nlow branches get their nine channel products as ONE 1x1 convolution on their own pixels (y_k -> Z_k, 9 N
    channels); the 3x3 convolution runs on [x | the other branches] only and gwd_pyr_tail_forward adds the bilinear gather of the
    Z_k and normalises.  Backward is the transpose: gwd_layernorm_backward, the high-resolution data / weight gradient,
    gwd_pyr_tail_backward (gz -> the gradient of every Z_k) and the 1x1 gradients; the partial weight gradients are folded into
    the one parameter's layout by gwd_pyr_tail_fold_wgrad."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, gelu, nlow, w_sink, ln_sinks, *ys):
        lib = _lib()
        B, H, W, C2 = x.shape
        N = w.shape[0]
        nbr = len(ys)
        if tuple(w.shape) != (N, 3, 3, (1 + nbr) * C2) or not 1 <= nlow <= nbr:
            raise ValueError("pyramid_tail: weight %r does not fit %d branches of %d channels" % (tuple(w.shape), nbr, C2))
        dt = x.dtype
        lows = [y.contiguous() for y in ys[:nlow]]
        cat, cat_cfg = _pyramid_cat_forward(x, ys[nlow:]) if nlow < nbr else (x.contiguous(), None)
        Chi = cat.shape[-1]
        w_hi = derived_weight(w, ("pyr_tail_hi", nlow), lambda: torch.cat([w.detach()[..., :C2], w.detach()[..., (1 + nlow) * C2:]], dim=-1))
        w_lo = [derived_weight(w, ("pyr_tail_lo", k), lambda k=k: w.detach()[..., (k + 1) * C2:(k + 2) * C2].permute(1, 2, 0, 3)
                               .reshape(9 * N, 1, 1, C2).contiguous()) for k in range(nlow)]
        part = torch.empty((B, H, W, N), dtype=dt, device=x.device)
        dims = (B, H, W, Chi, H, W, N, 3, 3)
        lib.conv_forward(cat, _weight_for(w_hi, None, dt), part, dims, stride=1, pad=1)
        Zs = []
        for y, wl in zip(lows, w_lo):
            h, wd = y.shape[1], y.shape[2]
            Z = torch.empty((B, h, wd, 9, N), dtype=dt, device=x.device)
            lib.conv_forward(y, _weight_for(wl, None, dt), Z.view(B, h, wd, 9 * N), (B, h, wd, C2, h, wd, 9 * N, 1, 1), stride=1, pad=0)
            Zs.append(Z)
        need_grad = any(ctx.needs_input_grad)
        out = torch.empty_like(part)
        z = torch.empty_like(part) if need_grad else None           # inference: the sum itself is never written
        mean = torch.empty(B * H * W, dtype=torch.float32, device=x.device)
        rstd = torch.empty(B * H * W, dtype=torch.float32, device=x.device)
        g, b = gamma.detach(), beta.detach()
        if lib.pyr_tail_forward(part, Zs, g, b, z, out, mean, rstd, gelu) is False:
            raise ValueError("pyramid_tail: no kernel for N = %d with branches %r" % (N, [tuple(y.shape[1:3]) for y in lows]))
        if need_grad:
            ctx.save_for_backward(cat, w, z, g, b, mean, rstd, *lows)
        ctx.cfg = (dims, bool(gelu), nlow, nbr, C2, w_sink, ln_sinks, cat_cfg, w_hi, w_lo)
        return out

    @staticmethod
    def backward(ctx, gy):
        lib = _lib()
        cat, w, z, g, b, mean, rstd, *lows = ctx.saved_tensors
        dims, gelu, nlow, nbr, C2, w_sink, ln_sinks, cat_cfg, w_hi, w_lo = ctx.cfg
        B, H, W, Chi, _, _, N, _, _ = dims
        dt = cat.dtype
        gz, dg, db = _ln_backward(gy.contiguous(), z, g, b, mean, rstd, gelu, ln_sinks)
        # ---- high-resolution part: data gradient of [x | the remaining branches], then the concat's own backward
        g_cat = _dgrad_stride1(gz, _weight_transposed(w_hi, None, dt), cat, dims, 1)
        g_high = _pyramid_cat_backward(cat_cfg, g_cat) if nlow < nbr else [g_cat]
        # ---- low-resolution part: the gradients of the product maps, then the 1x1 data gradients
        Gs = [torch.empty((B, y.shape[1], y.shape[2], 9, N), dtype=dt, device=z.device) for y in lows]
        lib.pyr_tail_backward(gz, Gs)
        # per branch: (y_k, the gradient of Z_k as one map of 9 N channels, the dims of the 1x1 convolution y_k -> Z_k)
        low = [(y, G.view(B, y.shape[1], y.shape[2], 9 * N), (B, y.shape[1], y.shape[2], C2, y.shape[1], y.shape[2], 9 * N, 1, 1))
               for y, G in zip(lows, Gs)]
        g_low = [_dgrad_stride1(G, _weight_transposed(wl, None, dt), y, d, 0) for (y, G, d), wl in zip(low, w_lo)]
        # ---- weight gradients: each part in its own shape, folded into the parameter's layout once all have been issued
        gw = None
        if ctx.needs_input_grad[1]:
            d_hi = WGRADS.scratch((N, 3, 3, Chi), z.device)
            d_lo = [WGRADS.scratch((9 * N, 1, 1, C2), z.device) for _ in lows]
            if w_sink is None:
                gw = torch.zeros(w.shape, dtype=torch.float32, device=w.device)
            dst = gw if w_sink is None else w_sink[0].view(w.shape)

            def fold(d_hi=d_hi, d_lo=d_lo, dst=dst, hook=None if w_sink is None else w_sink[1]):
                lib.pyr_tail_fold_wgrad(d_hi, d_lo, dst, C2)
                if hook is not None:
                    hook()

            WGRADS.add(cat, gz, d_hi, dims, dict(stride=1, pad=1))
            for i, ((y, G, d), dw) in enumerate(zip(low, d_lo)):
                WGRADS.add(y, G, dw, d, dict(stride=1, pad=0), fold if i == len(lows) - 1 else None)
        return tuple(g_high[:1] + [gw, dg, db] + [None] * 4 + g_low + g_high[1:])


def pyramid_tail_supported(x, ys, w):
    """The shapes gwd_pyr_tail_forward / _backward take (PyramidLayer picks the route with this)."""
    N, C2 = w.shape[0], x.shape[-1]
    return (x.is_cuda and not getattr(_lib(), "is_fake", False) and x.dtype in (torch.float32, torch.bfloat16) and C2 % 8 == 0
            and N % 32 == 0 and N <= 320 and len(ys) > PYRAMID_TAIL_NLOW >= 1 and tuple(w.shape[1:]) == (3, 3, (1 + len(ys)) * C2))


def pyramid_tail(x, ys, w, gamma, beta, gelu=False, nlow=None):
    """x (B,H,W,C2), ys[k] (B,h_k,w_k,C2) coarsest first, w (N,3,3,(1+len(ys)) C2) fp32 master, gamma / beta (N,) ->
    [GELU](LayerNorm(conv3x3(pyramid_concat(x, ys), w))): see _PyramidTailFn."""
    sg, sb = _sink(gamma), _sink(beta)
    ln_sinks = (sg, sb) if (sg is not None and sb is not None) else None
    return _PyramidTailFn.apply(x, w, gamma, beta, bool(gelu), int(PYRAMID_TAIL_NLOW if nlow is None else nlow), _sink(w), ln_sinks, *ys)


def upsample_bilinear_ac(x, size):
    """(B,Hs,Ws,C) -> (B,H,W,C), bilinear with align_corners=True."""
    return _ResampleFn.apply(x, tuple(size), hip.RESAMPLE_BILINEAR_AC)


def upsample_nearest(x, size):
    """(B,Hs,Ws,C) -> (B,H,W,C), legacy nearest (floor(dst * in / out))."""
    return _ResampleFn.apply(x, tuple(size), hip.RESAMPLE_NEAREST)


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        x = x.contiguous()
        B, H, W, C = x.shape
        y = torch.empty((B, H // k, W // k, C), dtype=x.dtype, device=x.device)
        _lib().avgpool_forward(x, y, B, H, W, C, k)
        ctx.cfg = (B, H, W, C, k)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, H, W, C, k = ctx.cfg
        gx = torch.empty((B, H, W, C), dtype=gy.dtype, device=gy.device)
        _lib().avgpool_backward(gy.contiguous(), gx, B, H, W, C, k)
        return gx, None


def avg_pool(x, k):
    """k x k average pooling with stride k on a pixel-major map."""
    return _AvgPoolFn.apply(x, int(k))


def _unit_last(t):
    """The attention kernels take any window / token / head strides, but a unit channel stride."""
    return t if t.stride(-1) == 1 else t.contiguous()


def _winattn_table_grad(tb, sink, run, rel):
    """Backward of the relative-position table of a window attention: run(dbias, head_major) launches the kernel.  On the device the
    kernel accumulates into a zeroed (heads, n_rel) scratch - a wave's flush is then one contiguous run of atomics instead of n_rel
    4-byte adds in n_rel different 64-byte segments, 41-59 us of every launch - and the transposed scratch is added to the table's
    gradient (the flat-buffer slice when there is a sink).  Returns what autograd gets for the table (None with a sink)."""
    direct = sink is not None
    if tb.is_cuda and rel is not None:
        tmp = WGRADS.scratch((tb.shape[1], tb.shape[0]), tb.device)
        run(tmp, True)
        if not direct:
            return tmp.t().contiguous()
        sink[0].view(tb.shape).add_(tmp.t())
    else:
        dtab = sink[0] if direct else torch.zeros_like(tb)
        run(dtab, False)
        if not direct:
            return dtab
    if sink[1] is not None:
        sink[1]()
    return None


class QkvHandle:
    """The packed qkv projection as ref_scores(..., handle=True) hands it on: a second output of that node, so the gradient of what
    reads it travels to ref_scores' backward on an autograd edge.  That backward writes (or zeroes) the q slot of the arriving gradient
    and never reads it: a consumer of the handle reads the k / v slots only and leaves the q slot of its gradient unwritten."""
    __slots__ = ("qkv",)

    def __init__(self, qkv):
        self.qkv = qkv


class _WinAttnFn(torch.autograd.Function):
    """Window attention (W, 49, H*D).  Operand i of q / k / v is the given tensor (W, 49, H, D), or slot i of the packed projection
    qkv (W, 49, 3, H, D) - as the qkv Linear writes it - where the tensor is None.  The operands taken from qkv get their gradient as
    views of ONE packed tensor; a slot no operand came from is zero-filled when `fill`, else left unwritten (QkvHandle).  `table` is the
    relative-position bias PARAMETER (n_rel, heads), gathered through rel (49*49 int32) inside the kernels; its gradient is accumulated
    by the backward kernel straight into the flat gradient buffer when the parameter is managed by engine.TrainStep (sink)."""

    @staticmethod
    def forward(ctx, q, k, v, qkv, table, rel, region, wpi, scale, sink, fill):
        own = [None if t is None else _unit_last(t) for t in (q, k, v)]
        if qkv is not None:
            qkv = qkv.contiguous()
        q, k, v = (qkv[:, :, i] if t is None else t for i, t in enumerate(own))
        W, N, H, D = q.shape
        out = torch.empty((W, N, H, D), dtype=q.dtype, device=q.device)
        tb = table.detach()
        _lib().winattn_forward(q, k, v, out, tb, region, wpi, scale, rel_index=rel)
        ctx.save_for_backward(qkv, *own, tb, rel, region)
        ctx.cfg = (wpi, scale, fill)
        ctx.sink = sink
        return out.view(W, N, H * D)

    @staticmethod
    def backward(ctx, go):
        qkv, *own, tb, rel, region = ctx.saved_tensors
        wpi, scale, fill = ctx.cfg
        q, k, v = (qkv[:, :, i] if t is None else t for i, t in enumerate(own))
        W, N, H, D = q.shape
        go = go.contiguous().view(W, N, H, D)
        g = None if qkv is None else torch.empty_like(qkv)
        gs = [g[:, :, i] if t is None else torch.empty((W, N, H, D), dtype=q.dtype, device=q.device) for i, t in enumerate(own)]
        if g is not None and fill:
            for i, t in enumerate(own):
                if t is not None:
                    g[:, :, i].zero_()
        gtab = _winattn_table_grad(tb, ctx.sink, lambda dtab, hm: _lib().winattn_backward(
            q, k, v, go, *gs, tb, dtab, region, wpi, scale, rel_index=rel, head_major=hm), rel)
        return (*(None if t is None else gt for t, gt in zip(own, gs)), g, gtab) + (None,) * 6


def _win_attn(q, k, v, qkv, table, rel, region, windows_per_image, scale, fill=True):
    return _WinAttnFn.apply(q, k, v, qkv, table, rel, region, int(windows_per_image), float(scale), _sink(table), fill)


def window_attention_qkv(q_new, qkv, table, rel, region, windows_per_image, scale):
    """softmax(scale*q_new k^T + bias (+shift mask)) v with k, v = qkv[:, :, 1], qkv[:, :, 2] (the 1/32 stage): the gradient of qkv
    comes back as ONE packed tensor instead of two zero-filled select-backward temporaries and their sum.  qkv: the packed projection
    (the q slot of its gradient is zero-filled), or the QkvHandle that ref_scores returned for it (the q slot is left to that backward)."""
    handle = isinstance(qkv, QkvHandle)
    return _win_attn(q_new, None, None, qkv.qkv if handle else qkv, table, rel, region, windows_per_image, scale, fill=not handle)


def window_attention_packed(qkv, table, rel, region, windows_per_image, scale):
    """softmax(scale*q k^T + bias (+shift mask)) v over 49-token windows; qkv (W,49,3,H,D); bias(h,i,j) = table[rel[i*49+j], h]."""
    return _win_attn(None, None, None, qkv, table, rel, region, windows_per_image, scale)


def window_attention(q, k, v, table, rel, region, windows_per_image, scale):
    """Separate q / k / v operands (W, 49, H, D): bf16 on the matrix cores (csrc/mfattn.hip, head_dim 4..32), fp32 on the
    lane-per-row kernels (csrc/winattn.hip)."""
    return _win_attn(q, k, v, None, table, rel, region, windows_per_image, scale)


class _RowAffineFn(torch.autograd.Function):
    """mu + exp(logsigma) * x with per-channel mu / logsigma (the reference tokens' re-parameterisation,
    multiscale_transformerr.py:289-292).  The parameter gradients are column sums over the rows: own colsum kernel straight into
    the flat gradient buffer - ATen's multi-block reduction zeroes its semaphore with an asynchronous memset once the row count grows
    (batch 16), which a HIP graph cannot replay (graphs.refusal: the capture is refused)."""

    @staticmethod
    def forward(ctx, x, mu, logsigma, sinks):
        e = logsigma.detach().exp().to(x.dtype)
        ctx.save_for_backward(x, e)
        ctx.sinks = sinks
        ctx.shapes = (mu.shape, logsigma.shape)
        return mu.detach().to(x.dtype) + e * x

    @staticmethod
    def backward(ctx, g):
        x, e = ctx.saved_tensors
        g = g.contiguous()
        C = g.shape[-1]
        rows = g.numel() // C
        gl = (g * x * e).contiguous()
        outs = []
        for t, sink, shape in ((g, ctx.sinks[0], ctx.shapes[0]), (gl, ctx.sinks[1], ctx.shapes[1])):
            if sink is not None:
                COLSUMS.add(t, sink[0].view(-1), rows, C, sink[1])
                outs.append(None)
            else:
                o = torch.zeros(C, dtype=torch.float32, device=g.device)
                _lib().colsum(t, o, rows, C)
                outs.append(o.view(shape))
        return g * e, outs[0], outs[1], None


def row_affine(x, mu, logsigma):
    """mu + exp(logsigma) * x, x (..., C), mu / logsigma (1, 1, C) parameters."""
    return _RowAffineFn.apply(x, mu, logsigma, (_sink(mu), _sink(logsigma)))


class _RefScoresFn(torch.autograd.Function):
    """ra (B, nwin*49, R, H) = scale * q . ref_k per head (multiscale_transformerr.py:296-298); q is read in place from the packed
    qkv projection (W, 49, 3, H, hd) and its gradient comes back as ONE packed tensor.  With `handle` the node returns qkv itself next
    to ra (an alias: no copy, no launch) for the other consumer of the projection, and the gradient of that output is the packed
    tensor this backward completes: its k / v slots are kept, its q slot is never read - only overwritten with ra's gradient, or zeroed
    where ra got none.  Without an arriving packed gradient the k / v slots are zero."""

    @staticmethod
    def forward(ctx, qkv, ref_k, B, scale, handle):
        ctx.set_materialize_grads(False)
        qkv, ref_k = qkv.contiguous(), ref_k.contiguous()
        W, N, _, H, hd = qkv.shape
        R = ref_k.shape[1]
        ra = torch.empty((B, (W // B) * N, R, H), dtype=qkv.dtype, device=qkv.device)
        _lib().ref_scores_forward(qkv[:, :, 0], ref_k, ra, B, W // B, scale)
        ctx.save_for_backward(qkv, ref_k)
        ctx.cfg = (B, scale)
        return (ra, qkv) if handle else ra

    @staticmethod
    def backward(ctx, g, gqkv=None):
        qkv, ref_k = ctx.saved_tensors
        B, scale = ctx.cfg
        if gqkv is None:
            gqkv = torch.zeros_like(qkv)
        if g is None:
            gqkv[:, :, 0].zero_()
            return gqkv, None, None, None, None
        dk = torch.empty(ref_k.shape, dtype=torch.float32, device=g.device)
        _lib().ref_scores_backward(qkv[:, :, 0], ref_k, g.contiguous(), gqkv[:, :, 0], dk, B, qkv.shape[0] // B, scale)
        return gqkv, dk.to(ref_k.dtype), None, None, None


class _RefMixFn(torch.autograd.Function):
    """q_new (B, T, C) = softmax_r(ra) . ref_v per head (multiscale_transformerr.py:304-309)."""

    @staticmethod
    def forward(ctx, ra, ref_v, H):
        ra, ref_v = ra.contiguous(), ref_v.contiguous()
        B, T = ra.shape[0], ra.shape[1]
        q_new = torch.empty((B, T, ref_v.shape[2]), dtype=ra.dtype, device=ra.device)
        att = torch.empty_like(ra) if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) else None
        _lib().ref_mix_forward(ra, ref_v, q_new, att, H)
        ctx.save_for_backward(att, ref_v)
        ctx.H = H
        return q_new

    @staticmethod
    def backward(ctx, g):
        att, ref_v = ctx.saved_tensors
        d_ra = torch.empty_like(att)
        dv = torch.empty(ref_v.shape, dtype=torch.float32, device=g.device)
        _lib().ref_mix_backward(att, ref_v, g.contiguous(), d_ra, dv, ctx.H)
        return d_ra, dv.to(ref_v.dtype), None


def ref_scores(qkv, ref_k, images, scale, handle=False):
    """qkv (images*nwin, 49, 3, H, hd) packed projection, ref_k (images, R, H*hd) -> (images, nwin*49, R, H); handle: -> (that, the
    QkvHandle to give window_attention_qkv in place of qkv, so that ONE packed gradient comes back for the projection)."""
    if not handle:
        return _RefScoresFn.apply(qkv, ref_k, int(images), float(scale), False)
    ra, alias = _RefScoresFn.apply(qkv, ref_k, int(images), float(scale), True)
    return ra, QkvHandle(alias)


def ref_mix(ra, ref_v, heads):
    """ra (images, T, R, H), ref_v (images, R, H*hd) -> (images, T, H*hd)."""
    return _RefMixFn.apply(ra, ref_v, int(heads))


class _TokAttnFn(torch.autograd.Function):
    """Class-token attention of one query, or of two that share k / v (token_attention_pair sends two only where the pair kernels
    exist): the pair is one launch each way, and its gk / gv are already the sum autograd would form from two nodes.  Where the library
    declines the pair call the single kernel runs per query and gk / gv are summed here.  ts: the queries, then k, v."""

    @staticmethod
    def forward(ctx, scale, *ts):
        *qs, k, v = [_unit_last(t) for t in ts]
        W, N, H, R = qs[0].shape
        outs = [torch.empty((W, N, H, R), dtype=q.dtype, device=q.device) for q in qs]
        if len(qs) == 1 or _lib().tokattn_pair_forward(*qs, k, v, *outs, scale) is False:
            for q, o in zip(qs, outs):
                _lib().tokattn_forward(q, k, v, o, scale)
        ctx.save_for_backward(*qs, k, v)
        ctx.scale = scale
        return tuple(o.view(W, N, H * R) for o in outs)

    @staticmethod
    def backward(ctx, *gos):
        *qs, k, v = ctx.saved_tensors
        W, N, H, R = qs[0].shape
        gos = [go.contiguous().view(W, N, H, R) for go in gos]
        gqs = [torch.empty_like(go) for go in gos]
        gk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        gv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        if len(qs) == 1 or _lib().tokattn_pair_backward(*qs, k, v, *gos, *gqs, gk, gv, ctx.scale) is False:
            _lib().tokattn_backward(qs[0], k, v, gos[0], gqs[0], gk, gv, ctx.scale)
            if len(qs) == 2:                             # summed as autograd sums two nodes
                gk2, gv2 = torch.empty_like(gk), torch.empty_like(gv)
                _lib().tokattn_backward(qs[1], k, v, gos[1], gqs[1], gk2, gv2, ctx.scale)
                gk, gv = gk + gk2, gv + gv2
        return (None, *gqs, gk, gv)


def token_attention(q, k, v, scale):
    """Class-token attention: q (W,49,H,4), k/v (W,49,H,e) -> (W,49,4H); softmax over the e feature channels."""
    return _TokAttnFn.apply(float(scale), q, k, v)[0]


def token_attention_pair(q, q2, k, v, scale):
    """token_attention(q, k, v), token_attention(q2, k, v); bf16 with e in {12, 16, 24}: one launch for the pair."""
    if q.dtype == torch.bfloat16 and k.shape[3] in (12, 16, 24):
        return _TokAttnFn.apply(float(scale), q, q2, k, v)
    return token_attention(q, k, v, scale), token_attention(q2, k, v, scale)


def _window_map_each(srcs, dsts, B, H, W, Cs, shift, gather, residuals=None):
    """One map: window_map.  Several: window_map_multi, or - when the library declines the joint launch - window_map per map."""
    if len(srcs) > 1 and _lib().window_map_multi(srcs, dsts, B, H, W, Cs, shift, gather, residuals=residuals) is not False:
        return
    for i, (s, d, c) in enumerate(zip(srcs, dsts, Cs)):
        _lib().window_map(s, d, B, H, W, c, shift, gather, residual=None if residuals is None else residuals[i])


class _WindowMapFn(torch.autograd.Function):
    """The 7x7 window partition (gather) or its reverse (scatter, with optional residual streams) of n maps of one geometry, as ONE
    launch each way; args: n maps, then the residuals (n for a scatter, none for a gather).  The backward is the opposite map."""

    @staticmethod
    def forward(ctx, gather, B, H, W, shift, n, *ts):
        srcs = [t.contiguous() for t in ts[:n]]
        ress = [None if r is None else r.contiguous() for r in ts[n:]]
        Cs = [s.shape[-1] for s in srcs]
        shape = (B * ((H + 6) // 7) * ((W + 6) // 7), 49) if gather else (B, H, W)
        dsts = [torch.empty(shape + (c,), dtype=s.dtype, device=s.device) for s, c in zip(srcs, Cs)]
        _window_map_each(srcs, dsts, B, H, W, Cs, shift, gather, residuals=ress or None)
        ctx.cfg = (gather, B, H, W, shift, Cs, [tuple(s.shape) for s in srcs], [r is not None and tuple(r.shape) for r in ts[n:]])
        return tuple(dsts)

    @staticmethod
    def backward(ctx, *gs):
        gather, B, H, W, shift, Cs, shapes, rshapes = ctx.cfg
        gs = [g.contiguous() for g in gs]
        outs = [torch.empty(sh, dtype=g.dtype, device=g.device) for g, sh in zip(gs, shapes)]
        _window_map_each(gs, outs, B, H, W, Cs, shift, not gather)
        return (None,) * 6 + tuple(outs) + tuple((g.view(rs) if rs else None) for g, rs in zip(gs, rshapes))


def window_gather_multi(xs, shift):
    """[window_gather(x, shift) for x in xs] (maps of one (B, H, W), any channel counts, at most 4) in one launch."""
    B, H, W = xs[0].shape[:3]
    return _WindowMapFn.apply(True, B, H, W, int(shift), len(xs), *xs)


def window_scatter_multi(wins, B, H, W, shift, residuals):
    """[window_scatter(w, B, H, W, shift, r) for w, r in zip(wins, residuals)] in one launch."""
    return _WindowMapFn.apply(False, int(B), int(H), int(W), int(shift), len(wins), *wins, *residuals)


def window_gather(x, shift):
    """(B,H,W,C) -> (B*nWin, 49, C): zero-pad to multiples of 7, cyclic shift by -shift, 7x7 window partition."""
    return window_gather_multi([x], shift)[0]


def window_scatter(win, B, H, W, shift, residual=None):
    """Inverse of window_gather (window reverse, un-shift, crop) -> (B,H,W,C) [+ residual, any shape with B*H*W*C elements]."""
    return window_scatter_multi([win], B, H, W, shift, [residual])[0]


class _InormGeluFn(torch.autograd.Function):
    SLICES = 32

    @staticmethod
    def forward(ctx, a, u, eps):
        a, u = a.contiguous(), u.contiguous()
        B, C = u.shape[0], u.shape[-1]
        L = u.numel() // (B * C)
        S = _InormGeluFn.SLICES
        y = torch.empty_like(u)
        part = torch.empty(_lib().workspace_bytes(hip.WS_INORM_GELU, B, S, C) // 4, dtype=torch.float32, device=u.device)
        stat = torch.empty((B, C, 2), dtype=torch.float32, device=u.device)
        _lib().inorm_gelu_forward(a, u, y, part, stat, B, L, C, S, float(eps))
        ctx.save_for_backward(u, stat)
        ctx.cfg = (B, L, C, S)
        return y

    @staticmethod
    def backward(ctx, gy):
        u, stat = ctx.saved_tensors
        B, L, C, S = ctx.cfg
        gy = gy.contiguous()
        du = torch.empty_like(u)
        part = torch.empty(_lib().workspace_bytes(hip.WS_INORM_GELU, B, S, C) // 4, dtype=torch.float32, device=u.device)
        _lib().inorm_gelu_backward(gy, u, stat, part, du, B, L, C, S)
        return gy, du, None


class _AnchorDepthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, att, anchor):
        B, P, R = att.shape
        att = att.contiguous()
        anchor = anchor.float().contiguous()
        pred = torch.empty((B, P), dtype=torch.float32, device=att.device)
        _lib().anchor_depth_forward(att, anchor, pred, B, P, R)
        ctx.save_for_backward(att, anchor)
        return pred

    @staticmethod
    def backward(ctx, g):
        att, anchor = ctx.saved_tensors
        B, P, R = att.shape
        datt = torch.empty_like(att) if ctx.needs_input_grad[0] else None
        danchor = torch.zeros((B, R), dtype=torch.float32, device=att.device)
        _lib().anchor_depth_backward(att, anchor, g.float().contiguous(), datt, danchor, B, P, R)
        return datt, danchor


def anchor_depth(att, anchor):
    """sum_r att[b,p,r] * anchor[b,r] (points_sample.py:277-279): att (B,P,R) softmax over the point channels, anchor (B,R) fp32
    -> (B,P) fp32; one streaming kernel each way instead of matrix-vector products in the batched-GEMM library."""
    return _AnchorDepthFn.apply(att, anchor)


class _PlaneLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, valid, tri, n_planes, min_area):
        lib = _lib()
        H, W = depth.shape[-2:]
        P = tri.shape[0]
        d = depth.reshape(H, W).contiguous()
        stats = torch.empty(4 * P + 1, dtype=torch.float64, device=d.device)
        loss = torch.empty(1, dtype=torch.float32, device=d.device)
        ws = torch.empty(lib.workspace_bytes(hip.WS_PLANE, P, H * W), dtype=torch.uint8, device=d.device)
        lib.plane_loss_forward(d, valid, tri, n_planes, P, H, W, int(min_area), ws, stats, loss)
        ctx.save_for_backward(d, valid, tri, n_planes, stats)
        ctx.shape = depth.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d, valid, tri, n_planes, stats = ctx.saved_tensors
        H, W = d.shape
        gd = torch.empty_like(d)
        _lib().plane_loss_backward(d, valid, tri, n_planes, tri.shape[0], H, W, stats, g.reshape(1).float().contiguous(), gd)
        return gd.view(ctx.shape), None, None, None, None


def plane_loss(depth, valid, tri, n_planes, min_area):
    """PlaneLoss of one image (glassrgbd.py:385-450): depth (1,1,H,W), valid (H,W) uint8, tri (P,6) int64 rounded / clamped
    vertices, n_planes device int32 (how many of the P triangles count).  Returns the scalar loss; gradient to depth."""
    return _PlaneLossFn.apply(depth, valid, tri, n_planes, int(min_area))


def inorm_gelu_residual(a, u, eps=1e-5):
    """a + gelu(instance_norm(u)): statistics over every dim but the first (image) and last (channel)."""
    return _InormGeluFn.apply(a, u, eps)


class _BroadcastRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, row, B, L, dtype):
        ctx.src = (row.shape, row.dtype)
        return row.reshape(1, 1, -1).to(dtype).expand(B, L, -1).contiguous()

    @staticmethod
    def backward(ctx, g):
        shape, dtype = ctx.src
        g = g.contiguous()
        C = g.shape[-1]
        out = torch.zeros(C, dtype=torch.float32, device=g.device)
        _lib().colsum(g, out, g.numel() // C, C)
        return out.to(dtype).reshape(shape), None, None, None


def broadcast_rows(row, B, L, dtype):
    """(.., C) parameter row -> materialised (B, L, C); the gradient is one column-sum kernel."""
    return _BroadcastRowsFn.apply(row, int(B), int(L), dtype)


class _PointSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap, coords, mode):
        fmap = fmap.contiguous()
        B, H, W, C = fmap.shape
        coords = coords.detach().reshape(B, -1, 2).float().contiguous()
        S = coords.shape[1]
        out = torch.empty((B, S, C), dtype=torch.float32, device=fmap.device)
        _lib().point_sample_forward(fmap, coords, out, B, H, W, C, S, mode)
        ctx.save_for_backward(coords)
        ctx.cfg = (B, H, W, C, S, mode, fmap.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        (coords,) = ctx.saved_tensors
        B, H, W, C, S, mode, dtype = ctx.cfg
        gmap = torch.empty((B, H, W, C), dtype=dtype, device=gout.device)
        g = gout.float().contiguous()
        if not _lib().point_sample_backward_gather(g, coords, gmap, B, H, W, C, S, mode):      # gather: every element written once
            gmap.zero_()
            _lib().point_sample_backward(g, coords, gmap, B, H, W, C, S, mode)
        return gmap, None, None


class _PointSampleFramedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap, coords, frame):
        fmap = fmap.contiguous()
        B, H, W, C = fmap.shape
        coords = coords.detach().reshape(B, -1, 2).float().contiguous()
        S = coords.shape[1]
        out = torch.empty((B, S, C), dtype=torch.float32, device=fmap.device)
        _lib().point_sample_framed_forward(fmap, coords, out, B, H, W, C, S, frame)
        ctx.save_for_backward(coords)
        ctx.cfg = (B, H, W, C, S, frame, fmap.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        (coords,) = ctx.saved_tensors
        B, H, W, C, S, frame, dtype = ctx.cfg
        gmap = torch.empty((B, H, W, C), dtype=dtype, device=gout.device)
        _lib().point_sample_framed_backward(gout.float().contiguous(), coords, gmap, B, H, W, C, S, frame)
        return gmap, None, None


def point_sample(fmap, coords, nearest=False, frame=None):
    """F.grid_sample(map, coords (B,S,1,2) or (B,S,2), align_corners=False, zeros padding) on a pixel-major map
    (B,H,W,C) -> fp32 (B,S,C); gradient to the map only.  frame = (Hf, Wf, shift), nearest only: the map as
    torch.roll(F.pad(map, to (Hf, Wf)), (-shift, -shift), (1, 2)) presents it (the shifted-window frame of the 1/32 stage), sampled in place."""
    if frame is not None:
        Hf, Wf, shift = (int(v) for v in frame)
        B, H, W, _ = fmap.shape
        if (Hf, Wf, shift) == (H, W, 0):
            frame = None
        elif not nearest:
            raise ValueError("point_sample: a frame needs nearest sampling")
        elif coords.numel() // (2 * B) <= 256:
            return _PointSampleFramedFn.apply(fmap, coords, (Hf, Wf, shift))
        else:                                               # more points than the gather backward stages: build the frame
            fmap = torch.nn.functional.pad(fmap, (0, 0, 0, Wf - W, 0, Hf - H))
            if shift:
                fmap = torch.roll(fmap, shifts=(-shift, -shift), dims=(1, 2))
    return _PointSampleFn.apply(fmap, coords, 1 if nearest else 0)


def dense_postprocess(depth, seg, sizes=None, min_depth=1e-3, max_depth=10.0, with_mm=True, out=None):
    """Inference post-processing of the dense outputs in one pass (gwd_dense_postprocess): depth (B,1,H,W) / (B,H,W) fp32 or
    bf16, seg (B,2,H,W) logits in any strides whose two pixel dims collapse (the model's pixel-major view qualifies), sizes
    (B,2) int32 = un-padded (h, w) or None.  -> (depth fp32 (B,H,W) clamped as engine_glassrgbd.py:249-252, depth_mm uint16
    or None, labels uint8); padding is 0 / 0 / 255.  out = the three tensors of an earlier call, to be overwritten."""
    if seg.dim() != 4 or seg.shape[1] != 2:
        raise ValueError("seg must be (B, 2, H, W) logits, got %s" % (tuple(seg.shape),))
    B, _, H, W = seg.shape
    if depth.numel() != B * H * W:
        raise ValueError("depth %s and seg %s differ" % (tuple(depth.shape), tuple(seg.shape)))
    depth = depth.reshape(B, H, W).contiguous()
    if H > 1 and seg.stride(2) != W * seg.stride(3):
        seg = seg.contiguous()
    if out is None:
        out = (torch.empty((B, H, W), dtype=torch.float32, device=depth.device),
               torch.empty((B, H, W), dtype=torch.uint16, device=depth.device) if with_mm else None,
               torch.empty((B, H, W), dtype=torch.uint8, device=depth.device))
    _lib().dense_postprocess(depth, seg, (seg.stride(0), seg.stride(3), seg.stride(1)), sizes, out[0], out[1], out[2], B, H, W,
                             min_depth, max_depth)
    return out


def dense_postprocess_resized(depth, seg, sizes, frame_sizes, out_hw, min_depth=1e-3, max_depth=10.0, twin=0, with_mm=True, out=None):
    """dense_postprocess at another size per image, in one pass (gwd_dense_postprocess_resized): the un-padded (h, w) region of
    image b (sizes (B,2) int32 on the device, None = all of H x W) is resized to frame_sizes[b] = (fh, fw) (device int32) by
    F.interpolate(mode="bilinear", align_corners=False)'s rule inside outputs of out_hw = (Fh, Fw) >= every frame; the rest is
    0 / 0 / 255.  twin > 0: depth / seg hold B + twin images and image b + twin is the prediction for the mirrored image b, which
    is mirrored back and averaged in (depth: mean of the clamped values; logits: sum).  H, W, Fh, Fw <= 16384.
    -> (depth fp32 (B,Fh,Fw), depth_mm uint16 or None, labels uint8); out = the three tensors of an earlier call."""
    if seg.dim() != 4 or seg.shape[1] != 2:
        raise ValueError("seg must be (B, 2, H, W) logits, got %s" % (tuple(seg.shape),))
    Bs, _, H, W = seg.shape
    twin = int(twin)
    B = Bs - twin
    if twin < 0 or B <= 0 or (twin and twin != B):
        raise ValueError("twin must be 0 or half of the %d source images, got %d" % (Bs, twin))
    if depth.numel() != Bs * H * W:
        raise ValueError("depth %s and seg %s differ" % (tuple(depth.shape), tuple(seg.shape)))
    Fh, Fw = (int(v) for v in out_hw)
    depth = depth.reshape(Bs, H, W).contiguous()
    if H > 1 and seg.stride(2) != W * seg.stride(3):
        seg = seg.contiguous()
    if out is None:
        out = (torch.empty((B, Fh, Fw), dtype=torch.float32, device=depth.device),
               torch.empty((B, Fh, Fw), dtype=torch.uint16, device=depth.device) if with_mm else None,
               torch.empty((B, Fh, Fw), dtype=torch.uint8, device=depth.device))
    _lib().dense_postprocess_resized(depth, seg, (seg.stride(0), seg.stride(3), seg.stride(1)), sizes, frame_sizes, twin, out[0], out[1],
                                     out[2], B, H, W, Fh, Fw, min_depth, max_depth)
    return out


def line_postprocess(logits, lines, sizes, thresh=0.6):
    """PostProcess_Line 'prediction' for two classes plus a ranking (gwd_line_postprocess): logits (B,Q,2), lines (B,Q,4|6),
    sizes (B,2) int32 (h, w) -> scores (B,Q), lines in pixels (B,Q,4), order (B,Q) int32 (score descending, equal scores by
    lower index), count (B,) int32 (scores > thresh)."""
    B, Q, ld = lines.shape
    logits, lines = logits.float().contiguous(), lines.float().contiguous()
    dev = logits.device
    scores = torch.empty((B, Q), dtype=torch.float32, device=dev)
    lines_px = torch.empty((B, Q, 4), dtype=torch.float32, device=dev)
    order = torch.empty((B, Q), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib().line_postprocess(logits, lines, sizes, scores, lines_px, order, count, B, Q, ld, thresh)
    return scores, lines_px, order, count


def line_nms(logits, lines, sizes, threshold, order=None, min_score=None, twin=0):
    """L-CNN's line NMS over the queries of every image (gwd_line_nms; the reference's postprocess at tol = 0, do_clip = False):
    logits (B+twin,Q,2), lines (B+twin,Q,4|6), sizes (B,2) int32 (h, w) the lines are scaled to, threshold a fraction of that
    size's diagonal (the reference uses 0.010 and 0.015).  order None: the queries are taken in query order, as the reference
    takes them; order (B+twin,Q) int32: in that order (line_postprocess's `order`: score descending).  min_score: only queries
    with score > min_score take part.  twin = B: image b + B is the prediction for the mirrored image b, and its queries, mirrored
    back, are candidates of image b too (appended in query order, merged by score under an order).
    -> nms_lines (B,C,4) float64 (x1, y1, x2, y2) pixels, nms_scores (B,C), nms_ids (B,C) int32 (query index, + Q for the twin's),
    nms_count (B,) int32, with C = Q or 2 Q: row r of an image is its r-th kept line, rows from nms_count on hold 0 / 0 / -1."""
    Bs, Q, ld = lines.shape
    twin = int(twin)
    B = Bs - twin
    if twin < 0 or B <= 0 or (twin and twin != B):
        raise ValueError("twin must be 0 or half of the %d images, got %d" % (Bs, twin))
    logits, lines = logits.float().contiguous(), lines.float().contiguous()
    if order is not None:
        order = order.contiguous()
    dev, C = logits.device, Q * (2 if twin else 1)
    nms_lines = torch.empty((B, C, 4), dtype=torch.float64, device=dev)
    nms_scores = torch.empty((B, C), dtype=torch.float32, device=dev)
    nms_ids = torch.empty((B, C), dtype=torch.int32, device=dev)
    nms_count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib().line_nms(logits, lines, sizes, order, threshold, min_score, nms_lines, nms_scores, nms_ids, nms_count, twin)
    return nms_lines, nms_scores, nms_ids, nms_count


REGION_KEYS = ("region_map", "region_count", "region_total", "regions", "planes", "depth_planar", "depth_planar_mm")
REGION_FIELDS = ("area", "x0", "y0", "x1", "y1", "anchor", "sum_x", "sum_y", "n_depth", "sum_mm", "min_mm", "max_mm")


def region_keys(planes=True, planar=True):
    """The keys glass_regions returns for these switches."""
    return REGION_KEYS[:4] + (("planes",) if planes or planar else ()) + (REGION_KEYS[5:] if planar else ())


def region_mm_range(min_depth, max_depth):
    """The millimetres lo .. hi (inclusive) that lie in [min_depth, max_depth] metres: a region's pixels `with depth`."""
    lo = max(1, -int(-(float(min_depth) * 1000.0 - 1e-6) // 1))
    hi = min(65535, int((float(max_depth) * 1000.0 + 1e-6) // 1))
    return lo, hi


def check_region_options(max_regions=32, min_area=100, connectivity=8, min_depth=1e-3, max_depth=10.0, planes=True, planar=True,
                         max_candidates=None):
    """Host validation of glass_regions' options (also what InferenceSession(regions=...) accepts); -> them as a dict."""
    if connectivity not in (4, 8):
        raise ValueError("glass_regions: connectivity must be 4 or 8, got %r" % (connectivity,))
    if not 1 <= int(max_regions) <= hip.REGION_MAX:
        raise ValueError("glass_regions: 1 <= max_regions <= %d, got %r" % (hip.REGION_MAX, max_regions))
    if int(min_area) < 1:
        raise ValueError("glass_regions: min_area >= 1, got %r" % (min_area,))
    max_candidates = hip.REGION_CANDIDATES if max_candidates is None else int(max_candidates)
    if not 1 <= max_candidates <= 1 << 24:
        raise ValueError("glass_regions: 1 <= max_candidates <= 2^24, got %r" % (max_candidates,))
    if not 0.0 < float(min_depth) < float(max_depth):
        raise ValueError("glass_regions: 0 < min_depth < max_depth, got %r, %r" % (min_depth, max_depth))
    lo, hi = region_mm_range(min_depth, max_depth)
    if lo > hi:
        raise ValueError("glass_regions: no whole millimetre lies in [%r, %r] metres" % (min_depth, max_depth))
    return dict(max_regions=int(max_regions), min_area=int(min_area), connectivity=int(connectivity), min_depth=float(min_depth),
                max_depth=float(max_depth), planes=bool(planes), planar=bool(planar), max_candidates=max_candidates)


def glass_regions(labels, depth_mm, sizes, max_regions=32, min_area=100, connectivity=8, min_depth=1e-3, max_depth=10.0, planes=True,
                  planar=True, max_candidates=None, depth=None):
    """From pixels to objects, on the device (gwd_glass_regions / gwd_region_planes / gwd_depth_planar):
    labels (B,Fh,Fw) uint8 (1 = glass), depth_mm (B,Fh,Fw) uint16, sizes (B,2) int32 (fh, fw) on the device - what
    InferenceSession.predict_frames returns; B <= 16, sides <= 16384.  A pixel outside its frame never takes part.

    -> dict: region_map (B,Fh,Fw) uint8 (0 = in no kept region, r + 1 = rank r), region_count (B,) int32 (-1: more than
    max_candidates components of min_area pixels or more, the image is refused), region_total (B,) int32 (components before
    min_area), regions (B,max_regions,12) int64 in REGION_FIELDS order, rows from region_count on 0.  The kept regions are the
    max_regions largest components (4- or 8-connected) of area >= min_area, ranked by (area descending, anchor ascending), anchor =
    the smallest raster index y * fw + x of the component.  n_depth / sum_mm / min_mm / max_mm run over the pixels whose
    millimetres lie in [min_depth, max_depth] metres.
    planes=True: planes (B,max_regions,6) float64 = alpha, beta, gamma, rms, n_used, status: the least-squares plane
    w = alpha x + beta y + gamma in inverse depth w = 1000 / depth_mm (1 / m) over those pixels; status 1 (NaN coefficients) for
    fewer than 3 or collinear pixels.  With pinhole intrinsics (fx, fy, cx, cy) the 3-D plane n . P = d follows in closed form:
    with m = (alpha fx, beta fy, gamma + alpha cx + beta cy), n = m / |m| and d = 1 / |m| (a point (X, Y, Z) projects to
    x = fx X / Z + cx, y = fy Y / Z + cy, so n . P = d divided by d Z is affine in (x, y, 1 / Z)).
    planar=True (implies the fit): depth_planar (B,Fh,Fw) float32 and depth_planar_mm uint16 = `depth` (float32, default
    depth_mm / 1000) and depth_mm with every pixel of a fitted region where alpha x + beta y + gamma > 0 rewritten to
    clamp(1 / (alpha x + beta y + gamma), min_depth, max_depth); outside the frames 0 / 0.
    Fresh tensors, no host sync; repeated calls give bit-identical results."""
    opt = check_region_options(max_regions, min_area, connectivity, min_depth, max_depth, planes, planar, max_candidates)
    for name, t, dt in (("labels", labels, torch.uint8), ("depth_mm", depth_mm, torch.uint16), ("sizes", sizes, torch.int32),
                        ("depth", depth, torch.float32)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt):
            raise TypeError("glass_regions: %s must be a %s tensor" % (name, dt))
    if labels.dim() != 3 or 0 in labels.shape:
        raise ValueError("glass_regions: labels must be (B, Fh, Fw), got %s" % (tuple(labels.shape),))
    B, Fh, Fw = labels.shape
    if B > hip.AUGMENT_BATCH or max(Fh, Fw) > 16384:
        raise ValueError("glass_regions: at most %d frames of at most 16384 per side, got %s" % (hip.AUGMENT_BATCH, tuple(labels.shape)))
    if tuple(depth_mm.shape) != (B, Fh, Fw) or tuple(sizes.shape) != (B, 2) or (depth is not None and tuple(depth.shape) != (B, Fh, Fw)):
        raise ValueError("glass_regions: depth_mm / depth must be %s and sizes (%d, 2)" % ((B, Fh, Fw), B))
    lib, dev, R = _lib(), labels.device, opt["max_regions"]
    labels, depth_mm, sizes = labels.contiguous(), depth_mm.contiguous(), sizes.contiguous()
    lo, hi = region_mm_range(opt["min_depth"], opt["max_depth"])
    ws = torch.empty(lib.workspace_bytes(hip.WS_REGIONS, B, Fh, Fw, opt["max_candidates"]), dtype=torch.uint8, device=dev)
    res = {"region_map": torch.empty((B, Fh, Fw), dtype=torch.uint8, device=dev),
           "region_count": torch.empty((B,), dtype=torch.int32, device=dev),
           "region_total": torch.empty((B,), dtype=torch.int32, device=dev),
           "regions": torch.empty((B, R, hip.REGION_RECORD), dtype=torch.int64, device=dev)}
    lib.glass_regions(labels, depth_mm, sizes, R, opt["min_area"], opt["connectivity"], opt["max_candidates"], lo, hi, ws,
                      res["region_map"], res["region_count"], res["region_total"], res["regions"])
    if opt["planes"] or opt["planar"]:
        res["planes"] = torch.empty((B, R, 6), dtype=torch.float64, device=dev)
        lib.region_planes(res["region_map"], depth_mm, sizes, res["region_count"], res["regions"], lo, hi, ws, res["planes"])
    if opt["planar"]:
        res["depth_planar"] = torch.empty((B, Fh, Fw), dtype=torch.float32, device=dev)
        res["depth_planar_mm"] = torch.empty((B, Fh, Fw), dtype=torch.uint16, device=dev)
        lib.depth_planar(res["region_map"], depth_mm, None if depth is None else depth.contiguous(), sizes, res["region_count"],
                         res["planes"], opt["min_depth"], opt["max_depth"], res["depth_planar"], res["depth_planar_mm"])
    return res


FUSION_KEYS = ("depth_fused", "depth_fused_mm", "fused_source", "fusion_ring", "fusion_planes", "fusion_scale")
FUSION_PLANE_FIELDS = ("alpha1", "beta1", "gamma1", "rms1", "n1", "alpha", "beta", "gamma", "rms", "n_used", "status", "spare")
FUSION_SCALE_FIELDS = ("scale", "n", "sum_sp", "sum_pp")
FUSED_SOURCES = {"sensor": hip.FUSED_SENSOR, "plane": hip.FUSED_PLANE, "network": hip.FUSED_NETWORK}


def fusion_keys():
    """The keys sensor_fusion returns."""
    return FUSION_KEYS


def _whole(name, v, what="sensor_fusion"):
    if isinstance(v, bool) or int(v) != v:
        raise TypeError("%s: %s must be a whole number, got %r" % (what, name, v))
    return int(v)


def check_fusion_options(ring=6, gap=1, trim=2.5, min_ring=50, max_rms=None, align=True, min_align=1000, min_depth=1e-3, max_depth=10.0):
    """Host validation of sensor_fusion's options (also what InferenceSession(fusion=...) accepts); -> them as a dict."""
    ring, gap = _whole("ring", ring), _whole("gap", gap)
    min_ring, min_align = _whole("min_ring", min_ring), _whole("min_align", min_align)
    if not isinstance(align, bool):
        raise TypeError("sensor_fusion: align must be True or False, got %r" % (align,))
    if not 1 <= ring <= hip.FUSION_MAX_RING:
        raise ValueError("sensor_fusion: 1 <= ring <= %d, got %r" % (hip.FUSION_MAX_RING, ring))
    if not 0 <= gap < ring:
        raise ValueError("sensor_fusion: 0 <= gap <= ring - 1, got gap %r with ring %r" % (gap, ring))
    if not 0.0 <= float(trim) < float("inf"):
        raise ValueError("sensor_fusion: trim >= 0 (0 = no second fit), got %r" % (trim,))
    if not 0 <= min_ring < 1 << 31:
        raise ValueError("sensor_fusion: min_ring >= 0, got %r" % (min_ring,))
    if max_rms is not None and not float(max_rms) >= 0.0:
        raise ValueError("sensor_fusion: max_rms must be None or >= 0 (1 / m), got %r" % (max_rms,))
    if not 0 <= min_align < 1 << 31:
        raise ValueError("sensor_fusion: min_align >= 0, got %r" % (min_align,))
    if not 0.0 < float(min_depth) < float(max_depth):
        raise ValueError("sensor_fusion: 0 < min_depth < max_depth, got %r, %r" % (min_depth, max_depth))
    lo, hi = region_mm_range(min_depth, max_depth)
    if lo > hi:
        raise ValueError("sensor_fusion: no whole millimetre lies in [%r, %r] metres" % (min_depth, max_depth))
    return dict(ring=ring, gap=gap, trim=float(trim), min_ring=min_ring, max_rms=None if max_rms is None else float(max_rms),
                align=align, min_align=min_align, min_depth=float(min_depth), max_depth=float(max_depth))


def sensor_fusion(sensor_mm, labels, depth, depth_mm, sizes, region_map, region_count, regions, ring=6, gap=1, trim=2.5, min_ring=50,
                  max_rms=None, align=True, min_align=1000, min_depth=1e-3, max_depth=10.0):
    """An RGB-D camera's depth plane, corrected where there is glass, on the device (gwd_fusion_ring / gwd_fusion_planes /
    gwd_fusion_depth).  sensor_mm (B,Fh,Fw) uint16 millimetres, 0 = no reading, registered to the frame;
    labels uint8, depth float32, depth_mm uint16, sizes (B,2) int32 - what InferenceSession.predict_frames returns - and region_map
    uint8, region_count (B,) int32, regions (B,R,12) int64 of glass_regions for the same frames.  B <= 16, sides <= 16384.  A value
    is valid when its millimetres lie in region_mm_range(min_depth, max_depth); a pixel outside its frame never takes part.

    -> dict in FUSION_KEYS order:
    depth_fused (B,Fh,Fw) float32, depth_fused_mm uint16, fused_source uint8 - per pixel the first that applies: 1 (sensor) not
    glass and a valid reading: the reading; 2 (plane) a pixel of a kept region whose frame plane has status 0 and
    alpha x + beta y + gamma > 0: clamp(1 / that, min_depth, max_depth); 3 (network) the rest - glass without a usable plane, holes
    of the sensor: clamp(depth * scale); outside the frames 0 / 0 / 0.
    fusion_ring (B,Fh,Fw) uint8: r + 1 on the ring of rank r - not glass, a valid reading, no glass pixel within Chebyshev distance
    `gap`, a pixel of a kept region within `ring` (the smallest such rank) - else 0.
    fusion_planes (B,R,12) float64 in FUSION_PLANE_FIELDS order: the least-squares plane in inverse depth 1000 / sensor_mm over a
    region's ring pixels (glass_regions' method), first over all of them, then - trim > 0 - over those within trim * rms1 of the
    first; status 0 usable, 1 fewer than 3 or collinear samples (NaN), 2 rejected: n_used < min_ring or rms > max_rms (1 / m).
    fusion_scale (B,4) float64 in FUSION_SCALE_FIELDS order: scale = sum sensor_mm * depth_mm / sum depth_mm^2 over the n pixels
    that are not glass, have no glass within `gap` and both values valid (exact integers); 1.0 when n < min_align or align=False.
    Fresh tensors, no host sync; repeated calls give bit-identical results."""
    opt = check_fusion_options(ring, gap, trim, min_ring, max_rms, align, min_align, min_depth, max_depth)
    for name, t, dt in (("sensor_mm", sensor_mm, torch.uint16), ("labels", labels, torch.uint8), ("depth", depth, torch.float32),
                        ("depth_mm", depth_mm, torch.uint16), ("sizes", sizes, torch.int32), ("region_map", region_map, torch.uint8),
                        ("region_count", region_count, torch.int32), ("regions", regions, torch.int64)):
        if not torch.is_tensor(t) or t.dtype != dt:
            raise TypeError("sensor_fusion: %s must be a %s tensor" % (name, dt))
    if labels.dim() != 3 or 0 in labels.shape:
        raise ValueError("sensor_fusion: labels must be (B, Fh, Fw), got %s" % (tuple(labels.shape),))
    B, Fh, Fw = labels.shape
    if B > hip.AUGMENT_BATCH or max(Fh, Fw) > 16384:
        raise ValueError("sensor_fusion: at most %d frames of at most 16384 per side, got %s" % (hip.AUGMENT_BATCH, tuple(labels.shape)))
    for name, t in (("sensor_mm", sensor_mm), ("depth", depth), ("depth_mm", depth_mm), ("region_map", region_map)):
        if tuple(t.shape) != (B, Fh, Fw):
            raise ValueError("sensor_fusion: %s must be %s like labels, got %s" % (name, (B, Fh, Fw), tuple(t.shape)))
    if tuple(sizes.shape) != (B, 2) or tuple(region_count.shape) != (B,):
        raise ValueError("sensor_fusion: sizes must be (%d, 2) and region_count (%d,)" % (B, B))
    if regions.dim() != 3 or regions.shape[0] != B or regions.shape[2] != hip.REGION_RECORD or not 1 <= regions.shape[1] <= hip.REGION_MAX:
        raise ValueError("sensor_fusion: regions must be (%d, 1..%d, %d), got %s" % (B, hip.REGION_MAX, hip.REGION_RECORD, tuple(regions.shape)))
    lib, dev, R = _lib(), labels.device, regions.shape[1]
    sensor_mm, labels, depth, depth_mm, sizes, region_map, region_count, regions = (
        t.contiguous() for t in (sensor_mm, labels, depth, depth_mm, sizes, region_map, region_count, regions))
    lo, hi = region_mm_range(opt["min_depth"], opt["max_depth"])
    ws = torch.empty(lib.workspace_bytes(hip.WS_FUSION, B, Fh, Fw), dtype=torch.uint8, device=dev)
    res = {"depth_fused": torch.empty((B, Fh, Fw), dtype=torch.float32, device=dev),
           "depth_fused_mm": torch.empty((B, Fh, Fw), dtype=torch.uint16, device=dev),
           "fused_source": torch.empty((B, Fh, Fw), dtype=torch.uint8, device=dev),
           "fusion_ring": torch.empty((B, Fh, Fw), dtype=torch.uint8, device=dev),
           "fusion_planes": torch.empty((B, R, hip.FUSION_PLANE), dtype=torch.float64, device=dev),
           "fusion_scale": torch.empty((B, 4), dtype=torch.float64, device=dev)}
    lib.fusion_ring(labels, sensor_mm, depth_mm, sizes, region_map, region_count, R, opt["ring"], opt["gap"], lo, hi, opt["align"],
                    opt["min_align"], ws, res["fusion_ring"], res["fusion_scale"])
    lib.fusion_planes(res["fusion_ring"], sensor_mm, sizes, region_count, regions, opt["ring"], lo, hi, opt["trim"], opt["min_ring"],
                      opt["max_rms"], ws, res["fusion_planes"])
    lib.fusion_depth(labels, sensor_mm, depth, sizes, region_map, region_count, res["fusion_planes"], res["fusion_scale"], lo, hi,
                     opt["min_depth"], opt["max_depth"], res["depth_fused"], res["depth_fused_mm"], res["fused_source"])
    return res


PROFILE_KEYS = ("profile_counts", "profile_fits", "profile_kind", "line_points")
PROFILE_COUNT_FIELDS = ("samples", "on_in", "on_glass", "on_depth", "a_in", "a_glass", "a_depth", "b_in", "b_glass", "b_depth",
                        "region_a", "region_b")
PROFILE_FIT_FIELDS = ("w0", "w1", "rms", "n_used", "status")
PROFILE_PROBES = ("on", "a", "b")


def profile_keys(intrinsics=False):
    """The keys line_profiles returns without / with intrinsics."""
    return PROFILE_KEYS if intrinsics else PROFILE_KEYS[:3]


def check_line_profile_options(offset=3.0, max_samples=2048, min_depth=1e-3, max_depth=10.0, hi=700, lo=300):
    """Host validation of line_profiles' options (also what InferenceSession(line_profiles=...) accepts); -> them as a dict."""
    if not 0.0 < float(offset) <= 16384.0:
        raise ValueError("line_profiles: 0 < offset <= 16384 pixels, got %r" % (offset,))
    if int(max_samples) != max_samples or not 2 <= int(max_samples) <= hip.PROFILE_MAX_SAMPLES:
        raise ValueError("line_profiles: 2 <= max_samples <= %d, got %r" % (hip.PROFILE_MAX_SAMPLES, max_samples))
    if int(hi) != hi or int(lo) != lo or not 0 <= int(lo) < int(hi) <= 1000:
        raise ValueError("line_profiles: 0 <= lo < hi <= 1000 per mille, got lo %r, hi %r" % (lo, hi))
    if not 0.0 < float(min_depth) < float(max_depth):
        raise ValueError("line_profiles: 0 < min_depth < max_depth, got %r, %r" % (min_depth, max_depth))
    lo_mm, hi_mm = region_mm_range(min_depth, max_depth)
    if lo_mm > hi_mm:
        raise ValueError("line_profiles: no whole millimetre lies in [%r, %r] metres" % (min_depth, max_depth))
    return dict(offset=float(offset), max_samples=int(max_samples), min_depth=float(min_depth), max_depth=float(max_depth),
                hi=int(hi), lo=int(lo))


def line_profiles(lines, count, labels, depth_mm, sizes, order=None, region_map=None, intrinsics=None, offset=3.0, max_samples=2048,
                  min_depth=1e-3, max_depth=10.0, hi=700, lo=300):
    """Every detected line walked through the dense results, on the device, in one launch (gwd_line_profiles):
    lines (B,C,4) float64 or float32 (x1, y1, x2, y2) frame pixels and count (B,) int32 - nms_lines / nms_count, or lines / count
    with order (B,C) int32 (row r reads lines[b, order[b, r]]) - and labels uint8 / depth_mm uint16 (B,Fh,Fw), sizes (B,2) int32 of
    the same frames; region_map: glass_regions' map; intrinsics (B,4) float64 (fx, fy, cx, cy) at frame size.  B <= 16, sides <=
    16384, C <= 2048.

    A line of squared length L2 gets S = n + 1 samples at t = k / n, n = ceil(sqrt(L2)) (at most max_samples - 1), and every sample
    three probes: on the line, and `offset` pixels to either side of it - a = on + offset (-dy, dx) / L, b = on - the same.  A probe
    reads the pixel (floor x, floor y) of its own frame.
    -> dict: profile_counts (B,C,12) int32 in PROFILE_COUNT_FIELDS order (per probe: in the frame, glass, with depth in
    [min_depth, max_depth]; region_a / region_b: the rank of region_map most samples of that side lie in, -1 for none),
    profile_fits (B,C,3,5) float64 per probe in PROFILE_FIT_FIELDS order: the least-squares fit of inverse depth 1000 / mm (1 / m),
    affine in t - which is the 3-D line, 1 / Z being affine along the image of a segment - at t = 0 and t = 1, the rms of its
    residual, the samples used and a status (0 fitted, 1 fewer than 2 samples with depth, 2 degenerate line, 3 a row from count on),
    profile_kind (B,C) int32: 1 / 2 glass on side a / b only (at least hi per mille glass on one side, at most lo on the other),
    3 both, 4 neither, 0 undecided; with intrinsics line_points (B,C,2,3) float64, the two ends in camera coordinates (NaN without
    a fit).  Rows from count on hold 0, regions -1, status 3.  Fresh tensors, no host sync; repeated calls are bit-identical."""
    opt = check_line_profile_options(offset, max_samples, min_depth, max_depth, hi, lo)
    if not torch.is_tensor(lines) or lines.dtype not in (torch.float32, torch.float64):
        raise TypeError("line_profiles: lines must be a float32 or float64 tensor")
    for name, t, dt in (("count", count, torch.int32), ("labels", labels, torch.uint8), ("depth_mm", depth_mm, torch.uint16),
                        ("sizes", sizes, torch.int32), ("order", order, torch.int32), ("region_map", region_map, torch.uint8),
                        ("intrinsics", intrinsics, torch.float64)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt):
            raise TypeError("line_profiles: %s must be a %s tensor" % (name, dt))
    if labels.dim() != 3 or 0 in labels.shape or lines.dim() != 3 or lines.shape[2] != 4 or lines.shape[1] == 0:
        raise ValueError("line_profiles: labels must be (B, Fh, Fw) and lines (B, C, 4), got %s, %s" % (tuple(labels.shape), tuple(lines.shape)))
    B, Fh, Fw = labels.shape
    C = lines.shape[1]
    if B > hip.AUGMENT_BATCH or max(Fh, Fw) > 16384 or C > hip.PROFILE_MAX_LINES:
        raise ValueError("line_profiles: at most %d frames of at most 16384 per side and %d lines each, got %s, %s"
                         % (hip.AUGMENT_BATCH, hip.PROFILE_MAX_LINES, tuple(labels.shape), tuple(lines.shape)))
    if lines.shape[0] != B or tuple(count.shape) != (B,) or tuple(depth_mm.shape) != (B, Fh, Fw) or tuple(sizes.shape) != (B, 2) \
            or (order is not None and tuple(order.shape) != (B, C)) or (region_map is not None and tuple(region_map.shape) != (B, Fh, Fw)) \
            or (intrinsics is not None and tuple(intrinsics.shape) != (B, 4)):
        raise ValueError("line_profiles: operands do not fit (B, C, Fh, Fw) = %s" % ((B, C, Fh, Fw),))
    dev = labels.device
    c = lambda t: None if t is None else t.contiguous()
    lo_mm, hi_mm = region_mm_range(opt["min_depth"], opt["max_depth"])
    res = {"profile_counts": torch.empty((B, C, hip.PROFILE_COUNTS), dtype=torch.int32, device=dev),
           "profile_fits": torch.empty((B, C, 3, 5), dtype=torch.float64, device=dev),
           "profile_kind": torch.empty((B, C), dtype=torch.int32, device=dev)}
    if intrinsics is not None:
        res["line_points"] = torch.empty((B, C, 2, 3), dtype=torch.float64, device=dev)
    _lib().line_profiles(c(lines), c(count), c(order), c(labels), c(depth_mm), c(sizes), c(region_map), c(intrinsics), opt["offset"],
                         opt["max_samples"], lo_mm, hi_mm, opt["hi"], opt["lo"], res["profile_counts"], res["profile_fits"],
                         res["profile_kind"], res.get("line_points"))
    return res


# ---------------------------------------------------------------------------------------------------------------------- rendering
RENDER_KEYS = ("canvas",)
_RENDER_TABLES = {}            # (device, the tables' bytes) -> the tables on the device: the defaults are uploaded once


def _render_tables(tables, device):
    key = (str(device), tables.tobytes())
    t = _RENDER_TABLES.get(key)
    if t is None:
        if len(_RENDER_TABLES) >= 32:
            _RENDER_TABLES.clear()
        t = _RENDER_TABLES[key] = torch.from_numpy(tables).to(device)
    return t


def _render_views(value, B, name, what="render_frames"):
    """One (B, h, w[, 3]) tensor or B separate views -> a list of B views (no copy)."""
    if value is None:
        return None
    if torch.is_tensor(value):
        if value.shape[0] != B:
            raise ValueError("%s: %s holds %d frames, sizes %d" % (what, name, value.shape[0], B))
        return [value[b] for b in range(B)]
    if not isinstance(value, (list, tuple)) or len(value) != B or not all(torch.is_tensor(t) for t in value):
        raise ValueError("%s: %s is one tensor or a list of %d tensors" % (what, name, B))
    return list(value)


def render_frames(sizes, panels, frames=None, planes=None, label_planes=None, region_map=None, lines=None, count=None, order=None,
                  scores=None, kinds=None, out=None, **options):
    """uint8 RGB panels of predict_frames' results at frame size, on the device, in ONE launch (gwd_render_frames, DESIGN.md section
    27).  sizes (B,2) int32 (fh, fw) on the device; panels: 1..8 dicts (render.PANEL_KEYS; a bare base stands for {"base": base}):
      base           "black", "frame", ("depth", i): planes[i] (uint16 millimetres) through `table` ((256,3) uint8, default
                     matplotlib's jet) over `range` = (lo_mm, hi_mm) (default 0 .. 8500), 0 mm: `void`; ("labels", i):
                     label_planes[i] (uint8) through `table` (default the PASCAL-VOC palette, 255 black);
      tint           the index of a label plane: where it is 1 the pixel moves `tint_alpha` / 256 of the way to `tint_color`;
      outlines       True: the outline pixels of region_map's regions in `region_colors`;
      lines          "score" (`score_table` over the call's score_range), "kind" (`kind_colors` by kinds) or an (r, g, b);
      ends           discs at both ends of every drawn row (default: with lines) in `end_color`.
    frames: B uint8 (h,w,3) tensors; planes / label_planes: a plane or a list of planes, each ONE (B,h,w) tensor or B separate
    (h,w) views (unit column stride, any row pitch: nothing is copied); region_map likewise.  lines (B,C,4) float32 / float64
    frame pixels with count (B,) int32, and order (B,C) int32, scores (B,C) (both indexed as ops.line_profiles takes them: row r
    reads lines[b, order[b, r]] and that row's score), kinds (B,C) int32 = profile_kind (indexed by the row r itself).
    options (render.RENDER_OPTIONS): width=2.0 pixels (<= 16), end_radius=2 pixels (0: none), min_score (rows below it, or with a NaN
    score, are not drawn), score_range=(0.92, 1.02), canvas_size=(Fh, Fw) (default: the largest operand).
    -> canvas (B, P, Fh, Fw, 3) uint8, a fresh tensor (or `out`, a contiguous uint8 tensor of that shape on the device) every byte
    of which the launch wrote; a pixel outside its frame is 0.  A frame is clipped to what its operands cover.  No host sync; repeated calls are bit-identical."""
    from . import render as R
    if set(options) - set(R.RENDER_OPTIONS):
        raise TypeError("render_frames: unknown option(s) %s (known: %s)" % (sorted(set(options) - set(R.RENDER_OPTIONS)), ", ".join(R.RENDER_OPTIONS)))
    opts = R.check_options(**options)
    if not torch.is_tensor(sizes) or sizes.dtype != torch.int32 or sizes.dim() != 2 or sizes.shape[1] != 2:
        raise TypeError("render_frames: sizes must be a (B, 2) int32 tensor")
    B = sizes.shape[0]
    if not 1 <= B <= hip.AUGMENT_BATCH:
        raise ValueError("render_frames: 1..%d frames per call, got %d" % (hip.AUGMENT_BATCH, B))

    def plane_list(value, name):
        if value is None:
            return []
        if torch.is_tensor(value) or (isinstance(value, (list, tuple)) and len(value) and torch.is_tensor(value[0]) and value[0].dim() == 2):
            value = [value]                               # one plane: a (B,h,w) tensor, or B views
        if len(value) > hip.RENDER_MAX_PLANES:
            raise ValueError("render_frames: at most %d %s, got %d" % (hip.RENDER_MAX_PLANES, name, len(value)))
        return [_render_views(v, B, "%s[%d]" % (name, i)) for i, v in enumerate(value)]

    frames = _render_views(frames, B, "frames")
    if frames is not None:                                # a frame is read where it lies when its pixels are dense, whatever its row pitch
        frames = [f if f.dim() != 3 or (f.stride(2) == 1 and f.stride(1) == 3) else f.contiguous() for f in frames]
    region_map = _render_views(region_map, B, "region_map")
    planes, label_planes = plane_list(planes, "planes"), plane_list(label_planes, "label_planes")
    for views, dt, name in [(frames, torch.uint8, "frames"), (region_map, torch.uint8, "region_map")] + \
            [(v, torch.uint16, "planes") for v in planes] + [(v, torch.uint8, "label_planes") for v in label_planes]:
        if views is not None and any(t.dtype != dt for t in views):
            raise TypeError("render_frames: %s must be %s" % (name, dt))
    for t, name, dts in ((lines, "lines", (torch.float32, torch.float64)), (count, "count", (torch.int32,)), (order, "order", (torch.int32,)),
                         (scores, "scores", (torch.float32, torch.float64)), (kinds, "kinds", (torch.int32,))):
        if t is not None and (not torch.is_tensor(t) or t.dtype not in dts):
            raise TypeError("render_frames: %s must be a %s tensor" % (name, " or ".join(str(d) for d in dts)))
    tables, recs = R.resolve(panels, len(planes), len(label_planes), frames is not None, region_map is not None, lines is not None,
                             scores is not None, kinds is not None)
    every = (frames or []) + (region_map or []) + [t for views in planes + label_planes for t in views]
    Fh, Fw = opts["canvas_size"] or (max([t.shape[0] for t in every] + [1]), max([t.shape[1] for t in every] + [1]))
    if max(Fh, Fw) > 16384:
        raise ValueError("render_frames: sides are limited to 16384, got %s" % ((Fh, Fw),))
    dev = sizes.device
    c = lambda t: None if t is None else t.contiguous()
    shape = (B, len(recs), Fh, Fw, 3)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != dev
                            or not out.is_contiguous()):
        raise ValueError("render_frames: out must be a contiguous uint8 %s tensor on %s" % (shape, dev))
    canvas = torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else out
    _lib().render_frames(canvas, c(sizes), _render_tables(tables, dev), recs, frames, planes, label_planes, region_map, c(lines), c(count),
                         c(order), c(scores), c(kinds), opts)
    return canvas


# ---------------------------------------------------------------------------------------------------------------------- point clouds
CLOUD_KEYS = ("cloud", "cloud_offsets")
CLOUD_FLAGS = {"point": 1, "normal": 2, "pane_normal": 4, "colour": 8}


def check_cloud_options(stride=1, min_depth=1e-3, max_depth=10.0, edge=None, normals=True, keep="all"):
    """Host validation of point_cloud's options (also what InferenceSession(cloud=...) accepts, next to `depth`); -> them as a dict."""
    stride = _whole("stride", stride, "point_cloud")
    if not 1 <= stride <= hip.CLOUD_MAX_STRIDE:
        raise ValueError("point_cloud: 1 <= stride <= %d, got %r" % (hip.CLOUD_MAX_STRIDE, stride))
    if not 0.0 < float(min_depth) < float(max_depth) < float("inf"):
        raise ValueError("point_cloud: 0 < min_depth < max_depth, got %r, %r" % (min_depth, max_depth))
    if edge is not None and not 0.0 < float(edge) < float("inf"):
        raise ValueError("point_cloud: edge must be None or a relative depth jump > 0, got %r" % (edge,))
    if not isinstance(normals, bool):
        raise TypeError("point_cloud: normals must be True or False, got %r" % (normals,))
    if keep not in hip.CLOUD_KEEP:
        raise ValueError("point_cloud: keep must be one of %s, got %r" % (", ".join(repr(k) for k in hip.CLOUD_KEEP), keep))
    return dict(stride=stride, min_depth=float(min_depth), max_depth=float(max_depth), edge=None if edge is None else float(edge),
                normals=normals, keep=keep)


def cloud_capacity(B, Fh, Fw, stride=1, frame_sizes=None):
    """The rows a cloud needs at most: B planes of the stride lattice, or exactly that of frame_sizes ((fh, fw) pairs) when given."""
    if frame_sizes is None:
        frame_sizes = [(Fh, Fw)] * B
    return sum(-(-min(int(h), Fh) // stride) * -(-min(int(w), Fw) // stride) for h, w in frame_sizes)


def point_cloud(depth, labels, sizes, intrinsics, frames=None, region_map=None, region_count=None, planes=None, source=None, poses=None,
                stride=1, min_depth=1e-3, max_depth=10.0, edge=None, normals=True, keep="all", capacity=None, frame_sizes=None):
    """The scene in 3-D, on the device (gwd_point_cloud; tests/cloud_ref.py is the statement): depth (B,Fh,Fw)
    float32 metres, labels uint8, sizes (B,2) int32 (fh, fw) on the device - what InferenceSession.predict_frames returns (depth may
    as well be depth_planar or depth_fused) - and intrinsics (B,4) float64 (fx, fy, cx, cy) at frame size.  B <= 16, sides <= 16384.
    frames: B uint8 (h,w,3) tensors as render_frames takes them (colour); region_map / region_count / planes of glass_regions (region
    byte, pane normals); source: fused_source; poses (B,3,4) float64 camera-to-world rows [R | t].

    The pixels (x, y) of a frame with x % stride == 0 and y % stride == 0 are candidates.  A candidate is a point when its depth is
    finite and in [min_depth, max_depth], its label is not 255, keep ("all", "glass": label 1, "non_glass") admits the label and -
    edge=e - no lattice neighbour with such a depth zn differs by more than e * min(zn, z) (the flying pixels at depth steps).
    Position ((x - cx) z / fx, (y - cy) z / fy, z), through the pose when given; normals=True: a pixel of a pane with a fitted plane
    takes the pane's normal in closed form (facing the camera), any other the normalised cross product of the differences of its
    1-pixel neighbours' positions, oriented towards the camera; all in fp64, rounded once to float32.
    -> dict in CLOUD_KEYS order: cloud (capacity, 32) uint8 - the points of frame 0 in raster order, then frame 1's, ...; a row is
    float32 x y z nx ny nz, uint8 red green blue label region source frame flags (CLOUD_FLAGS; gw_depth_amd.cloud.fields gives the
    views); every row behind the last point is 32 zero bytes (flags 0 = no point) - and cloud_offsets (B+1,) int32, the exclusive
    prefix of the frames' counts, [B] the total.  capacity defaults to B * ceil(Fh / stride) * ceil(Fw / stride); frame_sizes: what
    the host knows of `sizes` (B (fh, fw) pairs; a frame's image bounds it as well) - with it a capacity may go down to
    cloud_capacity(B, Fh, Fw, stride, frame_sizes), the most these frames can yield; a smaller one raises here, the kernels never
    truncate.  Fresh tensors, no host sync; repeated calls give bit-identical results."""
    opt = check_cloud_options(stride, min_depth, max_depth, edge, normals, keep)
    for name, t, dt in (("depth", depth, torch.float32), ("labels", labels, torch.uint8), ("sizes", sizes, torch.int32),
                        ("intrinsics", intrinsics, torch.float64)):
        if not torch.is_tensor(t) or t.dtype != dt:
            raise TypeError("point_cloud: %s must be a %s tensor" % (name, dt))
    for name, t, dt in (("region_map", region_map, torch.uint8), ("region_count", region_count, torch.int32),
                        ("planes", planes, torch.float64), ("source", source, torch.uint8), ("poses", poses, torch.float64)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt):
            raise TypeError("point_cloud: %s must be a %s tensor" % (name, dt))
    if depth.dim() != 3 or 0 in depth.shape:
        raise ValueError("point_cloud: depth must be (B, Fh, Fw), got %s" % (tuple(depth.shape),))
    B, Fh, Fw = depth.shape
    if B > hip.AUGMENT_BATCH or max(Fh, Fw) > 16384:
        raise ValueError("point_cloud: at most %d frames of at most 16384 per side, got %s" % (hip.AUGMENT_BATCH, tuple(depth.shape)))
    for name, t in (("labels", labels), ("region_map", region_map), ("source", source)):
        if t is not None and tuple(t.shape) != (B, Fh, Fw):
            raise ValueError("point_cloud: %s must be %s like depth, got %s" % (name, (B, Fh, Fw), tuple(t.shape)))
    if tuple(sizes.shape) != (B, 2) or tuple(intrinsics.shape) != (B, 4):
        raise ValueError("point_cloud: sizes must be (%d, 2) and intrinsics (%d, 4)" % (B, B))
    if len({t is None for t in (region_map, region_count, planes)}) != 1:
        raise ValueError("point_cloud: region_map, region_count and planes come together (ops.glass_regions with planes=True)")
    if planes is not None and (tuple(region_count.shape) != (B,) or planes.dim() != 3 or planes.shape[0] != B or planes.shape[2] != 6
                               or not 1 <= planes.shape[1] <= hip.REGION_MAX):
        raise ValueError("point_cloud: region_count must be (%d,) and planes (%d, 1..%d, 6)" % (B, B, hip.REGION_MAX))
    if poses is not None and tuple(poses.shape) != (B, 3, 4):
        raise ValueError("point_cloud: poses must be (%d, 3, 4) = rows [R | t] per frame, got %s" % (B, tuple(poses.shape)))
    frames = _render_views(frames, B, "frames", "point_cloud")
    if frames is not None:                                # a frame is read where it lies when its pixels are dense, whatever its row pitch
        if any(f.dtype != torch.uint8 for f in frames):
            raise TypeError("point_cloud: frames must be %s" % torch.uint8)
        frames = [f if f.dim() != 3 or (f.stride(2) == 1 and f.stride(1) == 3) else f.contiguous() for f in frames]
    if frame_sizes is not None:
        frame_sizes = [(int(h), int(w)) for h, w in frame_sizes]
        if len(frame_sizes) != B or any(h < 1 or w < 1 for h, w in frame_sizes):
            raise ValueError("point_cloud: frame_sizes is %d pairs (fh, fw) >= 1" % B)
    if frames is not None and all(f.dim() == 3 for f in frames):      # a frame's image bounds it too
        known = frame_sizes or [(Fh, Fw)] * B
        frame_sizes = [(min(h, f.shape[0]), min(w, f.shape[1])) for (h, w), f in zip(known, frames)]
    worst = cloud_capacity(B, Fh, Fw, opt["stride"], frame_sizes)
    capacity = cloud_capacity(B, Fh, Fw, opt["stride"]) if capacity is None else _whole("capacity", capacity, "point_cloud")
    if capacity < worst:
        raise ValueError("point_cloud: a capacity of %d rows is below the %d points these frames can yield at stride %d: the cloud is "
                         "never shortened" % (capacity, worst, opt["stride"]))
    if capacity > 2 ** 31 - 1:
        raise ValueError("point_cloud: a capacity of %d rows exceeds 2^31 - 1 (a larger stride, fewer frames per call)" % capacity)
    lib, dev = _lib(), depth.device
    c = lambda t: None if t is None else t.contiguous()
    ws = torch.empty(lib.workspace_bytes(hip.WS_CLOUD, B, Fh, Fw, opt["stride"]), dtype=torch.uint8, device=dev)
    res = {"cloud": torch.empty((capacity, hip.CLOUD_RECORD), dtype=torch.uint8, device=dev),
           "cloud_offsets": torch.empty((B + 1,), dtype=torch.int32, device=dev)}
    lib.point_cloud(c(depth), c(labels), c(sizes), c(intrinsics), frames, c(region_map), c(region_count), c(planes), c(source), c(poses),
                    frame_sizes, opt["stride"], opt["min_depth"], opt["max_depth"], opt["edge"], opt["normals"], opt["keep"], ws,
                    res["cloud"], res["cloud_offsets"])
    return res


# ---------------------------------------------------------------------------------------------------------------------- scene map
SCENE_KEYS = ("cloud", "cloud_offsets", "voxel_stats")


def check_scene_options(voxel, max_voxels, origin=(0.0, 0.0, 0.0), slots=None, min_obs=1, keep="all"):
    """Host validation of scene_merge's options (gw_depth_amd.cloud.SceneMap's parameters and extract's); -> them as a dict."""
    from . import cloud as _cloud
    voxel, max_voxels, origin, slots = _cloud.check_scene_parameters(voxel, max_voxels, origin, slots)
    return dict(voxel=voxel, max_voxels=max_voxels, origin=origin, slots=slots, **_cloud.check_extract_options(min_obs, keep))


def scene_merge(cloud, cloud_offsets, voxel, max_voxels=None, origin=(0.0, 0.0, 0.0), slots=None, min_obs=1, keep="all"):
    """One cloud merged into voxels of `voxel` metres, on the device (gwd_scene_*; tests/scene_ref.py is the
    statement): reset + integrate + extract on a throw-away gw_depth_amd.cloud.SceneMap - the device's np.unique over quantised
    positions.  cloud (rows, 32) uint8 / cloud_offsets (B+1,) int32 of point_cloud, in one world (poses=).  max_voxels defaults to
    the cloud's rows (a cloud cannot fill more).  -> dict in SCENE_KEYS order as SceneMap.extract returns it; with more than
    max_voxels voxels the cloud is EMPTY (cloud_offsets [0, 0]), never truncated.  No host sync.  A stream of calls keeps one
    SceneMap instead."""
    from . import cloud as _cloud
    if not torch.is_tensor(cloud) or cloud.dtype != torch.uint8 or cloud.dim() != 2 or cloud.shape[1] != hip.CLOUD_RECORD:
        raise TypeError("scene_merge: cloud must be a (rows, %d) uint8 tensor" % hip.CLOUD_RECORD)
    if max_voxels is None:
        max_voxels = max(int(cloud.shape[0]), 1)
    opt = check_scene_options(voxel, max_voxels, origin, slots, min_obs, keep)
    _cloud.check_integrate_operands(cloud, cloud_offsets)
    m = _cloud.SceneMap(opt["voxel"], opt["max_voxels"], opt["origin"], opt["slots"], device=cloud.device)
    return m.integrate(cloud, cloud_offsets).extract(opt["min_obs"], opt["keep"])


# ---------------------------------------------------------------------------------------------------------------------- scene view
VIEW_KEYS = ("view_depth", "view_labels", "view_index", "view_rgb")


def check_view_options(min_depth=1e-3, max_depth=10.0, footprint=0.0, max_splat=32, keep="all"):
    """Host validation of cloud_view's options; -> them as a dict."""
    for name, value in (("min_depth", min_depth), ("max_depth", max_depth), ("footprint", footprint)):
        try:
            if isinstance(value, (bool, str)):
                raise TypeError
            float(value)
        except (TypeError, ValueError):
            raise TypeError("cloud_view: %s must be a number of metres, got %r" % (name, value))
    if not 0.0 < float(min_depth) <= float(max_depth) < float("inf"):
        raise ValueError("cloud_view: 0 < min_depth <= max_depth, both finite, got %r, %r" % (min_depth, max_depth))
    if not 0.0 <= float(footprint) < float("inf"):
        raise ValueError("cloud_view: footprint must be finite and >= 0 metres, got %r" % (footprint,))
    max_splat = _whole("max_splat", max_splat, "cloud_view")
    if not 1 <= max_splat <= hip.VIEW_MAX_SPLAT:
        raise ValueError("cloud_view: 1 <= max_splat <= %d pixels, got %r" % (hip.VIEW_MAX_SPLAT, max_splat))
    if keep not in hip.CLOUD_KEEP:
        raise ValueError("cloud_view: keep must be one of %s, got %r" % (", ".join(repr(k) for k in hip.CLOUD_KEEP), keep))
    return dict(min_depth=float(min_depth), max_depth=float(max_depth), footprint=float(footprint), max_splat=max_splat, keep=keep)


def cloud_view(cloud, cloud_offsets, intrinsics, sizes, poses=None, plane=None, view_sizes=None, **options):
    """A cloud seen from V <= 16 posed pinhole cameras, z-buffered on the device (gwd_cloud_view, DESIGN.md section 33;
    tests/view_ref.py is the statement): cloud (rows, 32) uint8 with cloud_offsets int32 (only its last entry, the total, is read) -
    point_cloud's, or SceneMap.extract's - intrinsics (V,4) (fx, fy, cx, cy), sizes (V,2) (fh, fw), poses (V,3,4) camera-to-world rows
    [R | t] as point_cloud takes them (None: the cloud is in the camera's frame).  intrinsics and poses: tensors or nested sequences,
    taken as float64.  sizes: a nested sequence, or an int32 tensor on the cloud's device - then plane = (Fh, Fw)
    is needed, nothing is read back (view_sizes: what the host knows of such sizes, V pairs the device's are clamped to).  plane
    defaults to the largest fh and fw.

    A row with flag 1, finite coordinates and a label keep admits is drawn where min_depth <= Z <= max_depth as a square of
    footprint metres (at least one pixel, at most max_splat pixels) around its projection; footprint=0: the one nearest pixel.  A
    pixel keeps the nearest row (depth rounded once to float32, ties to the lowest row): exact, and the same bytes on every call.
    -> dict in VIEW_KEYS order, fresh tensors: view_depth (V,Fh,Fw) float32 (0: empty), view_labels uint8 (255: empty), view_index
    int32 (the row of the cloud, -1: empty), view_rgb (V,Fh,Fw,3) uint8 (0 without colour).  Three launches, no host sync."""
    opt = check_view_options(**options)
    if not torch.is_tensor(cloud) or cloud.dtype != torch.uint8 or cloud.dim() != 2 or cloud.shape[1] != hip.CLOUD_RECORD:
        raise TypeError("cloud_view: cloud must be a (rows, %d) uint8 tensor" % hip.CLOUD_RECORD)
    if not torch.is_tensor(cloud_offsets) or cloud_offsets.dtype != torch.int32:
        raise TypeError("cloud_view: cloud_offsets must be an int32 tensor (point_cloud's, on the device)")
    if cloud_offsets.dim() != 1 or cloud_offsets.numel() < 2 or cloud_offsets.device != cloud.device:
        raise ValueError("cloud_view: cloud_offsets must be (B + 1,) on the cloud's device, got %s on %s" % (tuple(cloud_offsets.shape), cloud_offsets.device))
    if cloud.shape[0] > 2 ** 31 - 1:
        raise ValueError("cloud_view: at most 2^31 - 1 rows per call, got %d" % cloud.shape[0])
    dev = cloud.device
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float64)
    if intrinsics.dim() != 2 or intrinsics.shape[1] != 4 or not 1 <= intrinsics.shape[0] <= hip.VIEW_MAX_VIEWS:
        raise ValueError("cloud_view: intrinsics must be (V, 4) = (fx, fy, cx, cy) per view, 1 <= V <= %d, got %s" % (hip.VIEW_MAX_VIEWS, tuple(intrinsics.shape)))
    V = intrinsics.shape[0]
    if poses is not None:
        poses = torch.as_tensor(poses, dtype=torch.float64)
        if tuple(poses.shape) != (V, 3, 4):
            raise ValueError("cloud_view: poses must be (%d, 3, 4) = rows [R | t] per view, got %s" % (V, tuple(poses.shape)))
    on_device = torch.is_tensor(sizes) and sizes.device == dev
    if torch.is_tensor(sizes) and sizes.dtype != torch.int32:
        raise TypeError("cloud_view: sizes as a tensor must be int32")
    if on_device:
        if plane is None:
            raise ValueError("cloud_view: sizes on the device need plane=(Fh, Fw): nothing is read back")
    else:
        view_sizes = sizes.tolist() if torch.is_tensor(sizes) else sizes
    if view_sizes is not None:
        try:
            view_sizes = [(_whole("fh", h, "cloud_view"), _whole("fw", w, "cloud_view")) for h, w in view_sizes]
        except ValueError:
            raise ValueError("cloud_view: sizes is %d pairs (fh, fw)" % V)
        if len(view_sizes) != V or any(h < 1 or w < 1 for h, w in view_sizes):
            raise ValueError("cloud_view: sizes is %d pairs (fh, fw) >= 1, got %r" % (V, view_sizes))
    if not on_device:
        sizes = torch.tensor(view_sizes, dtype=torch.int32)
    if tuple(sizes.shape) != (V, 2):
        raise ValueError("cloud_view: sizes must be (%d, 2), got %s" % (V, tuple(sizes.shape)))
    if plane is None:
        plane = (max(h for h, _ in view_sizes), max(w for _, w in view_sizes))
    try:
        Fh, Fw = (_whole("plane", v, "cloud_view") for v in plane)
    except ValueError:
        raise ValueError("cloud_view: plane is (Fh, Fw), got %r" % (plane,))
    if not 1 <= Fh <= 16384 or not 1 <= Fw <= 16384:
        raise ValueError("cloud_view: a plane is 1 .. 16384 per side, got %r" % ((Fh, Fw),))
    lib = _lib()
    if cloud.shape[0] == 0:                               # no rows: one row without flag 1 stands in, the total is clamped anyway
        cloud = torch.zeros((1, hip.CLOUD_RECORD), dtype=torch.uint8, device=dev)
    to = lambda t: None if t is None else t.to(dev, non_blocking=True).contiguous()
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ws = new((lib.workspace_bytes(hip.WS_VIEW, V, Fh, Fw),), torch.uint8)
    res = {"view_depth": new((V, Fh, Fw), torch.float32), "view_labels": new((V, Fh, Fw), torch.uint8),
           "view_index": new((V, Fh, Fw), torch.int32), "view_rgb": new((V, Fh, Fw, 3), torch.uint8)}
    lib.cloud_view(cloud.contiguous(), cloud_offsets.contiguous(), to(sizes), to(intrinsics), to(poses), view_sizes, opt["min_depth"],
                   opt["max_depth"], opt["footprint"], opt["max_splat"], opt["keep"], ws, res["view_depth"], res["view_index"],
                   res["view_labels"], res["view_rgb"])
    return res

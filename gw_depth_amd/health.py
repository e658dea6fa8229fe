"""Host side of the guarded optimizer step (csrc/health.hip): the segment and chunk tables of a flat buffer, the device state of
TrainStep(guard=..., stats_every=...) and the decoding of its records.  The tables are plain host functions (no device needed).

A flat buffer is laid out as engine.TrainStep lays it out: tensor `name` at offsets[name], numel elements long, the next one at the
next multiple of engine.ALIGN.  Segment s is exactly one tensor; the padding behind it belongs to no segment and is never read.
"""
import numpy as np
import torch

from . import hip

# include/gwdepth.h: gwd_health_ctl, gwd_health_record, gwd_segment_record, gwd_health_chunk
CTL_DTYPE = np.dtype([("sq", "<f8"), ("applied", "<i8"), ("skipped", "<i8"), ("streak", "<i8"), ("nonfinite_total", "<i4"), ("apply", "<i4"),
                      ("loss_finite", "<i4"), ("reserved", "<i4"), ("bc1", "<f4"), ("bc2", "<f4"), ("clip_coef", "<f4"), ("loss", "<f4")])
RING_DTYPE = np.dtype([("step", "<i8"), ("grad_norm", "<f8"), ("clip_coef", "<f4"), ("loss", "<f4"), ("apply", "<i4"), ("nonfinite_total", "<i4")])
STAT_DTYPE = np.dtype([("sumsq", "<f8"), ("absmax", "<f4"), ("nonfinite", "<i4")])
CHUNK_DTYPE = np.dtype([("begin", "<i8"), ("len", "<i4"), ("segment", "<i4")])
assert (CTL_DTYPE.itemsize, RING_DTYPE.itemsize, STAT_DTYPE.itemsize, CHUNK_DTYPE.itemsize) == \
    (hip.HEALTH_CTL_BYTES, hip.HEALTH_RING_BYTES, hip.HEALTH_RECORD_BYTES, hip.HEALTH_RECORD_BYTES)


def segment_table(names, offsets, numels):
    """-> (begin, end) lists: segment s is flat[begin[s] : end[s]), the tensor names[s]."""
    begin = [int(offsets[n]) for n in names]
    end = [b + int(numels[n]) for b, n in zip(begin, names)]
    return begin, end


def chunk_table(seg_begin, seg_end, chunk=hip.HEALTH_CHUNK):
    """Every segment cut, in segment order, into pieces of at most `chunk` elements -> CHUNK_DTYPE array.  No piece straddles two
    segments or touches padding; an empty segment has no piece; every piece but a segment's last is `chunk` long."""
    if chunk < 8 or chunk % 8:
        raise ValueError("chunk must be a positive multiple of 8, got %r" % (chunk,))
    rows = []
    for s, (b, e) in enumerate(zip(seg_begin, seg_end)):
        for lo in range(b, e, chunk):
            rows.append((lo, min(chunk, e - lo), s))
    return np.array(rows, dtype=CHUNK_DTYPE)


def check_tables(seg_begin, seg_end, chunks, n, chunk=hip.HEALTH_CHUNK, align=8):
    """What gwd_segment_stats relies on and cannot check on the device: raises ValueError otherwise."""
    prev = 0
    for s, (b, e) in enumerate(zip(seg_begin, seg_end)):
        if b % align or not (prev <= b <= e <= n):
            raise ValueError("segment %d = [%d, %d) is misaligned, out of order or outside the buffer of %d elements" % (s, b, e, n))
        prev = e
    cover = [b for b in seg_begin]
    last = -1
    for c in chunks:
        s, b, ln = int(c["segment"]), int(c["begin"]), int(c["len"])
        if s < last or not (0 <= s < len(cover)) or b != cover[s] or not (1 <= ln <= chunk) or b + ln > seg_end[s] or b % align:
            raise ValueError("chunk (%d, %d, %d) does not continue the cover of its segment" % (b, ln, s))
        cover[s] = b + ln
        last = s
    if cover != list(seg_end):
        raise ValueError("the chunks do not cover every segment exactly once")


def decode(buf, dtype):
    """A uint8 host tensor -> numpy records."""
    return np.frombuffer(buf.numpy().tobytes(), dtype=dtype)


class HealthState:
    """The device buffers of the guarded step: tables, the statistics of flat_g (row 0) and flat_p (row 1), control block + ring."""

    def __init__(self, names, offsets, numels, total, device, ring_len, lib):
        if int(ring_len) < 1:
            raise ValueError("ring must be >= 1, got %r" % (ring_len,))
        self.names, self.ring_len, self.S = list(names), int(ring_len), len(names)
        begin, end = segment_table(names, offsets, numels)
        chunks = chunk_table(begin, end)
        check_tables(begin, end, chunks, total)
        self.seg_begin = torch.tensor(begin, dtype=torch.int64, device=device)
        self.seg_end = torch.tensor(end, dtype=torch.int64, device=device)
        self.chunks = torch.from_numpy(chunks.view("<i8").reshape(-1, 2).copy()).to(device)
        self.partial = torch.empty(lib.workspace_bytes(hip.WS_HEALTH, len(chunks)), dtype=torch.uint8, device=device)
        self.stats = torch.zeros(2, self.S * hip.HEALTH_RECORD_BYTES, dtype=torch.uint8, device=device)
        self.state = torch.zeros(hip.HEALTH_CTL_BYTES + self.ring_len * hip.HEALTH_RING_BYTES, dtype=torch.uint8, device=device)
        self.ctl, self.ring = self.state[:hip.HEALTH_CTL_BYTES], self.state[hip.HEALTH_CTL_BYTES:]
        self.bad = torch.zeros(self.S, dtype=torch.int32, device=device)
        self.have_grad = self.have_param = False

    def grad_stats(self, lib, flat_g):
        lib.segment_stats(flat_g, self.seg_begin, self.seg_end, self.chunks, self.partial, self.stats[0])
        self.have_grad = True

    def param_stats(self, lib, flat_p):
        lib.segment_stats(flat_p, self.seg_begin, self.seg_end, self.chunks, self.partial, self.stats[1])
        self.have_param = True

    def decide(self, lib, loss, beta1, beta2, max_norm, grad_scale):
        lib.health_decide(self.stats[0], self.S, loss, self.ctl, self.ring, self.ring_len, self.bad, beta1, beta2, max_norm, grad_scale)

    def snapshot(self):
        """The control block on its way to the host -> (host uint8 tensor, event or None); nothing waits."""
        if not self.ctl.is_cuda:
            return self.ctl.clone(), None
        slot = torch.empty(hip.HEALTH_CTL_BYTES, dtype=torch.uint8, pin_memory=True)
        slot.copy_(self.ctl, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return slot, ev

    @staticmethod
    def ctl_dict(host):
        """gwd_health_ctl -> counters + the newest ring record (every field of the record is also a field of the block)."""
        c = decode(host, CTL_DTYPE)[0]
        return {"applied": int(c["applied"]), "skipped": int(c["skipped"]), "streak": int(c["streak"]), "sq": float(c["sq"]),
                "bc1": float(c["bc1"]), "bc2": float(c["bc2"]), "loss_finite": bool(c["loss_finite"]),
                "last": {"step": int(c["applied"] + c["skipped"]), "apply": bool(c["apply"]), "clip_coef": float(c["clip_coef"]),
                         "loss": float(c["loss"]), "nonfinite_total": int(c["nonfinite_total"])}}

    def read_ctl(self):
        return self.ctl_dict(self.ctl.cpu())                      # one D2H copy of 64 bytes

    def read_ring(self):
        """The ring in step order: a list of dicts (one D2H copy)."""
        rec = decode(self.ring.cpu(), RING_DTYPE)
        rec = sorted((r for r in rec if r["step"] > 0), key=lambda r: int(r["step"]))
        return [{"step": int(r["step"]), "apply": bool(r["apply"]), "grad_norm": float(r["grad_norm"]), "clip_coef": float(r["clip_coef"]),
                 "loss": float(r["loss"]), "nonfinite_total": int(r["nonfinite_total"])} for r in rec]

    def read_stats(self):
        """-> (grad records, param records), numpy STAT_DTYPE arrays of S entries (one D2H copy)."""
        rec = decode(self.stats.cpu().reshape(-1), STAT_DTYPE)
        return rec[:self.S], rec[self.S:]

    def read_bad(self):
        bad = self.bad.cpu().tolist()
        return [n for n, k in zip(self.names, bad) if k > 0]

    def seed_applied(self, applied):
        """A loaded checkpoint: Adam's step continues from `applied`; the skip counters start over."""
        c = np.zeros(1, dtype=CTL_DTYPE)
        c["applied"] = int(applied)
        self.ctl.copy_(torch.from_numpy(c.view(np.uint8).copy()))

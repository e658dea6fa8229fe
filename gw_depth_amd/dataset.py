"""Dataset loaders: from a GW-Depth directory to the batches TrainStep and evaluate() take.

gw_depth_amd/decode.py decodes the files (a pool of worker processes, one record per sample in shared memory); this module owns what
happens to the records on the way to DeviceAugment.apply_batch / device_collate (gw_depth_amd/data.py):

    FrameStore    decode once, keep every record in ONE uint8 arena - in HBM (where='device': an epoch costs no decode and no upload)
                  or in pinned host memory (where='pinned': one H2D copy per batch)
    StreamSource  no store: records go from the pool's shared memory into one of two pinned slabs, one H2D copy per batch, while the
                  pool already decodes the next batch
    epoch_indices the index order of torch.utils.data.DistributedSampler
    TrainLoader   batches for TrainStep.__call__;  eval_loader: the 5-tuples evaluate() iterates

A batch reaches the augmentation with at most one copy and ONE launch: RGB and label planes are views of the records, the 16-bit depth
planes are widened to int32 by gwd_widen_u16_batch (csrc/frames.hip).
"""
import math

import numpy as np
import torch

from . import data, hip
from .decode import ALIGN, plane_layout

MAX_BATCH = hip.WIDEN_BATCH            # frames() takes at most this many samples: one widen launch, one augmentation plan


def _round_up(n):
    return -(-int(n) // ALIGN) * ALIGN


def host_buffer(nbytes, device):
    """uint8 host memory a copy to `device` reads: pinned when the device is a GPU."""
    return torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=torch.device(device).type == "cuda")


def upload(host, dst):
    """THE host-to-device copy of this module (asynchronous from pinned memory): host uint8 (n,) -> dst uint8 (n,) on the device."""
    dst.copy_(host, non_blocking=True)
    return dst


class _Slab:
    """A pinned staging buffer that grows on demand and is reused only after the copy that read it last has completed."""

    def __init__(self, device):
        self.device, self.buf, self.event = torch.device(device), None, None

    def take(self, nbytes):
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = host_buffer(max(nbytes, 1), self.device)
        return self.buf[:nbytes]

    def copied(self):
        """Call behind the copy out of the slab."""
        if self.device.type == "cuda":
            self.event = torch.cuda.Event()
            self.event.record()


def _batch_layout(sizes):
    """Record offsets of a batch buffer (each at a multiple of ALIGN) and its size."""
    offs, total = [], 0
    for h, w in sizes:
        offs.append(total)
        total = _round_up(total + plane_layout(h, w)[3])
    return offs, total


def _frames_of(buf, offs, sizes):
    """[(rgb, depth_mm int32, labels)] of the records at `offs` in the device buffer `buf`: RGB and labels as views, the depth planes
    widened into one fresh int32 allocation by ONE launch."""
    if not sizes:
        return []
    npix = [h * w for h, w in sizes]
    wide = torch.empty(sum(npix), dtype=torch.int32, device=buf.device)
    out, jobs, at = [], [], 0
    for o, (h, w), n in zip(offs, sizes, npix):
        o_r, o_d, o_l, _ = plane_layout(h, w)
        depth = wide[at:at + n]
        jobs.append((buf[o + o_d:o + o_d + 2 * n], depth))
        out.append((buf[o + o_r:o + o_r + 3 * n].view(h, w, 3), depth.view(h, w), buf[o + o_l:o + o_l + n].view(h, w)))
        at += n
    hip.library().widen_u16_batch(jobs)
    return out


def _check_batch(indices, n):
    indices = [int(i) for i in indices]
    if not 0 < len(indices) <= MAX_BATCH:
        raise ValueError("1..%d samples per call, got %d" % (MAX_BATCH, len(indices)))
    for i in indices:
        if not 0 <= i < n:
            raise IndexError("sample %d of %d" % (i, n))
    return indices


class FrameStore:
    """Every sample of a dataset, decoded once: the records (decode.plane_layout) back to back in one uint8 arena, the polygon JSON,
    image ids and names on the host.  Build with FrameStore.build()."""

    def __init__(self, arena, offsets, sizes, shapes, image_ids, names, device, where):
        self.arena, self.offsets, self.sizes = arena, offsets, sizes
        self._shapes, self._ids, self._names = shapes, image_ids, names
        self.device, self.where = torch.device(device), where
        self._slabs, self._turn = [_Slab(device), _Slab(device)], 0

    @classmethod
    def build(cls, index, pool, device="cuda", where="device", chunk_bytes=256 << 20):
        """Decodes every sample of `index` through `pool` (a decode.DecodePool over the same index).  where='device': the arena is a
        device tensor, filled by one pinned H2D copy per chunk of samples (about `chunk_bytes` each, through two alternating slabs);
        where='pinned': the arena is pinned host memory."""
        if where not in ("device", "pinned"):
            raise ValueError("where must be 'device' or 'pinned', got %r" % (where,))
        device = torch.device(device)
        n = len(index)
        sizes = [index.size(i) for i in range(n)]                    # PNG headers only: the arena is allocated once
        offsets, total = _batch_layout(sizes)
        shapes, ids, names = [None] * n, [None] * n, [index.name(i) for i in range(n)]
        results = pool.map(range(n))

        def take(i, dst):
            r = next(results)
            if r.rgb.shape[:2] != sizes[i]:
                raise ValueError("sample %r decodes to %s, its header said %s" % (r.name, r.rgb.shape[:2], sizes[i]))
            dst[:r.record.size] = r.record
            shapes[i], ids[i] = r.shapes, r.image_id

        if where == "pinned":
            arena = host_buffer(total, device)
            view = arena.numpy()
            for i in range(n):
                take(i, view[offsets[i]:])
        else:
            arena = torch.empty(total, dtype=torch.uint8, device=device)
            slabs, turn, i = [_Slab(device), _Slab(device)], 0, 0
            while i < n:
                j = i + 1                                            # samples i .. j-1: whole records, about chunk_bytes of them
                while j < n and offsets[j] + plane_layout(*sizes[j])[3] - offsets[i] <= chunk_bytes:
                    j += 1
                end = offsets[j] if j < n else total
                slab = slabs[turn].take(end - offsets[i])
                view = slab.numpy()
                for k in range(i, j):
                    take(k, view[offsets[k] - offsets[i]:])
                upload(slab, arena[offsets[i]:end])
                slabs[turn].copied()
                turn, i = 1 - turn, j
            for s in slabs:
                s.take(0)                                            # the last copies have read their slabs
        return cls(arena, offsets, sizes, shapes, ids, names, device, where)

    def __len__(self):
        return len(self.offsets)

    @property
    def nbytes(self):
        return int(self.arena.numel())

    def shapes(self, i):
        return self._shapes[i]

    def image_id(self, i):
        return self._ids[i]

    def name(self, i):
        return self._names[i]

    def frames(self, indices):
        """[(rgb uint8 (h,w,3), depth_mm int32 (h,w), labels uint8 (h,w))] device tensors of up to 16 samples.  where='device': views
        of the arena plus one widen launch; where='pinned': the chosen records go over in ONE H2D copy first."""
        indices = _check_batch(indices, len(self))
        sizes = [self.sizes[i] for i in indices]
        if self.where == "device":
            return _frames_of(self.arena, [self.offsets[i] for i in indices], sizes)
        offs, total = _batch_layout(sizes)
        slab = self._slabs[self._turn]
        host = slab.take(total)
        src, dst = self.arena.numpy(), host.numpy()
        for i, o, (h, w) in zip(indices, offs, sizes):
            nb = plane_layout(h, w)[3]
            dst[o:o + nb] = src[self.offsets[i]:self.offsets[i] + nb]
        buf = upload(host, torch.empty(total, dtype=torch.uint8, device=self.device))
        slab.copied()
        self._turn = 1 - self._turn
        return _frames_of(buf, offs, sizes)

    def record_gt(self, indices):
        """[(depth_mm uint16 (h,w), labels uint8 (h,w))] of up to 16 samples as VIEWS of the device arena: the ground truth exactly as
        the records hold it, for evaluate.FrameMetrics.update - no widen launch, no copy.  where='device' only."""
        if self.where != "device":
            raise ValueError("record_gt needs the records in HBM (where='device'); a pinned store goes through frames()")
        out = []
        for i in _check_batch(indices, len(self)):
            h, w = self.sizes[i]
            _, o_d, o_l, _ = plane_layout(h, w)
            o = self.offsets[i]
            out.append((self.arena[o + o_d:o + o_d + 2 * h * w].view(torch.uint16).view(h, w), self.arena[o + o_l:o + o_l + h * w].view(h, w)))
        return out

    def record_rgb(self, indices):
        """[rgb uint8 (h,w,3)] of up to 16 samples as views of the device arena (record_gt's companion: frames() without the depth)."""
        if self.where != "device":
            raise ValueError("record_rgb needs the records in HBM (where='device'); a pinned store goes through frames()")
        out = []
        for i in _check_batch(indices, len(self)):
            h, w = self.sizes[i]
            out.append(self.arena[self.offsets[i]:self.offsets[i] + 3 * h * w].view(h, w, 3))
        return out


class StreamSource:
    """frames(indices) without a store, for datasets that do not fit: every call decodes its samples through the pool, gathers the
    records into one of two pinned slabs and sends them over in one H2D copy.  prefetch(indices) hands the pool a LATER batch's
    samples early, so that they are decoded while the device works on the current batch; frames() must then be called with the
    prefetched batches in the same order."""

    def __init__(self, index, pool, device="cuda"):
        self.index, self.pool, self.device = index, pool, torch.device(device)
        self._slabs, self._turn = [_Slab(device), _Slab(device)], 0
        self._batches = []             # prefetched batches, oldest first
        self._todo = []                # their samples not yet submitted to the pool
        self._meta = {}                # index -> (shapes, image_id) of the samples seen so far

    def __len__(self):
        return len(self.index)

    def name(self, i):
        return self.index.name(i)

    def shapes(self, i):
        """The polygon JSON of a sample frames() has delivered."""
        return self._meta[i][0]

    def image_id(self, i):
        return self._meta[i][1]

    def _pump(self):
        while self._todo and self.pool.free_slots:
            self.pool.submit(self._todo.pop(0))

    def prefetch(self, indices):
        indices = _check_batch(indices, len(self))
        self._batches.append(indices)
        self._todo += indices
        self._pump()

    def frames(self, indices):
        indices = _check_batch(indices, len(self))
        if not self._batches:
            self.prefetch(indices)
        if self._batches[0] != indices:
            raise ValueError("StreamSource.frames(%r) called while batch %r was prefetched first" % (indices, self._batches[0]))
        self._batches.pop(0)
        sizes = [self.index.size(i) for i in indices]
        offs, total = _batch_layout(sizes)
        slab = self._slabs[self._turn]
        dst = slab.take(total).numpy()
        for i, o, size in zip(indices, offs, sizes):
            self.pool.release()                                    # the previous record is in the slab: its slot decodes again
            self._pump()
            r = self.pool.next()
            if r.index != i or r.rgb.shape[:2] != size:
                raise RuntimeError("StreamSource: the pool delivered sample %d (%s) where %d (%s) was due - is it shared with another "
                                   "consumer?" % (r.index, r.rgb.shape[:2], i, size))
            dst[o:o + r.record.size] = r.record
            self._meta[i] = (r.shapes, r.image_id)
        self.pool.release()
        self._pump()
        buf = upload(slab.buf[:total], torch.empty(total, dtype=torch.uint8, device=self.device))
        slab.copied()
        self._turn = 1 - self._turn
        return _frames_of(buf, offs, sizes)


def epoch_indices(n, epoch, seed=0, shuffle=True, rank=0, world=1, drop_last=False):
    """The indices torch.utils.data.DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
    drop_last=drop_last) yields after set_epoch(epoch): randperm under manual_seed(seed + epoch), wrap-around padding (or truncation,
    with drop_last) to a multiple of `world`, then every world-th index from `rank`.  shuffle=False, world=1: range(n), the
    reference's SequentialSampler."""
    n, world, rank = int(n), int(world), int(rank)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank %d of world %d" % (rank, world))
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        indices = torch.randperm(n, generator=g).tolist()
    else:
        indices = list(range(n))
    if drop_last and n % world != 0:
        per_rank = math.ceil((n - world) / world)
    else:
        per_rank = math.ceil(n / world)
    total = per_rank * world
    if not drop_last:
        pad = total - len(indices)
        if pad <= len(indices):
            indices += indices[:pad]
        else:
            indices += (indices * math.ceil(pad / len(indices)))[:pad]
    else:
        indices = indices[:total]
    return indices[rank:total:world]


def _to_device(targets, device):
    return [{k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in t.items()} for t in targets]


def _assemble(source, indices, augment, device, dtype, with_center, pad_to):
    """frames -> one augment.params(w, h) per item IN BATCH ORDER -> data.assemble_batch."""
    frames = source.frames(indices)
    params = [augment.params(int(f[0].shape[1]), int(f[0].shape[0])) for f in frames]
    items = [f + (source.shapes(i), source.image_id(i)) for f, i in zip(frames, indices)]
    return data.assemble_batch(items, params, device=device, dtype=dtype, with_center=with_center, pad_to=pad_to)


class TrainLoader:
    """Iterates one epoch of training batches: {'images', 'pad_mask', 'depth', 'seg', 'targets'} as TrainStep.__call__ takes them,
    target tensors on the device.  `source` is a FrameStore or a StreamSource, `augment` a data.DeviceAugment; the order is
    epoch_indices(len(source), epoch, ...) in batches of `batch_size` (<= 16).  Call set_epoch(e) before each epoch, as with the
    reference's DistributedSampler (main_glassrgbd.py:86-97, 199-200)."""

    def __init__(self, source, batch_size, augment, seed=0, shuffle=True, rank=0, world=1, drop_last=True, pad_to=None, with_center=True,
                 dtype=torch.float32):
        if not 0 < int(batch_size) <= MAX_BATCH:
            raise ValueError("batch_size must be 1..%d, got %r" % (MAX_BATCH, batch_size))
        self.source, self.batch_size, self.augment = source, int(batch_size), augment
        self.seed, self.shuffle, self.rank, self.world, self.drop_last = seed, shuffle, rank, world, drop_last
        self.pad_to, self.with_center, self.dtype = pad_to, with_center, dtype
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def batches(self):
        """The index lists of this epoch's batches (the sampler never drops: drop_last is the BATCH sampler's, as in the reference)."""
        idx = epoch_indices(len(self.source), self.epoch, self.seed, self.shuffle, self.rank, self.world, False)
        out = [idx[k:k + self.batch_size] for k in range(0, len(idx), self.batch_size)]
        if self.drop_last and out and len(out[-1]) < self.batch_size:
            out.pop()
        return out

    def __len__(self):
        return len(self.batches())

    def __iter__(self):
        batches = self.batches()
        ahead = getattr(self.source, "prefetch", None)
        if ahead is not None and batches:
            ahead(batches[0])
        for k, indices in enumerate(batches):
            if ahead is not None and k + 1 < len(batches):
                ahead(batches[k + 1])                              # decoded while this batch is assembled and the step runs
            batch, targets = _assemble(self.source, indices, self.augment, self.source.device, self.dtype, self.with_center, self.pad_to)
            batch["targets"] = _to_device(targets, self.source.device)
            yield batch


class _EvalLoader:
    def __init__(self, source, augment, with_center, dtype):
        self.source, self.augment, self.with_center, self.dtype = source, augment, with_center, dtype

    def __len__(self):
        return len(self.source)

    def __iter__(self):
        from .model import NestedTensor
        n = len(self.source)
        ahead = getattr(self.source, "prefetch", None)
        if ahead is not None and n:
            ahead([0])
        for i in range(n):
            if ahead is not None and i + 1 < n:
                ahead([i + 1])
            b, targets = _assemble(self.source, [i], self.augment, self.source.device, self.dtype, self.with_center, None)
            yield (NestedTensor(b["images"], b["pad_mask"]), NestedTensor(b["depth"], b["pad_mask"]), NestedTensor(b["seg"], b["pad_mask"]),
                   _to_device(targets, self.source.device), [self.source.name(i)])


def eval_loader(source, augment=None, with_center=True, dtype=torch.float32):
    """The loader evaluate() iterates (main_glassrgbd.py:93-97: batch size 1, sequential, nothing dropped): 5-tuples
    (samples, depth_gt, seg_gt, targets, [name]) with the first three NestedTensors.  augment: DeviceAugment(train=False) by default."""
    return _EvalLoader(source, data.DeviceAugment(train=False) if augment is None else augment, with_center, dtype)

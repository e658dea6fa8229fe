"""The grouped augmentation kernels (gwd_resample_u8_pass_batch, gwd_gather2d_batch, gwd_color_adjust_batch) on the GPU:
DeviceAugment.apply_batch equals DeviceAugment.apply on the device and the oracle chain, bit for bit, on the seven frames of
tests/augment_batch_cases.py; and the raw entry points write nothing outside their outputs and refuse n = 0 and n = 17."""
import ctypes

import numpy as np
import pytest
import torch

from gw_depth_amd import data, hip
from tests import augment_batch_cases as cases

pytestmark = pytest.mark.gpu

SEVEN = list(range(cases.N))
BATCHES = [([k], True, True) for k in SEVEN] + [(SEVEN, True, True), ((SEVEN * 3)[:16], True, True), (SEVEN, False, True), (SEVEN, True, False)]
IDS = ["frame%d" % k for k in SEVEN] + ["seven", "sixteen", "no_depth", "no_labels"]


@pytest.fixture
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    return hip.library()


@pytest.mark.parametrize("indices,depth,labels", BATCHES, ids=IDS)
def test_apply_batch_bit_exact(lib, indices, depth, labels):
    cases.check_batch(indices, "cuda", depth=depth, labels=labels)


POISON = 0xA5
GUARD = 256


class Arena:
    """Outputs carved out of one poisoned byte buffer with GUARD bytes before, between and after them."""

    def __init__(self, sizes):
        self.offsets, n = [], GUARD
        for s in sizes:
            self.offsets.append(n)
            n += (s + 15) // 16 * 16 + GUARD
        self.sizes = list(sizes)
        self.buf = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")

    def out(self, k, shape, dtype=torch.uint8):
        return self.buf[self.offsets[k]:self.offsets[k] + self.sizes[k]].view(dtype).view(shape)

    def guards_untouched(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for o, s in zip(self.offsets, self.sizes):
            keep[o:o + s] = False
        return bool((self.buf[keep] == POISON).all())


def test_resample_batch_writes_only_its_outputs(lib):
    """Jobs of different ksize, n_out and other in one launch per axis, each against the single-call kernel."""
    rng = np.random.default_rng(21)
    shapes = [((72, 128), 181), ((61, 97), 33), ((128, 40), 5), ((50, 90), 9)]           # (h, w), n_out: up- and downscales, ksize 3..53
    for axis in (1, 0):
        parts, jobs, wants, n_tab = [], [], [], 0
        dims = [((h, n) if axis == 1 else (n, w)) + (3,) for (h, w), n in shapes]
        arena = Arena([int(np.prod(d)) for d in dims])
        for k, ((h, w), n_out) in enumerate(shapes):
            src = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
            b, kk = data.bilinear_tables(w if axis == 1 else h, n_out)
            flip = k % 2 == 1                                                             # every other job reads its source flipped on both axes
            m0, m1 = data._flip_map(w if axis == 1 else h, flip), data._flip_map(h if axis == 1 else w, flip)
            want = torch.empty(dims[k], dtype=torch.uint8, device="cuda")
            lib.resample_u8_pass(src, want, torch.from_numpy(b).cuda(), torch.from_numpy(kk).cuda(), axis, w * 3, m0[0], m0[1], m1[0], m1[1])
            jobs.append((src, arena.out(k, dims[k]), w * 3, n_tab, n_tab + b.size, kk.shape[1], m0[0], m0[1], m1[0], m1[1]))
            parts += [b.reshape(-1), kk.reshape(-1)]
            n_tab += b.size + kk.size
            wants.append(want)
        assert len({j[5] for j in jobs}) == len(jobs)                                     # all different ksize
        lib.resample_u8_pass_batch(jobs, axis, 3, torch.from_numpy(np.concatenate(parts)).cuda())
        for j, want in zip(jobs, wants):
            assert torch.equal(j[1], want)
        assert arena.guards_untouched()


def test_gather_batch_writes_only_its_outputs(lib):
    """Element widths 1, 2, 3 and 4 in one launch, odd sizes, more than one workgroup per job."""
    rng = np.random.default_rng(22)
    specs = [(torch.uint8, 1, (70, 45), (33, 91)), (torch.int16, 1, (31, 64), (57, 19)), (torch.uint8, 3, (40, 50), (61, 77)),
             (torch.int32, 1, (72, 128), (96, 170))]
    eb = [torch.empty(0, dtype=dt).element_size() * per for dt, per, _, _ in specs]
    arena = Arena([oh * ow * e for e, (_, _, _, (oh, ow)) in zip(eb, specs)])
    parts, jobs, wants, n_tab = [], [], [], 0
    for k, (dt, per, (h, w), (oh, ow)) in enumerate(specs):
        src = torch.from_numpy(rng.integers(0, 120, (h, w, per) if per > 1 else (h, w))).to(dt).cuda()
        yt, xt = rng.integers(0, h, oh).astype(np.int32), rng.integers(0, w, ow).astype(np.int32)
        want = src[torch.from_numpy(yt).cuda().long()][:, torch.from_numpy(xt).cuda().long()].contiguous()
        dst = arena.out(k, want.shape, dt)
        jobs.append((src, dst, w * eb[k], n_tab, n_tab + oh, oh, ow, eb[k]))
        parts += [yt, xt]
        n_tab += oh + ow
        wants.append(want)
    lib.gather2d_batch(jobs, torch.from_numpy(np.concatenate(parts)).cuda())
    for j, want in zip(jobs, wants):
        assert torch.equal(j[1], want)
    assert arena.guards_untouched()


def test_color_batch_writes_only_its_images(lib):
    """All four modes and an untouched job in one launch, in place, each against the single-call kernel."""
    rng = np.random.default_rng(23)
    ops = [("brightness", 1.3), ("contrast", 0.7), (None, 0.0), ("saturation", 1.4), ("hue", float(data.hue_shift(-0.2))), ("contrast", 1.2)]
    shapes = [(37, 53), (64, 70), (20, 20), (45, 31), (50, 50), (33, 129)]
    arena = Arena([h * w * 3 for h, w in shapes])
    jobs, wants, srcs = [], [], []
    for k, ((name, f), (h, w)) in enumerate(zip(ops, shapes)):
        src = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
        img = arena.out(k, (h, w, 3))
        img.copy_(src)
        want = src.clone()
        if name is not None:
            lib.color_adjust(src, want, name, f, torch.zeros(1, dtype=torch.int64, device="cuda") if name == "contrast" else None)
        jobs.append((img, name, f))
        wants.append(want)
        srcs.append(src)
    sums = torch.zeros(hip.AUGMENT_BATCH, dtype=torch.int64, device="cuda")
    lib.color_adjust_batch(jobs, sums, sums_only=True)
    assert all(torch.equal(j[0], src) for j, src in zip(jobs, srcs))                                      # touches no pixel ...
    assert [bool(v) for v in sums.tolist()[:len(ops)]] == [name == "contrast" for name, _ in ops]         # ... and only the contrast sums
    lib.color_adjust_batch(jobs, sums)
    for j, want in zip(jobs, wants):
        assert torch.equal(j[0], want)
    assert arena.guards_untouched()


def test_raw_entry_points_refuse_zero_and_seventeen_jobs(lib):
    """n = 0 and n over the cap return -1 before anything is launched: the (valid) outputs keep their poison."""
    L = lib.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    arena = Arena([8 * 8 * 3])
    dst = arena.out(0, (8, 8, 3))
    tables = torch.cat([torch.tensor([[i, 1] for i in range(8)], dtype=torch.int32).view(-1), torch.full((8,), 1 << 22, dtype=torch.int32),
                        torch.arange(8, dtype=torch.int32)]).cuda()
    for n in (0, hip.AUGMENT_BATCH + 1):
        rj = (hip.ResampleJob * 17)()
        cj = (hip.ColorJob * 17)()
        for r, c in zip(rj, cj):
            r.src, r.dst, r.src_row_stride = src.data_ptr(), dst.data_ptr(), 24
            r.bounds_off, r.kk_off, r.ksize, r.n_out, r.other, r.base0, r.step0, r.base1, r.step1 = 0, 16, 1, 8, 8, 0, 1, 0, 1
            c.rgb, c.npix, c.mode, c.factor = dst.data_ptr(), 64, 0, 0.5
        assert L.gwd_resample_u8_pass_batch(rj, n, 1, 3, tables.data_ptr(), tables.numel(), stream) == -1
        assert L.gwd_color_adjust_batch(cj, n, None, hip.COLOR_ADJUST, stream) == -1
    for n in (0, hip.GATHER_BATCH + 1):
        gj = (hip.GatherJob * (hip.GATHER_BATCH + 1))()
        for g in gj:
            g.src, g.dst, g.src_row_stride_bytes = src.data_ptr(), dst.data_ptr(), 24
            g.ytab_off, g.xtab_off, g.oh, g.ow, g.elem_bytes = 24, 24, 8, 8, 3
        assert L.gwd_gather2d_batch(gj, n, tables.data_ptr(), tables.numel(), stream) == -1
    gj = (hip.GatherJob * 1)()
    gj[0].src, gj[0].dst, gj[0].src_row_stride_bytes = src.data_ptr(), dst.data_ptr(), 24
    gj[0].ytab_off, gj[0].xtab_off, gj[0].oh, gj[0].ow, gj[0].elem_bytes = 24, 24, 8, 8, 5
    assert L.gwd_gather2d_batch(gj, 1, tables.data_ptr(), tables.numel(), stream) == -4                  # unsupported element width
    gj[0].elem_bytes, gj[0].xtab_off = 3, 25
    assert L.gwd_gather2d_batch(gj, 1, tables.data_ptr(), tables.numel(), stream) == -3                  # a table beyond the buffer
    torch.cuda.synchronize()
    assert arena.guards_untouched() and bool((dst == POISON).all())

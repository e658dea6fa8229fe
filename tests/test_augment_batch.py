"""DeviceAugment.apply_batch on the CPU stand-in: the host planning of a whole batch (composed NEAREST tables, windowed first
resize, one table buffer, grouped launches) gives, value for value, what DeviceAugment.apply gives frame by frame and what the
oracle chain gives step by step - in a number of library calls that does not depend on the batch size.  The kernels behind the
three grouped entry points are checked by tests/test_augment_batch_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

from gw_depth_amd import data, hip
from tests import augment_batch_cases as cases
from tests.fake_device import FakeDevice

# the launch budget of one batch, whatever its size
BUDGET = {"resample_u8_pass_batch": 4, "gather2d_batch": 1, "color_adjust": 4, "color_sums": 4, "upload_tables": 1}


class CountingFakeDevice(FakeDevice):
    """The three grouped entry points as loops over the stand-in's single calls, with a count of the grouped calls."""

    def __init__(self):
        self.calls = {k: 0 for k in BUDGET}

    def resample_u8_pass_batch(self, jobs, axis, C, tables):
        self.calls["resample_u8_pass_batch"] += 1
        assert 0 < len(jobs) <= hip.AUGMENT_BATCH
        for src, dst, row_stride, bounds_off, kk_off, ksize, base0, step0, base1, step1 in jobs:
            n_out = dst.shape[1] if axis == 1 else dst.shape[0]
            assert dst.shape[2] == C
            bounds = tables[bounds_off:bounds_off + 2 * n_out].view(n_out, 2)
            kk = tables[kk_off:kk_off + n_out * ksize].view(n_out, ksize)
            self.resample_u8_pass(src, dst, bounds, kk, axis, row_stride, base0, step0, base1, step1)

    def gather2d_batch(self, jobs, tables):
        self.calls["gather2d_batch"] += 1
        assert 0 < len(jobs) <= hip.GATHER_BATCH
        for src, dst, row_stride_bytes, ytab_off, xtab_off, oh, ow, elem_bytes in jobs:
            self.gather2d(src, dst, tables[ytab_off:ytab_off + oh], tables[xtab_off:xtab_off + ow], row_stride_bytes, elem_bytes)

    def color_adjust_batch(self, jobs, sums, sums_only=False):
        self.calls["color_sums" if sums_only else "color_adjust"] += 1
        assert 0 < len(jobs) <= hip.AUGMENT_BATCH
        if any(mode == "contrast" for _, mode, _ in jobs):
            assert sums is not None and sums.numel() >= len(jobs) and not sums.any()      # zeroed by the caller, one per job
        if sums_only:                                                   # the stand-in's contrast computes its own mean
            return
        for rgb, mode, factor in jobs:
            if mode is not None:
                self.color_adjust(rgb, rgb, mode, factor)


@pytest.fixture
def fake(monkeypatch):
    lib = CountingFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        assert host.dtype == torch.int32 and host.dim() == 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


BATCHES = [[k] for k in range(cases.N)] + [list(range(cases.N))]


@pytest.mark.parametrize("indices", BATCHES, ids=["frame%d" % b[0] if len(b) == 1 else "all" for b in BATCHES])
@pytest.mark.parametrize("full", [True, False], ids=["polygons", "lines"])
def test_apply_batch_equals_apply_and_the_oracle(fake, indices, full):
    cases.check_batch(indices, "cpu", full=full)
    assert fake.calls["upload_tables"] == 1
    for k, n in fake.calls.items():
        assert n <= BUDGET[k], (k, n)


def test_library_calls_do_not_depend_on_the_batch_size(fake):
    seven = list(range(cases.N))
    counts = []
    for indices in ([2], seven, (seven * 3)[:16]):                     # B = 1 (frame 2 runs both resize stages), 7 and 16
        for k in fake.calls:
            fake.calls[k] = 0
        cases.check_batch(indices, "cpu")
        counts.append(dict(fake.calls))
    assert counts[1] == counts[2], counts
    # one frame alone launches no more than the whole batch, and with a chain that uses every kind of launch exactly as much
    assert counts[0] == dict(counts[1], color_sums=1), counts
    assert counts[1] == BUDGET, counts


def test_validation_params_launch_no_jitter_and_one_upload(fake):
    p = data.DeviceAugment(train=False, max_size=160, test_size=96).params(128, 72)
    frames = cases.device_frames([0, 4], "cpu")
    out = data.DeviceAugment.apply_batch(frames, [cases.frame(0)[3]] * 2, [p, p])
    assert fake.calls == {"resample_u8_pass_batch": 2, "gather2d_batch": 1, "color_adjust": 0, "color_sums": 0, "upload_tables": 1}
    for f, o in zip(frames, out):
        want = data.DeviceAugment.apply(*f, cases.frame(0)[3], p)
        assert all(torch.equal(a, b) for a, b in zip(o, want))


def test_untouched_frames_are_returned_as_they_are(fake):
    (rgb, dep, lab), = cases.device_frames([4], "cpu")
    out = data.DeviceAugment.apply_batch([(rgb, dep, lab)], [cases.frame(4)[3]], [{"flip": None, "steps": []}])
    assert out[0][0] is rgb and out[0][1] is dep and out[0][2] is lab and sum(fake.calls.values()) == 0


def test_more_than_sixteen_frames_raise(fake):
    seventeen = (list(range(cases.N)) * 3)[:17]
    with pytest.raises(ValueError):
        data.DeviceAugment.apply_batch(cases.device_frames(seventeen, "cpu"), [cases.frame(k)[3] for k in seventeen],
                                       [cases.CASES[k][1] for k in seventeen])
    with pytest.raises(ValueError):
        data.DeviceAugment.apply_batch([], [], [])
    assert sum(fake.calls.values()) == 0


def test_assemble_batch_equals_assemble_item_and_collate(fake):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "line_transforms.npz"))
    shapes = json.loads(str(z["item_shapes"]))
    rgb, dmm, lab = torch.from_numpy(z["item_rgb"]), torch.from_numpy(z["item_depth_mm"]).to(torch.int32), torch.from_numpy(z["item_labels"])
    h, w = rgb.shape[:2]
    aug = data.DeviceAugment(train=True, max_size=2 * max(h, w), seed=4)
    params = [None, {"flip": "h", "steps": [("resize", max(8, min(h, w) // 2), None)], "jitter": data.jitter_params(aug.rng)},
              {"flip": "v", "steps": [("resize", min(h, w) + 3, None), ("crop", (1, 2, min(h, w) - 2, min(h, w) - 3)), ("resize", min(h, w), None)]}]
    items = [(rgb, dmm, lab, shapes, 31 + n) for n in range(len(params))]
    batch, targets = data.assemble_batch(items, params, device="cpu")
    singles = [data.assemble_item(*it, with_center=True, params=p) for it, p in zip(items, params)]
    want = data.device_collate([s[:3] for s in singles], device="cpu")
    assert sorted(batch) == sorted(want)
    for k in want:
        assert batch[k].dtype == want[k].dtype and torch.equal(batch[k], want[k]), k
    for t, s in zip(targets, singles):
        assert sorted(t) == sorted(s[3])
        for k in t:
            assert t[k].dtype == s[3][k].dtype and torch.equal(t[k], s[3][k]), k
    plain = data.assemble_batch(items, params, device="cpu", with_center=False)[1]
    assert all(t["lines"].shape[1] == 4 and torch.equal(t["lines"], u["lines"][:, :4]) for t, u in zip(plain, targets))


def test_composed_and_windowed_tables_equal_the_step_by_step_result():
    """200 random (size, crop, size) triples per axis: the composed NEAREST table is the crop of the first resize followed by the
    second, and a BILINEAR pass with its tables sliced to the window is the window of the full pass."""
    rng = np.random.default_rng(17)
    for _ in range(200):
        n0, n1 = int(rng.integers(2, 300)), int(rng.integers(2, 300))
        c = int(rng.integers(1, n1 + 1))
        i = int(rng.integers(0, n1 - c + 1))
        n2 = int(rng.integers(1, 300))
        flipped = bool(rng.integers(0, 2))
        line = rng.integers(0, 12000, n0).astype(np.int32)
        # NEAREST: flip -> resize n0 -> n1 -> crop [i, i + c) -> resize c -> n2, one step at a time
        step = line[::-1] if flipped else line
        step = step[data.nearest_table(n0, n1)][i:i + c][data.nearest_table(c, n2)]
        yt1 = data.nearest_table(n0, n1)
        if flipped:
            yt1 = n0 - 1 - yt1
        composed = yt1[i + data.nearest_table(c, n2)]                   # ytab[y] = yt1[i + yt2[y]]
        np.testing.assert_array_equal(line[composed], step)
        # ... and as the planner builds it
        tab = np.arange(n0, dtype=np.int32)[::-1] if flipped else np.arange(n0, dtype=np.int32)
        tab = tab[data._nearest_table_cached(n0, n1)][i:i + c][data._nearest_table_cached(c, n2)]
        np.testing.assert_array_equal(tab, composed)
        # BILINEAR: one pass over a row of pixels, full then cropped, against the pass with the tables sliced to the window
        px = rng.integers(0, 256, n0).astype(np.int64)
        bounds, kk = data.bilinear_tables(n0, n1)

        def one_pass(b, k):
            t = np.arange(k.shape[1])[None, :]
            idx = np.minimum(b[:, :1] + t, n0 - 1)
            acc = (px[idx] * k * (t < b[:, 1:2])).sum(1) + (1 << 21)
            return np.clip(acc >> 22, 0, 255)

        np.testing.assert_array_equal(one_pass(bounds[i:i + c], kk[i:i + c]), one_pass(bounds, kk)[i:i + c])
        cb, ck = data._bilinear_tables_cached(n0, n1)
        np.testing.assert_array_equal(cb, bounds)
        np.testing.assert_array_equal(ck, kk)

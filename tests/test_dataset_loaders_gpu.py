"""Dataset loaders on the device.  gwd_widen_u16_batch (csrc/frames.hip) element by element at every launch edge, in process; the
loaders end to end - FrameStore in HBM, FrameStore in pinned memory, StreamSource - against batches assembled from arrays this test
decodes itself, in a fresh child process (tests/dataset_child.py: the decode pool must start before the GPU is initialised).
Everything is compared bit for bit."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gw_depth_amd import data, hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "dataset_child.py")
SPECIAL = np.array([0, 1, 32767, 32768, 65535], dtype=np.uint16)
SENTINEL, GUARD = -123456789, 64
LENGTHS = [1, 2, 7, 8, 9, 2047, 2048, 2049, 37 * 53, 65537]
SRC_OFFSETS, DST_OFFSETS = [0, 2, 6, 14], [0, 4, 12]                  # bytes past a 16-byte boundary


def plane(n, src_off, rng):
    """n 16-bit values: random, with the special values at the first and the last element and on both sides of every 16-byte
    boundary of a source that starts src_off bytes past one."""
    v = rng.integers(0, 65536, n, dtype=np.uint16)
    head = ((16 - src_off) % 16) // 2
    edges = np.arange(head, n + 1, 8)
    marks = np.unique(np.clip(np.concatenate([[0, n - 1], edges - 1, edges, edges + 1]), 0, n - 1)) if n else np.zeros(0, dtype=np.int64)
    v[marks] = SPECIAL[(np.arange(marks.size) + src_off + n) % 5]
    return v


class Case:
    """One job: its source bytes inside a 16-byte aligned device buffer, its destination between two guards of sentinels."""

    def __init__(self, n, src_off, dst_off, rng, device):
        self.n, self.values = n, plane(n, src_off, rng)
        host = np.zeros(16 + src_off + 2 * n + 16, dtype=np.uint8)
        host[16 + src_off:16 + src_off + 2 * n] = self.values.view(np.uint8)
        self.src_buf = torch.from_numpy(host).to(device)
        assert self.src_buf.data_ptr() % 16 == 0
        self.src = self.src_buf[16 + src_off:16 + src_off + 2 * n]
        self.lead = GUARD + dst_off // 4
        self.dst_buf = torch.full((self.lead + n + GUARD,), SENTINEL, dtype=torch.int32, device=device)
        assert self.dst_buf.data_ptr() % 16 == 0 and (GUARD * 4) % 16 == 0
        self.dst = self.dst_buf[self.lead:self.lead + n]

    def check(self, what):
        got = self.dst_buf.cpu().numpy()
        assert (got[:self.lead] == SENTINEL).all() and (got[self.lead + self.n:] == SENTINEL).all(), what
        assert np.array_equal(got[self.lead:self.lead + self.n], self.values.astype(np.int32)), what


def test_widen_one_job_at_every_length_and_alignment():
    lib = hip.library()
    assert not getattr(lib, "is_fake", False)
    rng = np.random.default_rng(5)
    cases = [Case(n, so, do, rng, "cuda") for n in LENGTHS for so in SRC_OFFSETS for do in DST_OFFSETS]
    for c in cases:
        lib.widen_u16_batch([(c.src, c.dst)])
    torch.cuda.synchronize()
    for c, key in zip(cases, ((n, so, do) for n in LENGTHS for so in SRC_OFFSETS for do in DST_OFFSETS)):
        c.check(key)
    assert all(set(SPECIAL.tolist()) <= set(c.values.tolist()) for c in cases if c.n >= 2047)


def test_widen_sixteen_jobs_of_mixed_lengths_in_one_launch():
    lib = hip.library()
    rng = np.random.default_rng(6)
    lengths = LENGTHS + [0, 420 * 560, 3, 16, 4095, 500 * 404]        # one empty job; two whole depth planes of the end-to-end test
    assert len(lengths) == hip.WIDEN_BATCH
    cases = [Case(n, SRC_OFFSETS[k % 4], DST_OFFSETS[(k // 2) % 3], rng, "cuda") for k, n in enumerate(lengths)]
    lib.widen_u16_batch([(c.src, c.dst) for c in cases])
    torch.cuda.synchronize()
    for k, c in enumerate(cases):
        c.check((k, c.n))
    with pytest.raises(ValueError):
        lib.widen_u16_batch([(c.src, c.dst) for c in cases] + [(cases[0].src, cases[0].dst)])
    with pytest.raises(ValueError):
        lib.widen_u16_batch([(cases[0].src, cases[1].dst)])
    odd = cases[3].src_buf[17:17 + 2 * cases[3].n]                    # an odd source address is refused, nothing is written
    with pytest.raises(RuntimeError, match="-3"):
        lib.widen_u16_batch([(odd, cases[3].dst)])


# ------------------------------------------------------------------------------------------------------------------------ end to end
SIZES = [(420, 560), (480, 640), (500, 404)]
N = 9


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_synth_dataset", os.path.join(ROOT, "tools", "make_synth_dataset.py"))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    d = str(tmp_path_factory.mktemp("synth_gpu"))
    synth.write_dataset(d, N, SIZES, seed=0)
    return d


def run_child(mode, dataset_dir, timeout):
    r = subprocess.run([sys.executable, CHILD, mode, dataset_dir], timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, "tests/dataset_child.py %s ended with status %d:\n%s" % (mode, r.returncode, r.stdout[-3000:])
    assert r.stdout.rstrip().endswith("ok")


def test_train_loader_batches_equal_hand_built_batches_for_every_source(dataset_dir):
    """FrameStore (device), FrameStore (pinned) and StreamSource: every batch of two epochs of TrainLoader(batch_size=4, pad_to=64,
    DeviceAugment(train=True, seed=s)), s = 0..3, is torch.equal - tensor for tensor, target for target - to data.assemble_batch
    on arrays the child decodes itself with Pillow, in DistributedSampler's order with an identically seeded DeviceAugment."""
    from tests import dataset_child as child
    flips, chains = set(), set()
    for s in child.SEEDS:                                             # the draws the child will make, made here on the CPU
        aug = data.DeviceAugment(train=True, seed=s)
        for e in range(child.EPOCHS):
            for indices in child.epoch_batches(N, e, child.BATCH):
                for i in indices:
                    h, w = SIZES[i % 3]
                    p = aug.params(w, h)
                    flips.add(p["flip"])
                    chains.add(tuple(step[0] for step in p["steps"]))
    assert flips == {"h", "v", None}, flips
    assert chains == {("resize",), ("resize", "crop", "resize")}, chains
    run_child("loaders", dataset_dir, 600)


def test_evaluate_and_train_step_take_the_loaders_batches(dataset_dir):
    """eval_loader feeds evaluate() with the product model at batch 1 (frames shrunk by DeviceAugment(train=False, test_size=96,
    max_size=128)): the stats equal those over a plain list of the same tuples built by hand.  Two eager TrainStep steps on loader
    batches (B = 2) give finite losses equal to those of the same steps - from the same weights and AdamW state - on hand-built batches.  After close() the process has no children."""
    run_child("model", dataset_dir, 900)

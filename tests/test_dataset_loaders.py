"""Dataset loaders on the CPU: file layout and decoding (gw_depth_amd/decode.py), the worker pool, the sampler, and the store /
stream / loader logic of gw_depth_amd/dataset.py over the CPU stand-in.  Every comparison is bit-exact: nothing here rounds.
The widen kernel and the loaders on the device are checked by tests/test_dataset_loaders_gpu.py."""
import ctypes
import importlib.util
import json
import os
import random
import shutil
import signal
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

from gw_depth_amd import data, dataset, decode, hip
from tests.test_augment_batch import CountingFakeDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(45, 61), (64, 48), (37, 53)]
N = 7


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


synth = load_tool("make_synth_dataset")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("synth"))
    synth.write_dataset(d, N, SIZES, seed=3)
    return d


@pytest.fixture(scope="module")
def index(root):
    return decode.GlassRGBDIndex(**synth.index_args(root))


@pytest.fixture(scope="module")
def direct(index):
    """Every sample as Pillow and json read it, decoded once for all tests (never written to)."""
    out = []
    for i in range(len(index)):
        img, dep, seg, js = index.paths(i)
        doc = json.load(open(js))
        arrays = [np.asarray(Image.open(p)) for p in (img, dep, seg)]
        for a in arrays:
            a.setflags(write=False)
        out.append((*arrays, doc["shapes"], doc["imageId"], index.name(i)))
    return out


def same_item(got, want):
    return (all(np.array_equal(g, w) and g.dtype == w.dtype and g.shape == w.shape for g, w in zip(got[:3], want[:3]))
            and got[3] == want[3] and got[4] == want[4] and got[5] == want[5])


# ------------------------------------------------------------------------------------------------------------------ decode and layout
def test_synthetic_dataset_has_the_stated_content(root, index, direct):
    assert len(index) == N and [d[0].shape[:2] for d in direct] == [SIZES[k % 3] for k in range(N)]
    assert {Image.open(index.paths(i)[2]).mode for i in range(N)} == {"L", "P"}
    assert all(Image.open(index.paths(i)[1]).mode == "I;16" and Image.open(index.paths(i)[0]).mode == "RGB" for i in range(N))
    for rgb, dep, lab, shapes, _, _ in direct[:-1]:
        assert dep.min() == 0 and dep.max() == 65535 and lab.max() > 0
        assert sum(1 for s in shapes if len(s["points"]) == 0) == 1 and sum(1 for s in shapes if len(s["points"]) >= 3) >= 2
    assert direct[-1][3] == []
    again = os.path.join(os.path.dirname(root), "again")
    synth.write_dataset(again, 2, SIZES, seed=3)                     # seeded: the same bytes
    for sub, ext in (("images", ".png"), ("depth", ".png"), ("seg", ".png"), ("lines", ".json")):
        assert open(os.path.join(again, sub, "s0000" + ext), "rb").read() == open(os.path.join(root, sub, "s0000" + ext), "rb").read()


def test_decode_item_equals_pillow_and_json(index, direct):
    for i, want in enumerate(direct):
        got = decode.decode_item(index, i)
        assert same_item(got, want), i
        assert got[0].dtype == np.uint8 and got[1].dtype == np.uint16 and got[2].dtype == np.uint8
        assert index.size(i) == got[0].shape[:2]


def _variant(root, tmp_path, change):
    d = str(tmp_path / "variant")
    shutil.copytree(root, d)
    change(d)
    return decode.GlassRGBDIndex(**synth.index_args(d))


@pytest.mark.parametrize("sub,make", [
    ("images", lambda p: Image.open(p).convert("RGBA").save(p)),
    ("images", lambda p: Image.open(p).convert("L").save(p)),
    ("depth", lambda p: Image.open(p).convert("L").save(p)),
    ("depth", lambda p: Image.open(p).convert("RGB").save(p)),
    ("seg", lambda p: Image.open(p).convert("RGB").save(p)),
    ("seg", lambda p: Image.open(p).convert("1").save(p)),
    ("depth", lambda p: Image.open(p).crop((0, 0, 20, 20)).save(p)),
    ("seg", lambda p: Image.open(p).crop((0, 0, 30, 31)).save(p)),
], ids=["rgba", "grey-image", "depth-8bit", "depth-rgb", "labels-rgb", "labels-1bit", "depth-size", "labels-size"])
def test_bad_modes_and_sizes_raise_with_the_file_name(root, tmp_path, sub, make):
    idx = _variant(root, tmp_path, lambda d: make(os.path.join(d, sub, "s0002.png")))
    with pytest.raises(ValueError, match=os.path.join(sub, "s0002.png")):
        decode.decode_item(idx, 2)
    assert same_item(decode.decode_item(idx, 3), decode.decode_item(decode.GlassRGBDIndex(**synth.index_args(root)), 3))


def test_depth_of_mode_I_is_taken_within_16_bits(index, monkeypatch, direct):
    real = Image.open

    def as_int32(scale):
        def opener(path, *a, **k):
            im = real(path, *a, **k)
            return Image.fromarray(np.asarray(im).astype(np.int32) * scale) if os.sep + "depth" + os.sep in str(path) else im
        return opener

    monkeypatch.setattr(decode.Image, "open", as_int32(1))
    got = decode.decode_item(index, 0)
    assert got[1].dtype == np.uint16 and np.array_equal(got[1], direct[0][1])
    monkeypatch.setattr(decode.Image, "open", as_int32(2))            # 65535 * 2 no longer fits
    with pytest.raises(ValueError, match="s0000.png"):
        decode.decode_item(index, 0)


@pytest.mark.parametrize("h,w", [(1, 1), (37, 53), (720, 1280)])
def test_plane_layout(h, w):
    o_r, o_d, o_l, total = decode.plane_layout(h, w)
    sizes = (3 * h * w, 2 * h * w, h * w)
    offs = (o_r, o_d, o_l)
    assert all(o % 256 == 0 for o in offs) and o_r == 0
    for k in range(2):                                                # no overlap, and no earlier aligned start would do
        assert offs[k] + sizes[k] <= offs[k + 1] < offs[k] + sizes[k] + 256
    assert total == o_l + sizes[2]
    buf = bytearray(total)
    views = decode.record_views(buf, h, w)
    assert [v.shape for v in views] == [(h, w, 3), (h, w), (h, w)] and [v.dtype.itemsize for v in views] == [1, 2, 1]
    views[1][...] = 0x1234
    assert buf[o_d] == 0x34 and buf[o_d + 1] == 0x12                  # little-endian


def test_index_takes_the_first_token_and_skips_blank_lines(root, tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("s0003 518.8 extra\n\n   \n\ts0001\t7\ns0005\n\n")
    kw = dict(synth.index_args(root), filenames_file=str(lst))
    idx = decode.GlassRGBDIndex(**kw)
    assert len(idx) == 3 and [idx.name(i) for i in range(3)] == ["s0003", "s0001", "s0005"]
    assert idx.paths(1) == (os.path.join(root, "images", "s0001.png"), os.path.join(root, "depth", "s0001.png"),
                            os.path.join(root, "seg", "s0001.png"), os.path.join(os.path.realpath(os.path.join(root, "lines")), "s0001.json"))
    assert idx.id_to_img[1003] == "s0003"
    assert decode.GlassRGBDIndex(**dict(kw, images_json=None)).id_to_img == {}
    args = types.SimpleNamespace(data_path=kw["data_path"], gt_depth_path=kw["gt_depth_path"], gt_seg_path=kw["gt_seg_path"],
                                 gt_line_path=kw["gt_line_path"], filenames_file_train=str(lst),
                                 filenames_file_eval=os.path.join(root, "val.txt"), glassrgbd_images_json=kw["images_json"])
    assert decode.GlassRGBDIndex.from_args(args, "train").names == idx.names
    assert len(decode.GlassRGBDIndex.from_args(args, "val")) == N          # the tool's own lists carry extra tokens and a blank line
    with pytest.raises(ValueError):
        decode.GlassRGBDIndex.from_args(args, "test")


def test_decode_module_does_not_load_torch():
    import subprocess
    code = "import sys; import gw_depth_amd.decode, gw_depth_amd; sys.exit(1 if 'torch' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, timeout=120).returncode == 0


# ------------------------------------------------------------------------------------------------------------------------------ sampler
def test_epoch_indices_equal_distributed_sampler():
    from torch.utils.data import DistributedSampler
    checked = 0
    for n in (1, 11, 16):
        for world in (1, 3):
            for rank in range(world):
                for shuffle in (True, False):
                    for drop_last in (True, False):
                        for seed in (0, 5):
                            s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed, drop_last=drop_last)
                            for e in (0, 1, 5):
                                s.set_epoch(e)
                                got = dataset.epoch_indices(n, e, seed=seed, shuffle=shuffle, rank=rank, world=world, drop_last=drop_last)
                                assert got == list(s) and len(got) == len(s), (n, world, rank, shuffle, drop_last, seed, e)
                                checked += 1
    assert checked == 3 * 4 * 2 * 2 * 2 * 3
    assert dataset.epoch_indices(9, 4, shuffle=False) == list(range(9))
    with pytest.raises(ValueError):
        dataset.epoch_indices(4, 0, rank=2, world=2)


# --------------------------------------------------------------------------------------------------------------------------------- pool
def test_pool_delivers_in_request_order(root, tmp_path, direct):
    big = str(tmp_path / "big")
    synth.write_dataset(big, 1, [(900, 1200)], seed=1)                # ~100 x the pixels of the small ones: it finishes last
    for sub, ext in (("images", ".png"), ("depth", ".png"), ("seg", ".png"), ("lines", ".json")):
        shutil.copy(os.path.join(big, sub, "s0000" + ext), os.path.join(big, sub, "large" + ext))
        for k in range(N):
            shutil.copy(os.path.join(root, sub, "s%04d%s" % (k, ext)), os.path.join(big, sub))
    open(os.path.join(big, "train.txt"), "w").write("large\n" + "".join("s%04d\n" % k for k in range(N)))
    idx = decode.GlassRGBDIndex(**synth.index_args(big))
    with decode.DecodePool(idx, workers=3, slots=8) as pool:
        for i in range(8):
            pool.submit(i)
        with pytest.raises(RuntimeError, match="in flight"):
            pool.submit(0)
        got = []
        for i in range(8):
            r = pool.next()
            got.append(r.name)
            assert r.index == i
            if i:
                assert same_item(tuple(r[:6]), direct[i - 1])
            else:
                assert r.rgb.shape == (900, 1200, 3) and same_item(tuple(r[:6]), decode.decode_item(idx, 0))
            assert set(r.timings) >= {"image", "depth", "labels", "json"}
        assert got == ["large"] + ["s%04d" % k for k in range(N)]
        with pytest.raises(RuntimeError, match="nothing submitted"):
            pool.next()
        order = [6, 0, 6, 3]
        assert [r.index for r in pool.map(order)] == order
    with decode.DecodePool(idx, workers=2, slots=1) as pool:          # one slot: still every sample, one at a time
        assert [(r.index, r.rgb.shape[0]) for r in pool.map([1, 0, 2])] == [(1, 45), (0, 900), (2, 64)]


def test_worker_count_comes_from_the_affinity_mask(index, monkeypatch):
    monkeypatch.setattr(os, "cpu_count", lambda: (_ for _ in ()).throw(AssertionError("os.cpu_count() must not be consulted")))
    for cpus, want in ((64, 15), (16, 15), (4, 3), (2, 1), (1, 1)):
        monkeypatch.setattr(os, "sched_getaffinity", lambda pid, n=cpus: set(range(n)))
        assert decode.default_workers() == want
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: {0, 1, 2})
    with decode.DecodePool(index) as pool:
        assert pool.workers == 2 and len(pool.pids()) == 2
    with decode.DecodePool(index, workers=40) as pool:
        assert pool.workers == 16 and len(pool.pids()) == 16
        assert [r.index for r in pool.map(range(N))] == list(range(N))


def test_corrupt_png_surfaces_as_runtime_error_naming_the_sample(root, tmp_path, direct):
    def truncate(d):
        p = os.path.join(d, "depth", "s0002.png")
        raw = open(p, "rb").read()
        open(p, "wb").write(raw[:len(raw) // 2])
        open(os.path.join(d, "images", "s0004.png"), "wb").write(b"not a png")       # the header itself is unreadable

    idx = _variant(root, tmp_path, truncate)
    with decode.DecodePool(idx, workers=2, slots=5) as pool:
        for i in (1, 2, 3, 4, 5):
            pool.submit(i)
        assert same_item(tuple(pool.next()[:6]), direct[1])
        with pytest.raises(RuntimeError, match="s0002"):
            pool.next()
        assert same_item(tuple(pool.next()[:6]), direct[3])          # the pool goes on behind a failed sample
        with pytest.raises(RuntimeError, match="s0004"):
            pool.next()
        assert same_item(tuple(pool.next()[:6]), direct[5])
        assert pool.in_flight == 1                                   # the one the caller still looks at


def test_close_leaves_no_child_and_no_shared_memory(index):
    from multiprocessing import shared_memory
    pool = decode.DecodePool(index, workers=3)
    assert [h["torch_loaded"] for h in pool.handshakes] == [False] * 3 and "torch" in sys.modules      # loaded here, not there
    assert sorted(h["pid"] for h in pool.handshakes) == sorted(pool.pids())
    list(pool.map(range(N)))
    names, procs = pool.shm_names(), list(pool._procs)
    assert names and all(p.poll() is None for p in procs)
    pool.close()
    pool.close()                                                      # idempotent
    assert all(p.poll() is not None for p in procs)
    for n in names:
        with pytest.raises(FileNotFoundError):
            shared_memory.SharedMemory(name=n)
    with pytest.raises(RuntimeError, match="closed"):
        pool.submit(0)


def test_a_dead_worker_raises_instead_of_hanging(index):
    with decode.DecodePool(index, workers=1, timeout=30.0) as pool:
        pool.submit(0)
        pool.next()
        os.kill(pool.pids()[0], signal.SIGKILL)
        pool._procs[0].wait(timeout=30.0)
        with pytest.raises(RuntimeError, match="worker 0"):
            pool.submit(1)
            pool.next()


def test_pool_refuses_to_start_once_the_gpu_is_initialised(index, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    with pytest.raises(RuntimeError, match="GPU is already initialised"):
        decode.DecodePool(index, workers=1)


# ------------------------------------------------------------------------------------------------- store, stream and loaders (stand-in)
class LoaderFakeDevice(CountingFakeDevice):
    """The augmentation stand-in plus gwd_widen_u16_batch in torch, with a count of the launches."""

    def __init__(self):
        super().__init__()
        self.widen_calls = []

    def widen_u16_batch(self, jobs):
        assert 0 < len(jobs) <= hip.WIDEN_BATCH
        self.widen_calls.append(len(jobs))
        for src, dst in jobs:
            assert src.dtype == torch.uint8 and dst.dtype == torch.int32 and src.numel() == 2 * dst.numel() and dst.is_contiguous()
            dst.copy_(src.view(torch.int16).to(torch.int32) & 0xFFFF)


@pytest.fixture
def fake(monkeypatch):
    lib = LoaderFakeDevice()
    lib.uploads = []
    real = dataset.upload

    def counted(host, dst):
        assert host.dtype == torch.uint8 and host.dim() == 1 and host.shape == dst.shape
        lib.uploads.append(int(host.numel()))
        return real(host, dst)

    monkeypatch.setattr(dataset, "upload", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


@pytest.fixture(scope="module")
def pool(index):
    with decode.DecodePool(index, workers=2) as p:
        yield p


def same_frames(frames, indices, direct):
    for (rgb, dep, lab), i in zip(frames, indices):
        w = direct[i]
        assert rgb.dtype == torch.uint8 and dep.dtype == torch.int32 and lab.dtype == torch.uint8
        assert torch.equal(rgb, torch.from_numpy(w[0].copy())) and torch.equal(lab, torch.from_numpy(w[2].copy()))
        assert torch.equal(dep, torch.from_numpy(w[1].astype(np.int32)))
    return len(frames) == len(indices)


@pytest.mark.parametrize("where", ["device", "pinned"])
def test_store_frames_equal_direct_decoding(fake, index, pool, direct, where):
    store = dataset.FrameStore.build(index, pool, device="cpu", where=where, chunk_bytes=20000)     # several chunks of 1-2 samples
    built = list(fake.uploads)
    assert len(store) == N and store.arena.dtype == torch.uint8 and store.nbytes == store.arena.numel()
    assert store.nbytes >= sum(decode.plane_layout(*s)[3] for s in (SIZES[k % 3] for k in range(N)))
    assert (len(built) > 2 and sum(built) == store.nbytes) if where == "device" else built == []
    for i in range(N):
        assert store.shapes(i) == direct[i][3] and store.image_id(i) == direct[i][4] and store.name(i) == direct[i][5]
    for indices in ([0], [6, 2, 2, 5], list(range(N)), (list(range(N)) * 3)[:16]):
        del fake.uploads[:], fake.widen_calls[:]
        frames = store.frames(indices)
        assert same_frames(frames, indices, direct)
        assert fake.widen_calls == [len(indices)]                     # ONE launch, whatever the batch
        assert len(fake.uploads) == (0 if where == "device" else 1)                  # pinned: ONE copy per call
        if where == "device":                                         # RGB and labels are views of the arena, plane by plane
            base = store.arena.data_ptr()
            for (rgb, dep, lab), i in zip(frames, indices):
                o_r, _, o_l, _ = decode.plane_layout(*store.sizes[i])
                assert rgb.data_ptr() == base + store.offsets[i] + o_r and lab.data_ptr() == base + store.offsets[i] + o_l
                assert store.offsets[i] % 256 == 0
    with pytest.raises(ValueError):
        store.frames(list(range(N)) * 3)
    with pytest.raises(ValueError):
        store.frames([])
    with pytest.raises(IndexError):
        store.frames([N])
    with pytest.raises(ValueError):
        dataset.FrameStore.build(index, pool, device="cpu", where="disk")


def test_stream_source_equals_direct_decoding(fake, index, direct):
    with decode.DecodePool(index, workers=2, slots=3) as small:      # fewer slots than a batch has samples
        src = dataset.StreamSource(index, small, device="cpu")
        batches = [[4, 1, 6, 0, 2], [3], [5, 5, 0, 1, 2, 3, 4, 6]]
        src.prefetch(batches[0])
        for k, b in enumerate(batches):
            if k + 1 < len(batches):
                src.prefetch(batches[k + 1])
            del fake.uploads[:], fake.widen_calls[:]
            assert same_frames(src.frames(b), b, direct)
            assert len(fake.uploads) == 1 and fake.widen_calls == [len(b)]
            assert all(src.shapes(i) == direct[i][3] and src.image_id(i) == direct[i][4] and src.name(i) == direct[i][5] for i in b)
        assert same_frames(src.frames([2, 0]), [2, 0], direct)       # without a prefetch
        src.prefetch([1, 2])
        with pytest.raises(ValueError, match="prefetched"):
            src.frames([2, 1])
        assert same_frames(src.frames([1, 2]), [1, 2], direct)
        assert len(src) == N


class SmallAugment:
    """DeviceAugment's interface with chains sized for the stand-in; records the order of its draws."""

    def __init__(self, seed):
        self.rng, self.drawn = random.Random(seed), []

    def params(self, w, h):
        r = self.rng
        self.drawn.append((w, h))
        steps = [("resize", r.choice([24, 32, 40]), 64)]
        if r.random() < 0.5:
            steps = [("resize", 48, None), ("crop", (r.randint(0, 8), r.randint(0, 8), 36, 38)), ("resize", r.choice([24, 40]), 64)]
        return {"flip": r.choice(["h", "v", None]), "steps": steps, "jitter": data.jitter_params(r) if r.random() < 0.5 else None}


def hand_batch(direct, indices, augment, pad_to=None):
    items = [(torch.from_numpy(direct[i][0].copy()), torch.from_numpy(direct[i][1].astype(np.int32)), torch.from_numpy(direct[i][2].copy()),
              direct[i][3], direct[i][4]) for i in indices]
    params = [augment.params(it[0].shape[1], it[0].shape[0]) for it in items]
    return data.assemble_batch(items, params, device="cpu", pad_to=pad_to)


def same_batch(batch, targets, want, want_targets):
    assert sorted(batch) == sorted(want)
    for k in want:
        assert batch[k].dtype == want[k].dtype and torch.equal(batch[k], want[k]), k
    assert len(targets) == len(want_targets)
    for t, u in zip(targets, want_targets):
        assert sorted(t) == sorted(u)
        for k in u:
            assert t[k].dtype == u[k].dtype and torch.equal(t[k], u[k]), k
    return True


@pytest.mark.parametrize("kind", ["store", "stream"])
def test_train_loader_batches_equal_hand_built_ones(fake, index, pool, direct, kind):
    source = dataset.FrameStore.build(index, pool, device="cpu") if kind == "store" else dataset.StreamSource(index, pool, device="cpu")
    aug, twin = SmallAugment(11), SmallAugment(11)
    loader = dataset.TrainLoader(source, 3, aug, seed=2, pad_to=16)
    assert len(loader) == 2
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        order = dataset.epoch_indices(N, epoch, seed=2)
        want_batches = [order[0:3], order[3:6]]                      # drop_last: the seventh sample is left out
        assert loader.batches() == want_batches
        seen = len(aug.drawn)
        for b, indices in zip(loader, want_batches):
            assert aug.drawn[seen:] == [direct[i][0].shape[1::-1] for i in indices]      # one draw per item, in batch order
            seen = len(aug.drawn)
            targets = b.pop("targets")
            assert same_batch(b, targets, *hand_batch(direct, indices, twin, pad_to=16))
            assert b["images"].shape[2] % 16 == 0 and b["images"].shape[3] % 16 == 0 and b["images"].shape[0] == 3
    assert len(aug.drawn) == 12
    assert dataset.epoch_indices(N, 0, seed=2) != dataset.epoch_indices(N, 1, seed=2)


def test_loader_length_drop_last_and_ranks(fake, index, pool):
    store = dataset.FrameStore.build(index, pool, device="cpu")
    aug = SmallAugment(0)
    L = lambda **kw: dataset.TrainLoader(store, augment=aug, **kw)
    assert len(L(batch_size=2)) == 3 and len(L(batch_size=2, drop_last=False)) == 4
    assert len(L(batch_size=16)) == 0 and len(L(batch_size=16, drop_last=False)) == 1 and list(L(batch_size=16)) == []
    assert [len(b) for b in L(batch_size=2, drop_last=False).batches()] == [2, 2, 2, 1]
    assert L(batch_size=7, shuffle=False).batches() == [list(range(N))]
    parts = [L(batch_size=2, drop_last=False, world=3, rank=r, seed=4) for r in range(3)]
    for p in parts:
        p.set_epoch(3)
    assert [len(p) for p in parts] == [2, 2, 2]                       # 7 -> 9 indices by wrap-around, 3 per rank
    flat = [[i for b in p.batches() for i in b] for p in parts]
    assert flat == [dataset.epoch_indices(N, 3, seed=4, rank=r, world=3) for r in range(3)] and set(sum(flat, [])) == set(range(N))
    last = list(L(batch_size=4, drop_last=False, shuffle=False))[-1]
    assert last["images"].shape[0] == 3 and len(last["targets"]) == 3
    with pytest.raises(ValueError):
        L(batch_size=17)
    with pytest.raises(ValueError):
        L(batch_size=0)


def test_eval_loader_yields_the_tuples_evaluate_iterates(fake, index, pool, direct):
    from gw_depth_amd.model import NestedTensor
    store = dataset.FrameStore.build(index, pool, device="cpu")
    aug = data.DeviceAugment(train=False, test_size=32, max_size=48)
    loader = dataset.eval_loader(store, aug)
    assert len(loader) == N
    got = list(loader)
    assert len(got) == N
    for i, (samples, depth_gt, seg_gt, targets, names) in enumerate(got):
        assert all(isinstance(x, NestedTensor) for x in (samples, depth_gt, seg_gt)) and names == [direct[i][5]] and len(targets) == 1
        want, want_targets = hand_batch(direct, [i], aug)
        assert same_batch({"images": samples.tensors, "pad_mask": samples.mask, "depth": depth_gt.tensors, "seg": seg_gt.tensors},
                          targets, want, want_targets)
        assert samples.tensors.shape[0] == 1 and not bool(samples.mask.any())
        assert int(targets[0]["image_id"]) == direct[i][4] and targets[0]["orig_size"].tolist() == list(direct[i][0].shape[:2])
    assert isinstance(dataset.eval_loader(store).augment, data.DeviceAugment) and not dataset.eval_loader(store).augment.train


# ---------------------------------------------------------------------------------------------------------------------------------- ABI
def test_widen_entry_point_is_declared_bound_and_refuses_bad_arguments():
    assert "gwd_widen_u16_batch" in hip.ENTRY_POINTS and hip.WIDEN_BATCH == 16
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    assert "#define GWD_WIDEN_BATCH 16" in header and "#define GWD_VERSION 10" in header
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    fn = lib.gwd_widen_u16_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(hip.WidenJob), ctypes.c_int32, ctypes.c_void_p]
    assert ctypes.sizeof(hip.WidenJob) == 24
    assert fn(None, 1, None) == -1                                    # null jobs
    jobs = (hip.WidenJob * 17)()
    for j in jobs:
        j.src, j.dst, j.n = 0x1000, 0x2000, 0                         # never dereferenced: n == 0 jobs are skipped, nothing is launched
    assert fn(jobs, 0, None) == -1 and fn(jobs, -3, None) == -1 and fn(jobs, 17, None) == -1
    assert fn(jobs, 16, None) == 0 and fn(jobs, 1, None) == 0
    for field, bad, want in (("src", None, -1), ("dst", None, -1), ("n", -1, -1), ("src", 0x1001, -3), ("dst", 0x2002, -3)):
        keep = getattr(jobs[3], field)
        setattr(jobs[3], field, bad)
        assert fn(jobs, 16, None) == want, (field, bad)
        assert fn(jobs, 3, None) == 0                                 # the bad record is the fourth
        setattr(jobs[3], field, keep)
    assert fn(jobs, 16, None) == 0

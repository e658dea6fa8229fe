"""The end-to-end half of tests/test_dataset_loaders_gpu.py, run as a fresh process: the decode pool has to start before this process
initialises the GPU.  usage: python tests/dataset_child.py {loaders|model} DATASET_DIR   (exit status 0 = every check held)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
from PIL import Image

from gw_depth_amd import decode

SEEDS = (0, 1, 2, 3)
BATCH, PAD_TO, EPOCHS = 4, 64, 2


def index_of(root):
    return decode.GlassRGBDIndex(os.path.join(root, "images"), os.path.join(root, "depth"), os.path.join(root, "seg"),
                                 os.path.join(root, "lines"), os.path.join(root, "train.txt"), os.path.join(root, "images.json"))


def decode_directly(index):
    """The test's own decoding: Pillow and json, nothing of gw_depth_amd.decode."""
    out = []
    for i in range(len(index)):
        img, dep, seg, js = index.paths(i)
        doc = json.load(open(js))
        out.append((np.asarray(Image.open(img)), np.asarray(Image.open(dep)).astype(np.int32), np.asarray(Image.open(seg)),
                    doc["shapes"], doc["imageId"], index.name(i)))
    return out


def epoch_batches(n, epoch, batch, seed=0):
    """Batches of `batch` indices in DistributedSampler's order for one rank, the ragged last batch dropped."""
    from torch.utils.data import DistributedSampler
    s = DistributedSampler(range(n), num_replicas=1, rank=0, shuffle=True, seed=seed)
    s.set_epoch(epoch)
    idx = list(s)
    return [idx[k:k + batch] for k in range(0, len(idx) - batch + 1, batch)]


def hand_batch(direct, indices, augment, pad_to, device="cuda"):
    import torch
    from gw_depth_amd import data
    items = [(torch.from_numpy(direct[i][0].copy()).to(device), torch.from_numpy(direct[i][1]).to(device),
              torch.from_numpy(direct[i][2].copy()).to(device), direct[i][3], direct[i][4]) for i in indices]
    params = [augment.params(it[0].shape[1], it[0].shape[0]) for it in items]
    batch, targets = data.assemble_batch(items, params, device=device, pad_to=pad_to)
    batch["targets"] = [{k: v.to(device) for k, v in t.items()} for t in targets]
    return batch


def assert_same_batch(got, want, what):
    import torch
    assert sorted(got) == sorted(want), what
    for k in want:
        if k == "targets":
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k)
    assert len(got["targets"]) == len(want["targets"]), what
    for t, u in zip(got["targets"], want["targets"]):
        assert sorted(t) == sorted(u), what
        for k in u:
            assert t[k].is_cuda and t[k].dtype == u[k].dtype and torch.equal(t[k], u[k]), (what, k)


def live_children():
    me, out = os.getpid(), []
    for d in os.listdir("/proc"):
        if d.isdigit():
            try:
                fields = open("/proc/%s/stat" % d).read().rsplit(")", 1)[1].split()
            except OSError:
                continue
            if int(fields[1]) == me and fields[0] != "Z":
                out.append(int(d))
    return out


def run_loaders(root):
    index = index_of(root)
    pool = decode.DecodePool(index, workers=4)
    import torch
    from gw_depth_amd import data, dataset, hip
    assert not torch.cuda.is_initialized(), "the pool must be up before the GPU is"
    assert not getattr(hip.library(), "is_fake", False)
    direct = decode_directly(index)
    n = len(index)
    want = {}
    for s in SEEDS:                                                   # the reference batches, once, shared by the three sources
        twin = data.DeviceAugment(train=True, seed=s)
        for e in range(EPOCHS):
            for k, indices in enumerate(epoch_batches(n, e, BATCH)):
                want[s, e, k] = hand_batch(direct, indices, twin, PAD_TO)
    sources = {"store-device": dataset.FrameStore.build(index, pool, device="cuda", where="device", chunk_bytes=3 << 20),
               "store-pinned": dataset.FrameStore.build(index, pool, device="cuda", where="pinned"),
               "stream": dataset.StreamSource(index, pool, device="cuda")}
    assert sources["store-device"].arena.is_cuda and sources["store-pinned"].arena.is_pinned()
    for name, source in sources.items():
        for s in SEEDS:
            loader = dataset.TrainLoader(source, BATCH, data.DeviceAugment(train=True, seed=s), pad_to=PAD_TO)
            for e in range(EPOCHS):
                loader.set_epoch(e)
                assert len(loader) == n // BATCH
                got = 0
                for k, b in enumerate(loader):
                    assert_same_batch(b, want[s, e, k], (name, s, e, k))
                    assert b["images"].shape[0] == BATCH and b["images"].shape[2] % PAD_TO == 0 and b["images"].shape[3] % PAD_TO == 0
                    got += 1
                assert got == n // BATCH
        print("%s: %d batches equal the hand-built ones" % (name, len(want)))
    torch.cuda.synchronize()
    pool.close()
    assert live_children() == [], live_children()


def run_model(root):
    index = index_of(root)
    pool = decode.DecodePool(index, workers=4)
    import torch
    from gw_depth_amd import data, dataset
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.evaluate import evaluate
    from gw_depth_amd.model import NestedTensor
    from tests.golden_check import build
    assert not torch.cuda.is_initialized()
    direct = decode_directly(index)
    store = dataset.FrameStore.build(index, pool, device="cuda")

    # evaluate(): the loader against a plain list of the same tuples built by hand, product model, batch 1
    cfg, model, crits = build(device="cuda")
    args = type("A", (), {"with_line": True, "with_dense": True, "min_depth_eval": 1e-3, "max_depth_eval": 10.0})()
    small = lambda: data.DeviceAugment(train=False, test_size=96, max_size=128)
    by_hand, aug = [], small()
    for i in range(len(index)):
        b = hand_batch(direct, [i], aug, None)
        by_hand.append((NestedTensor(b["images"], b["pad_mask"]), NestedTensor(b["depth"], b["pad_mask"]),
                        NestedTensor(b["seg"], b["pad_mask"]), b["targets"], [direct[i][5]]))
    got = evaluate(model, crits, None, dataset.eval_loader(store, small()), None, "cuda", None, args)
    want = evaluate(model, crits, None, by_hand, None, "cuda", None, args)
    print("evaluate over the loader:", json.dumps(got, sort_keys=True))
    print("evaluate over the list:  ", json.dumps(want, sort_keys=True))
    assert set(got) == set(want) and {"rms", "silog", "Mean IU", "loss"} <= set(got)
    assert all(np.isfinite(v) for v in got.values())
    assert got == want

    # Two eager train steps on loader batches (B = 2) against the same steps on hand-built batches.  "The same step" has to start
    # from the same weights and AdamW state: a train step does not repeat bit for bit from one run to the next (the weight-gradient
    # kernels accumulate with float atomics, bench.py's restart_from_seed says the same), so two TrainSteps that each take their own
    # first step differ in the last bits of the weights before the second - seen on the device as 73.23546600341797 against
    # 73.2359390258789 in one run and as equal values in another, with bit-identical inputs and an equal first loss both times.
    # One TrainStep therefore takes every step twice from one state, once per batch; the second pair runs on updated weights.
    loader = dataset.TrainLoader(store, 2, data.DeviceAugment(train=True, seed=1), pad_to=PAD_TO)
    from_loader = [b for _, b in zip(range(2), loader)]
    twin = data.DeviceAugment(train=True, seed=1)
    hand = [hand_batch(direct, indices, twin, PAD_TO) for indices in epoch_batches(len(index), 0, 2)[:2]]
    cfg, model, crits = build(device="cuda")
    step = TrainStep(model, crits, cfg, compute_dtype=torch.float32)
    got, want = [], []
    for k, (a, b) in enumerate(zip(from_loader, hand)):
        assert_same_batch(a, b, ("train batch", k))
        state = (step.flat_p.clone(), step.flat_m.clone(), step.flat_v.clone(), step.step_count)
        got.append(float(step(a)[1]))
        for buf, saved in zip((step.flat_p, step.flat_m, step.flat_v), state):
            buf.copy_(saved)
        step.step_count = state[3]
        want.append(float(step(b)[1]))
    print("losses on loader batches:    ", got)
    print("losses on hand-built batches:", want)
    assert step.step_count == 2 and not torch.equal(step.flat_p, state[0])
    assert len(got) == 2 and all(np.isfinite(v) for v in got)
    assert got == want
    pool.close()
    assert live_children() == [], live_children()


if __name__ == "__main__":
    {"loaders": run_loaders, "model": run_model}[sys.argv[1]](sys.argv[2])
    print("ok")

#!/usr/bin/env python
"""The augmentation of a batch, frame by frame against grouped: 8 seeded 720 x 1280 frames (RGB + depth + labels) with the training
parameters of DeviceAugment(train=True, seed=0), jitter included, through DeviceAugment.apply per frame + device_collate and through
DeviceAugment.apply_batch + device_collate, in one process on one build.

Time: host clock around work that ends in a device synchronise; the two paths alternate batch by batch; 3 warm-ups, then 50 batches
each, repeated three times to show the spread.  Counts (one untimed batch per path): launches = the kernels and memsets the library
calls enqueue plus the device operations torch issues (fills, dtype copies), copies = host-to-device transfers.
Prints one JSON line and saves it as profiles/augment_batch_bench.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten

from gw_depth_amd import data, hip

B, H, W, WARMUP, BATCHES, REPEATS = 8, 720, 1280, 3, 50, 3


def make_batch():
    aug = data.DeviceAugment(train=True, seed=0)
    frames, lines, params = [], [], []
    for k in range(B):
        rng = np.random.default_rng(k)
        frames.append((torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda(),
                       torch.from_numpy(rng.integers(0, 12000, (H, W)).astype(np.int32)).cuda(),
                       torch.from_numpy(rng.integers(0, 3, (H, W)).astype(np.uint8)).cuda()))
        lines.append(torch.from_numpy(rng.random((12, 4)).astype(np.float32)) * torch.tensor([W, H, W, H]))
        params.append(aug.params(W, H))
    return frames, lines, params


def per_frame(frames, lines, params):
    out = [data.DeviceAugment.apply(*f, l, p) for f, l, p in zip(frames, lines, params)]
    return data.device_collate([o[:3] for o in out])


def batched(frames, lines, params):
    out = data.DeviceAugment.apply_batch(frames, lines, params)
    return data.device_collate([o[:3] for o in out])


class CountingLibrary:
    """The device library with a count of what its calls enqueue: one kernel per call; a per-frame contrast is a memset and two."""

    def __init__(self, lib):
        self._lib, self.kernels, self.memsets = lib, 0, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def counted(*a, **k):
            contrast = name == "color_adjust" and a[2] == "contrast"
            self.kernels += 2 if contrast else 1
            self.memsets += int(contrast)
            return fn(*a, **k)
        return counted


class TorchDeviceOps(TorchDispatchMode):
    """Counts what torch itself sends to the device: host-to-device copies, and every other non-view, non-allocating operation
    with a device result (fills, dtype conversions, copies) as one launch."""
    FREE = ("aten.empty", "aten.new_empty", "aten.detach", "aten.alias", "aten.lift_fresh", "aten.is_pinned", "aten._pin_memory")

    def __init__(self):
        super().__init__()
        self.h2d, self.launches = 0, 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        ins = [t for t in tree_flatten((args, kwargs))[0] if isinstance(t, torch.Tensor)]
        if any(isinstance(t, torch.Tensor) and t.is_cuda for t in tree_flatten(out)[0]):
            if any(not t.is_cuda for t in ins):
                self.h2d += 1
            elif not func.is_view and not str(func).startswith(self.FREE):
                self.launches += 1
        return out


def count(path, batch):
    lib = CountingLibrary(hip.library())
    hip.set_library(lib)
    try:
        with TorchDeviceOps() as ops:
            path(*batch)
    finally:
        hip.set_library(lib._lib)
    torch.cuda.synchronize()
    return {"launches": lib.kernels + lib.memsets + ops.launches, "library_kernels": lib.kernels, "library_memsets": lib.memsets,
            "torch_device_ops": ops.launches, "host_to_device_copies": ops.h2d}


def main():
    assert torch.cuda.is_available(), "augbatch_bench needs the GPU: a time taken elsewhere says nothing"
    batch = make_batch()
    a, b = per_frame(*batch), batched(*batch)
    assert all(torch.equal(a[k], b[k]) for k in a), "the two paths disagree"
    paths = {"per_frame": per_frame, "batch": batched}
    ms = {k: [] for k in paths}
    for _ in range(REPEATS):
        for _ in range(WARMUP):
            for fn in paths.values():
                fn(*batch)
        torch.cuda.synchronize()
        spent = {k: 0.0 for k in paths}
        for _ in range(BATCHES):
            for k, fn in paths.items():                                 # alternating: both see the same machine
                t0 = time.perf_counter()
                fn(*batch)
                torch.cuda.synchronize()
                spent[k] += time.perf_counter() - t0
        for k in paths:
            ms[k].append(round(spent[k] / BATCHES * 1e3, 4))
    res = {"tool": "tools/augbatch_bench.py", "device": torch.cuda.get_device_name(0), "frames": B, "frame_hw": [H, W],
           "warmup": WARMUP, "batches": BATCHES, "outputs_equal": True}
    for k, fn in paths.items():
        res[k] = dict(count(fn, batch), ms_per_batch=ms[k], ms_per_batch_median=sorted(ms[k])[len(ms[k]) // 2])
    res["speedup_median"] = round(res["per_frame"]["ms_per_batch_median"] / res["batch"]["ms_per_batch_median"], 3)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "augment_batch_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

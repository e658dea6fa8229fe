#!/usr/bin/env python3
"""The train step on a stream of AUGMENTED batch shapes: bf16, B = 8, the shape stream of DeviceAugment(seed=0)
on 720 x 1280 frames, synthetic frames (synth.synth_batch with the items' sizes).  Every arm sees the same stream and gets its
own model:

    a   graph=False, raw shapes                         what a user had to do before shape buckets
    b   graph=True,  raw shapes, default cache          every miss costs a capture (two warm-up passes + the capture pass)
    c   graph=True,  max_graphs=16, every batch of the stream padded to its bucket of 64 (F.pad on the collated batch: the same
        tensors device_collate(pad_to=64) would hand the step; the collate itself is not part of this tool)

    python tools/varshape_bench.py --arms a,a,b,c [--steps 200] [--steps-b 40] [--max-size 1024] [--json out.json]
    python tools/varshape_bench.py --largest            one eager step of the largest bucket of the stream, nothing else
    python tools/varshape_bench.py --lsap [--old-lib parent.so]     gwd_lsap at the benchmark's problem (L=6, B=8, Q=100, 7 targets)

--max-size caps the longer side of every augmented frame (DeviceAugment's max_size, 1024 in the reference's chain): the stream
reaches 8 x 1024 x 1024 at the default, 1.7 x the pixels of the 16 x 480 x 640 step.

The clock: the batches of a chunk (--chunk steps) are generated and uploaded first, then the chunk's steps run with ONE synchronise
at its end; an arm's whole-stream time is the sum over its chunks, captures included.  Inside a chunk every step's kind (replay /
capture + replay / eager) comes from TrainStep.graph_stats() and its HOST time is kept: a capture ends in synchronising calls, so its
host time is its cost; ms per replayed step = (whole-stream time - host time of the other steps) / replays."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gw_depth_amd import Config, build_model, hip  # noqa: E402
from gw_depth_amd.data import bucket_shape  # noqa: E402
from gw_depth_amd.engine import TrainStep  # noqa: E402
from gw_depth_amd.synth import det_fill_, synth_batch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shape_census import item_shape_stream, lru_hit_rate  # noqa: E402

SRC_W, SRC_H, BATCH = 1280, 720, 8


def make_step(**kw):
    cfg = Config(device="cuda", dropout=0.1, log_depth_error=True)
    model, crits, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda()
    crits[0].cuda()
    return TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, **kw)


def raw_batch(i, shapes):
    """Batch i of the stream at its raw padded size, on the device."""
    H, W = max(s[0] for s in shapes), max(s[1] for s in shapes)
    b = synth_batch(BATCH, H, W, seed=1000 + i, n_lines=7, sizes=shapes)
    out = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    out["targets"] = [{k: v.cuda() for k, v in t.items()} for t in b["targets"]]
    return out


def to_bucket(b, step):
    """The same batch collated to its bucket: more zero pixels, mask True, depth 0, label 0 at the bottom and the right."""
    h, w = b["images"].shape[-2:]
    H, W = bucket_shape(h, w, step)
    pad = (0, W - w, 0, H - h)
    return {"images": F.pad(b["images"], pad), "pad_mask": F.pad(b["pad_mask"], pad, value=True), "depth": F.pad(b["depth"], pad),
            "seg": F.pad(b["seg"], pad), "targets": b["targets"]}


def run_arm(arm, stream, chunk):
    kw = {"a": dict(graph=False), "b": dict(graph=True), "c": dict(graph=True, max_graphs=16)}[arm]
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    step = make_step(**kw)
    total_s, kinds, host_ms, keys = 0.0, [], [], []
    for c0 in range(0, len(stream), chunk):
        batches = [raw_batch(i, stream[i]) for i in range(c0, min(c0 + chunk, len(stream)))]
        if arm == "c":
            batches = [to_bucket(b, 64) for b in batches]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            before = step.graph_stats()
            h0 = time.perf_counter()
            step(b)
            host_ms.append(1000 * (time.perf_counter() - h0))
            after = step.graph_stats()
            kinds.append("capture" if after["captures"] > before["captures"] else ("replay" if after["replays"] > before["replays"] else "eager"))
            keys.append(tuple(b["images"].shape[-2:]))
        step.flush()
        torch.cuda.synchronize()
        total_s += time.perf_counter() - t0
        del batches
        print("[%s] %d/%d steps, %.1f ms/step so far" % (arm, len(kinds), len(stream), 1000 * total_s / len(kinds)), file=sys.stderr, flush=True)
    n = len(kinds)
    cap = [m for k, m in zip(kinds, host_ms) if k == "capture"]
    other = sum(m for k, m in zip(kinds, host_ms) if k != "replay")
    replays = kinds.count("replay")
    st = step.graph_stats()
    res = {"arm": arm, "settings": {k: v for k, v in kw.items()}, "pad_to": 64 if arm == "c" else None, "steps": n,
           "ms_per_step_whole_stream": round(1000 * total_s / n, 2),
           "ms_per_replayed_step": round((1000 * total_s - other) / replays, 2) if replays else None,
           "ms_per_capture": round(sum(cap) / len(cap), 1) if cap else None,
           "ms_per_eager_step_host": round(sum(m for k, m in zip(kinds, host_ms) if k == "eager") / max(kinds.count("eager"), 1), 2) if "eager" in kinds else None,
           "hit_rate": round(replays / n, 4), "distinct_shapes": len(set(keys)), "graph_stats": st,
           "lru_model_hit_rate": round(lru_hit_rate(keys, step._cache.bound()), 4) if kw["graph"] else None,
           "peak_reserved_gb": round(torch.cuda.max_memory_reserved() / 2 ** 30, 2)}
    del step
    return res


def largest(stream):
    """One eager step of the largest bucket the stream reaches, alone."""
    H, W = bucket_shape(max(s[0] for sh in stream for s in sh), max(s[1] for sh in stream for s in sh), 64)
    step = make_step(graph=False)
    b = raw_batch(0, [(H, W)] * BATCH)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, total, _ = step(b)
    torch.cuda.synchronize()
    return {"largest_bucket": [BATCH, H, W], "eager_step_ms_first": round(1000 * (time.perf_counter() - t0), 1), "loss": float(total),
            "finite": bool(torch.isfinite(total)), "peak_reserved_gb": round(torch.cuda.max_memory_reserved() / 2 ** 30, 2)}


def lsap_timing(old_lib, reps=200, series=5):
    """gwd_lsap at the benchmark's problem on this build and (--old-lib: a shared library holding another build's gwd_lsap) on that
    one, back to back in one process, alternating: `series` series of `reps` launches each, one event pair per series."""
    L_, B, Q, T = 6, 8, 100, 7
    g = torch.Generator().manual_seed(5)
    cost = (torch.rand(L_, B, Q, 64, generator=g) * 5 - 1).cuda()
    off = torch.tensor([T * i for i in range(B + 1)], dtype=torch.int32, device="cuda")
    outs = {}
    libs = {"this": ctypes.CDLL(hip.library().lib._name)}      # a handle of its own: the project's keeps its argtypes
    if old_lib:
        libs["other"] = ctypes.CDLL(os.path.abspath(old_lib))
    for lib in libs.values():
        lib.gwd_lsap.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 5 + [ctypes.c_void_p]
        lib.gwd_lsap.restype = ctypes.c_int
    stream = torch.cuda.current_stream().cuda_stream

    def launch(name):
        out = outs.setdefault(name, torch.empty((L_, 64), dtype=torch.int32, device="cuda"))
        rc = libs[name].gwd_lsap(cost.data_ptr(), off.data_ptr(), out.data_ptr(), L_, B, Q, 64, 64, stream)
        assert rc == 0, rc

    res = {k: [] for k in libs}
    for name in libs:
        for _ in range(10):
            launch(name)
    torch.cuda.synchronize()
    for _ in range(series):
        for name in libs:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                launch(name)
            e.record()
            torch.cuda.synchronize()
            res[name].append(round(1000 * s.elapsed_time(e) / reps, 2))
    same = torch.equal(outs["this"], outs["other"]) if "other" in outs else None
    return {"problem": "L=6 B=8 Q=100, 7 targets per image, capacity 64", "us_per_launch": res, "same_assignment": same, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="a,a,b,c")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--steps-b", type=int, default=40)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--max-size", type=int, default=1024)
    ap.add_argument("--largest", action="store_true")
    ap.add_argument("--lsap", action="store_true")
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available() and not getattr(hip.library(), "is_fake", False)
    stream = item_shape_stream(SRC_W, SRC_H, BATCH, a.steps, seed=0, max_size=a.max_size)
    out = {"stream": "DeviceAugment(seed=0) on %dx%d, B=%d, bf16, max_size %d" % (SRC_H, SRC_W, BATCH, a.max_size)}
    if a.largest:
        out["largest"] = largest(stream)
    elif a.lsap:
        out["lsap"] = lsap_timing(a.old_lib)
    else:
        out["arms"] = []
        for arm in a.arms.split(","):
            out["arms"].append(run_arm(arm, stream[:a.steps_b] if arm == "b" else stream, a.chunk))
            print(json.dumps(out["arms"][-1]), flush=True)
            if a.json:                       # after every arm: a later arm that fails leaves the earlier ones on disk
                with open(a.json, "w") as f:
                    json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

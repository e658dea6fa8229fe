#!/usr/bin/env python
"""Feeding rate of the dataset loaders against the train step, measured in one run on one GPU.

Writes a synthetic dataset (tools/make_synth_dataset.py: 64 samples of 720 x 1280 by default), then reports as ONE JSON line:

    decode_ms_per_sample     on one worker, split image / depth / labels / json (+ the copy into shared memory)
    samples_per_s            through DecodePool with 1, 4, 8 and 15 workers
    store                    FrameStore.build time and nbytes, device and pinned
    batch_ms                 frames() + assemble_batch per batch of B = 8 under DeviceAugment(train=True, seed=0), for the store in
                             HBM, the store in pinned memory and StreamSource: host-timed (wall time per batch of a whole epoch,
                             device drained at its end) and device-timed (events around one batch at a time, the device idle before)
    step_ms                  eager TrainStep steps of the same run: on bench.py's synthetic batch and on the loader's own batches

    python tools/loader_bench.py [--out profiles/loader_bench.json]

Every pool is started before this process initialises the GPU."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gw_depth_amd import decode


def synth_tool():
    spec = importlib.util.spec_from_file_location("make_synth_dataset", os.path.join(ROOT, "tools", "make_synth_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def decode_rates(index, worker_counts, passes):
    """({part: ms per sample on one worker}, {workers: samples/s}); each pool decodes the whole dataset `passes` times after a warm-up
    pass (page cache, worker start)."""
    split, rates = {}, {}
    n = len(index)
    for w in worker_counts:
        with decode.DecodePool(index, workers=w) as pool:
            for _ in pool.map(range(min(n, 2 * pool.workers))):
                pass
            sums = {}
            t0 = time.perf_counter()
            for _ in range(passes):
                for r in pool.map(range(n)):
                    for k, v in r.timings.items():
                        sums[k] = sums.get(k, 0.0) + v
            el = time.perf_counter() - t0
            rates[str(pool.workers)] = round(passes * n / el, 1)
            if pool.workers == 1:
                split = {k: round(1e3 * v / (passes * n), 3) for k, v in sums.items()}
                split["total"] = round(1e3 * el / (passes * n), 3)
    return split, rates


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", default=None, help="dataset directory (default: a temporary one, removed afterwards)")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[720, 1280])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 4, 8, 15])
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    tmp = None
    root = a.dir
    if root is None:
        tmp = tempfile.TemporaryDirectory(prefix="gwd_loader_bench_")
        root = tmp.name
    synth = synth_tool()
    t0 = time.perf_counter()
    if not os.path.exists(os.path.join(root, "train.txt")):
        synth.write_dataset(root, a.n, [tuple(a.size)], seed=0, jobs=min(16, len(os.sched_getaffinity(0))))
    res = {"samples": a.n, "size": a.size, "batch": a.batch, "cpus": len(os.sched_getaffinity(0)), "write_dataset_s": round(time.perf_counter() - t0, 1)}
    index = decode.GlassRGBDIndex(**synth.index_args(root))
    res["png_bytes_per_sample"] = int(sum(os.path.getsize(p) for i in range(len(index)) for p in index.paths(i)[:3]) / len(index))
    print("dataset written", res, file=sys.stderr, flush=True)

    res["decode_ms_per_sample"], res["samples_per_s"] = decode_rates(index, a.workers, a.passes)
    print("decode measured", res["samples_per_s"], file=sys.stderr, flush=True)
    pool = decode.DecodePool(index)                                  # the pool of the rest of the run: up before the GPU is
    res["pool_workers"] = pool.workers

    import torch
    from gw_depth_amd import Config, build_model, data, dataset
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import det_fill_, synth_batch
    assert not torch.cuda.is_initialized()
    sync = torch.cuda.synchronize

    sources, res["store"] = {}, {}
    for where in ("device", "pinned"):
        sync()
        t0 = time.perf_counter()
        sources["store-" + where] = s = dataset.FrameStore.build(index, pool, device="cuda", where=where)
        sync()
        res["store"][where] = {"build_s": round(time.perf_counter() - t0, 3), "nbytes": s.nbytes}
    sources["stream"] = dataset.StreamSource(index, pool, device="cuda")

    def loader_of(source):
        return dataset.TrainLoader(source, a.batch, data.DeviceAugment(train=True, seed=0), pad_to=64)

    res["batch_ms"] = {}
    for name, source in sources.items():
        loader = loader_of(source)
        for b in loader:                                             # warm-up epoch: allocator, table caches, page cache
            pass
        sync()
        nb = 0
        t0 = time.perf_counter()
        for e in range(a.epochs):
            loader.set_epoch(e + 1)
            for b in loader:
                nb += 1
        sync()
        host_ms = 1e3 * (time.perf_counter() - t0) / nb
        spans = []
        loader.set_epoch(a.epochs + 1)
        it = iter(loader)
        while True:
            sync()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            if next(it, None) is None:
                break
            end.record()
            sync()
            spans.append(start.elapsed_time(end))
        res["batch_ms"][name] = {"host": round(host_ms, 2), "device": round(sum(spans) / len(spans), 2), "batches": nb}
        print(name, res["batch_ms"][name], file=sys.stderr, flush=True)

    cfg = Config(device="cuda", dropout=0.1, log_depth_error=True)
    model, crits, _ = build_model(cfg)
    model.load_state_dict(det_fill_({k: v.detach().clone() for k, v in model.state_dict().items()}, seed=0))
    model.cuda()
    crits[0].cuda()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=False)
    b = synth_batch(a.batch, 480, 640, seed=1)
    fixed = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    fixed["targets"] = [{k: v.cuda() for k, v in t.items()} for t in b["targets"]]

    def timed(batches, warmup):
        for bb in batches[:warmup]:
            step(bb)
        sync()
        t0 = time.perf_counter()
        for bb in batches[warmup:]:
            step(bb)
        sync()
        return round(1e3 * (time.perf_counter() - t0) / (len(batches) - warmup), 2)

    res["step_ms"] = {"eager_bf16_synthetic_480x640": timed([fixed] * (a.steps + 2), 2)}
    loader = loader_of(sources["store-device"])
    own = [bb for _, bb in zip(range(a.steps + 2), loader)]
    res["step_ms"]["eager_bf16_loader_batches"] = timed(own, 2)
    res["step_ms"]["loader_batch_shapes"] = sorted({tuple(bb["images"].shape[2:]) for bb in own})
    loader.set_epoch(1)
    sync()
    t0 = time.perf_counter()
    k = 0
    for bb in loader_of(sources["stream"]):                          # the loop a training driver runs: stream, assemble, step
        step(bb)
        k += 1
    sync()
    res["step_ms"]["stream_loader_plus_eager_step"] = round(1e3 * (time.perf_counter() - t0) / k, 2)
    pool.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""How many padded batch shapes the training augmentation produces, and how a bounded cache of captured steps fares on them
(DESIGN.md §13).  CPU only: the shape stream is DeviceAugment.params' size arithmetic, deterministic given the seed.

    python tools/shape_census.py [--batches 2000] [--seed 0] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gw_depth_amd.data import DeviceAugment, padded_size, resized_shape  # noqa: E402


def augmented_shape(p, w, h):
    """(h, w) of a (w, h) frame behind the transform chain `p` of DeviceAugment.params - the size arithmetic of apply() alone."""
    for step in p["steps"]:
        if step[0] == "resize":
            h, w = resized_shape(w, h, step[1], step[2])
        else:
            h, w = int(step[1][2]), int(step[1][3])
    return int(h), int(w)


def item_shape_stream(w, h, batch, batches, seed=0, max_size=1024):
    """The (h, w) of every item of `batches` consecutive training batches of `batch` (w, h) frames under DeviceAugment(train=True,
    seed): a list of lists.  Pure host arithmetic, deterministic given the seed."""
    aug = DeviceAugment(train=True, max_size=max_size, seed=seed)
    return [[augmented_shape(aug.params(w, h), w, h) for _ in range(batch)] for _ in range(batches)]


def batch_shape_stream(w, h, batch, batches, seed=0, pad_to=None, max_size=1024):
    """The padded (H, W) of the batches of item_shape_stream: what device_collate(pad_to=pad_to) makes of them."""
    return [padded_size(max(s[0] for s in shapes), max(s[1] for s in shapes), pad_to)
            for shapes in item_shape_stream(w, h, batch, batches, seed=seed, max_size=max_size)]


def lru_hit_rate(keys, capacity):
    """Fraction of `keys` found in a least-recently-used cache of `capacity` entries that admits every miss."""
    from collections import OrderedDict
    cache, hits = OrderedDict(), 0
    for k in keys:
        if k in cache:
            cache.move_to_end(k)
            hits += 1
        else:
            if len(cache) >= capacity:
                cache.popitem(last=False)
            cache[k] = True
    return hits / max(len(keys), 1)


# (source w, source h, batch size, steps to try, cache sizes to try)
ROWS = [(1280, 720, 8, (None, 32, 64, 128), (6, 16)),
        (1280, 720, 2, (None, 64), (6, 16, 32, 64)),
        (640, 480, 8, (None, 64), (6, 16))]


def census(w, h, batch, step, caches, batches, seed):
    raw = batch_shape_stream(w, h, batch, batches, seed=seed)
    got = batch_shape_stream(w, h, batch, batches, seed=seed, pad_to=step)
    extra = sum(a * b for a, b in got) / sum(a * b for a, b in raw) - 1.0
    return {"source": "%dx%d" % (h, w), "batch": batch, "step": step, "distinct": len(set(got)), "extra_pixels": extra,
            "lru_hit": {str(c): lru_hit_rate(got, c) for c in caches}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = [census(w, h, b, s, caches, a.batches, a.seed) for w, h, b, steps, caches in ROWS for s in steps]
    print("| source, batch | rounding | distinct (H, W) | extra pixels | LRU hit rates |")
    print("|---|---|---|---|---|")
    for r in rows:
        hits = ", ".join("LRU-%s %.1f %%" % (c, 100 * v) for c, v in r["lru_hit"].items())
        print("| %s, B=%d | %s | %d | %s | %s |" % (r["source"], r["batch"], "none" if r["step"] is None else "up to %d" % r["step"], r["distinct"],
                                                "none" if r["step"] is None else "+%.1f %%" % (100 * r["extra_pixels"]), hits))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"batches": a.batches, "seed": a.seed, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Writes a small synthetic dataset in GW-Depth's directory layout (what gw_depth_amd.decode.GlassRGBDIndex reads), with Pillow:

    DIR/images/<name>.png   8-bit RGB: smooth gradients plus noise (not trivially compressible)
    DIR/depth/<name>.png    16-bit depth in millimetres (mode I;16) with holes; 0 and 65535 both occur
    DIR/seg/<name>.png      glass labels, alternately mode L and mode P
    DIR/lines/<name>.json   labelme-style polygons ('shapes': closed polygons with 'points' and 'poly_id'; one polygon without
                            points in every sample that has shapes; the LAST sample has no shapes at all), 'imageId', image size
    DIR/train.txt, DIR/val.txt   one sample per line, name first (further tokens and blank lines as real lists have them)
    DIR/images.json         {'images': [{'id', 'file_name'}]}

    python tools/make_synth_dataset.py DIR --n 64 --size 720 1280            every sample 720 x 1280
    python tools/make_synth_dataset.py DIR --n 7 --size 45 61 --size 64 48   sizes in turn
    python tools/make_synth_dataset.py DIR --n 9 --size 480 640 --ragged     sizes derived from the one given, in turn

Seeded and deterministic: the same arguments write the same bytes."""
import argparse
import json
import os

import numpy as np
from PIL import Image, ImageDraw


def ragged_sizes(h, w):
    """Three sizes from one: the size itself, a shorter and wider one, a narrower one."""
    return [(h, w), (max(1, h - h // 8), w + w // 6), (h + h // 24, max(1, w - w // 5))]


def _polygons(rng, h, w, count):
    """`count` convex polygons (3..6 vertices, clockwise around a centre) inside the frame, as float pixel coordinates."""
    polys = []
    for _ in range(count):
        cx, cy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h
        rx, ry = rng.uniform(0.08, 0.3) * w, rng.uniform(0.08, 0.3) * h
        k = int(rng.integers(3, 7))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        pts = [[float(np.clip(cx + rx * np.cos(a), 0, w - 1)), float(np.clip(cy + ry * np.sin(a), 0, h - 1))] for a in ang]
        polys.append([[round(x, 2), round(y, 2)] for x, y in pts])
    return polys


def write_sample(root, name, k, h, w, rng, with_shapes=True):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    phase = rng.uniform(0, 2 * np.pi, 3)
    rgb = np.stack([127 + 90 * np.sin(xx / max(w, 2) * 3.1 + yy / max(h, 2) * (1.3 + c) + phase[c]) for c in range(3)], axis=-1)
    rgb = np.clip(rgb + rng.normal(0, 6, rgb.shape), 0, 255).astype(np.uint8)
    depth = 800 + 4000 * (yy / max(h, 2)) + 1500 * np.cos(xx / max(w, 2) * 2.0 + phase[0]) + rng.normal(0, 12, (h, w))
    depth = np.clip(depth, 1, 65534).astype(np.uint16)
    holes = rng.random((h, w)) < 0.03
    depth[holes] = 0
    depth.flat[0] = 0
    depth.flat[depth.size - 1] = 65535
    polys = _polygons(rng, h, w, int(rng.integers(2, 5))) if with_shapes else []
    mask = Image.new("L", (w, h), 0)
    draw = ImageDraw.Draw(mask)
    for j, pts in enumerate(polys):
        draw.polygon([tuple(p) for p in pts], fill=1 + j % 3)
    if k % 2:                                                 # every other label image is paletted: the stored byte is the label
        mask = mask.convert("P")
        mask.putpalette([0, 0, 0, 255, 0, 0, 0, 255, 0, 0, 0, 255] + [0] * (252 * 3))
    Image.fromarray(rgb).save(os.path.join(root, "images", name + ".png"))
    Image.fromarray(depth).save(os.path.join(root, "depth", name + ".png"))
    mask.save(os.path.join(root, "seg", name + ".png"))
    shapes = [{"label": "glass", "points": pts, "poly_id": j, "shape_type": "polygon"} for j, pts in enumerate(polys)]
    if with_shapes:
        shapes.insert(1, {"label": "glass", "points": [], "poly_id": len(polys), "shape_type": "polygon"})
    with open(os.path.join(root, "lines", name + ".json"), "w") as f:
        json.dump({"imageId": 1000 + k, "imagePath": name + ".png", "imageHeight": h, "imageWidth": w, "shapes": shapes}, f)


def _write_one(job):
    root, name, k, h, w, seed, with_shapes = job
    write_sample(root, name, k, h, w, np.random.default_rng([seed, k]), with_shapes=with_shapes)


def write_dataset(root, n, sizes, seed=0, jobs=1):
    """Writes n samples with `sizes` [(h, w), ...] in turn (every sample from its own seeded generator, so `jobs` processes write the
    same bytes as one); returns the keyword arguments of GlassRGBDIndex for the train list."""
    for d in ("images", "depth", "seg", "lines"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names = ["s%04d" % k for k in range(n)]
    todo = [(root, name, k, int(sizes[k % len(sizes)][0]), int(sizes[k % len(sizes)][1]), seed, not (n > 1 and k == n - 1))
            for k, name in enumerate(names)]
    if jobs > 1:
        from concurrent.futures import ProcessPoolExecutor
        with ProcessPoolExecutor(max_workers=jobs) as ex:
            list(ex.map(_write_one, todo))
    else:
        for job in todo:
            _write_one(job)
    for split in ("train", "val"):
        with open(os.path.join(root, split + ".txt"), "w") as f:
            for k, name in enumerate(names):
                f.write(name + (" 518.86\n" if k % 2 else "\n") + ("\n" if k == 1 else ""))
    with open(os.path.join(root, "images.json"), "w") as f:
        json.dump({"images": [{"id": 1000 + k, "file_name": name + ".png"} for k, name in enumerate(names)]}, f)
    return index_args(root)


def index_args(root, split="train"):
    return {"data_path": os.path.join(root, "images"), "gt_depth_path": os.path.join(root, "depth"), "gt_seg_path": os.path.join(root, "seg"),
            "gt_line_path": os.path.join(root, "lines"), "filenames_file": os.path.join(root, split + ".txt"),
            "images_json": os.path.join(root, "images.json")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, action="append", metavar=("H", "W"))
    ap.add_argument("--ragged", action="store_true", help="derive three sizes from the (first) --size and use them in turn")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--jobs", type=int, default=1, help="processes that write samples side by side")
    a = ap.parse_args()
    sizes = [tuple(s) for s in (a.size or [[480, 640]])]
    if a.ragged:
        sizes = ragged_sizes(*sizes[0])
    print(json.dumps(write_dataset(a.dir, a.n, sizes, a.seed, a.jobs)))


if __name__ == "__main__":
    main()

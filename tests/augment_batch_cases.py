"""The seven frames of the batched-augmentation tests (tests/test_augment_batch.py on the CPU stand-in,
tests/test_augment_batch_gpu.py through the kernels) and the two references every batch is compared with: DeviceAugment.apply
frame by frame and the oracle chain step by step.  The smallest shapes that reach every branch of DeviceAugment.apply_batch;
the contrast sits in jitter slot 0, 1, 2, 3 and 0 of frames 0, 1, 2, 3 and 5.  Everything is integer equality."""
import functools

import numpy as np
import torch

from gw_depth_amd import data
from oracle import pil_color_ref as C
from oracle import pil_resize_ref as ref

CASES = [
    # (h, w), params                                                                                   what it reaches
    ((72, 128), {"flip": None, "steps": [("resize", 96, 1024)],                                        # upscale, ksize 3
                 "jitter": [("contrast", 1.3), ("brightness", 0.7), ("saturation", 1.2), ("hue", 0.1)]}),
    ((61, 97), {"flip": "h", "steps": [("resize", 120, 160)],                                          # odd sizes, max-size clamp
                "jitter": [("hue", -0.3), ("contrast", 0.8), ("brightness", 1.25), ("saturation", 0.6)]}),
    ((72, 128), {"flip": "v", "steps": [("resize", 80, None), ("crop", (5, 9, 50, 61)), ("resize", 100, 1024)],   # two stages, windowed
                 "jitter": [("saturation", 1.4), ("brightness", 0.9), ("contrast", 1.1), ("hue", 0.37)]}),
    ((90, 50), {"flip": "h", "steps": [("resize", 70, None), ("crop", (0, 0, 40, 40)), ("resize", 64, 1024)],     # portrait, window at 0
                "jitter": [("brightness", 1.1), ("hue", -0.05), ("saturation", 0.75), ("contrast", 0.65)]}),
    ((72, 128), {"flip": "v", "steps": []}),                                                           # RGB through the gather
    ((72, 128), {"flip": None, "steps": [],                                                            # copy, then jitter
                 "jitter": [("contrast", 0.9), ("saturation", 1.0), ("hue", 0.0), ("brightness", 1.4)]}),
    ((128, 128), {"flip": None, "steps": [("resize", (128, 20), None)]}),                              # vertical pass only, ksize 15
]
N = len(CASES)
ADJUST = {"brightness": C.adjust_brightness, "contrast": C.adjust_contrast, "saturation": C.adjust_saturation, "hue": C.adjust_hue}


@functools.lru_cache(maxsize=None)
def frame(k):
    """Seeded inputs of frame k: rgb, depth_mm, labels (numpy), lines, poly_ids, centres (host tensors)."""
    (h, w), _ = CASES[k]
    rng = np.random.default_rng(100 + k)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    dep = rng.integers(0, 12000, (h, w)).astype(np.int32)
    lab = rng.integers(0, 3, (h, w)).astype(np.uint8)
    frac = torch.tensor([[0.08, 0.28, 0.78, 0.83], [0.04, 0.07, 0.04, 0.97], [0.0, 0.99, 0.99, 0.0], [0.94, 0.14, 0.98, 0.17],
                         [0.30, 0.30, 0.60, 0.30], [0.60, 0.30, 0.45, 0.70], [0.45, 0.70, 0.30, 0.30]])
    lines = (frac * torch.tensor([w, h, w, h], dtype=torch.float32)).round()
    ids = torch.tensor([0, 0, 1, 1, 2, 2, 2])
    centres = torch.stack([data.chain_points(lines[ids == i]).mean(0) for i in ids.tolist()])
    for a in (rgb, dep, lab):
        a.setflags(write=False)
    return rgb, dep, lab, lines, ids, centres


@functools.lru_cache(maxsize=None)
def oracle_images(k):
    """Frame k through the oracle, one new image per step as the reference's Compose makes them."""
    rgb, dep, lab = frame(k)[:3]
    p = CASES[k][1]
    if p["flip"] == "h":
        rgb, dep, lab = rgb[:, ::-1], dep[:, ::-1], lab[:, ::-1]
    if p["flip"] == "v":
        rgb, dep, lab = rgb[::-1], dep[::-1], lab[::-1]
    rgb, dep, lab = np.ascontiguousarray(rgb), np.ascontiguousarray(dep), np.ascontiguousarray(lab)
    for step in p["steps"]:
        h, w = rgb.shape[:2]
        if step[0] == "resize":
            oh, ow = data.resized_shape(w, h, step[1], step[2])
            if (oh, ow) != (h, w):
                rgb, dep, lab = ref.resize_bilinear_u8(rgb, oh, ow), ref.resize_nearest(dep, oh, ow), ref.resize_nearest(lab, oh, ow)
        else:
            i, j, ch, cw = step[1]
            rgb, dep, lab = (np.ascontiguousarray(a[i:i + ch, j:j + cw]) for a in (rgb, dep, lab))
    for name, f in p.get("jitter", []):
        rgb = ADJUST[name](rgb, f)
    return rgb, dep, lab


def device_frames(indices, device, depth=True, labels=True):
    out = []
    for k in indices:
        rgb, dep, lab = (torch.from_numpy(a.copy()).to(device) for a in frame(k)[:3])
        out.append((rgb, dep if depth else None, lab if labels else None))
    return out


def check_batch(indices, device, depth=True, labels=True, full=True):
    """apply_batch over the frames `indices` == apply frame by frame == the oracle chain; the inputs stay as they were."""
    frames = device_frames(indices, device, depth, labels)
    lines = [frame(k)[3] for k in indices]
    params = [CASES[k][1] for k in indices]
    ids = [frame(k)[4] for k in indices] if full else None
    centres = [frame(k)[5] for k in indices] if full else None
    got = data.DeviceAugment.apply_batch(frames, lines, params, poly_ids=ids, centres=centres)
    assert len(got) == len(indices)
    for n, k in enumerate(indices):
        fresh = device_frames([k], device, depth, labels)[0]
        for a, b in zip(frames[n], fresh):                              # the caller's tensors are unmodified
            assert (a is None and b is None) or torch.equal(a, b), (k, "input modified")
        want = data.DeviceAugment.apply(*fresh, lines[n], params[n], **({"poly_ids": ids[n], "centres": centres[n]} if full else {}))
        assert len(got[n]) == len(want) == (6 if full else 5)
        for j, (g, w_) in enumerate(zip(got[n], want)):
            if w_ is None:
                assert g is None, (k, j)
                continue
            assert g.dtype == w_.dtype and g.shape == w_.shape and g.device == w_.device, (k, j, g.shape, w_.shape)
            assert torch.equal(g, w_), (k, j)
        for j, o in enumerate(oracle_images(k)):
            if got[n][j] is not None:
                assert got[n][j].is_contiguous()
                np.testing.assert_array_equal(got[n][j].cpu().numpy(), o, err_msg="frame %d output %d" % (k, j))
    return got

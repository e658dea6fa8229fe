"""The fp64 restatement of gwd_dense_postprocess_resized (include/gwdepth.h) in plain torch, and the seeded inputs the kernel
tests share with the CPU tests that vouch for them.

Source sample: s = san(depth) (below min -> min, above max -> max, +inf -> max, NaN -> min); with a twin the mean of the image's
sample and its twin's at the column mirrored inside the un-padded width, and the logits summed class by class.  Resize: the
rule of F.interpolate(mode="bilinear", align_corners=False) over the un-padded h x w region with exact integer coordinates
    n = max((2 d + 1) h - fh, 0), i0 = n // (2 fh), lambda = (n % (2 fh)) / (2 fh), i1 = min(i0 + 1, h - 1)
rows first, then columns; a tap of weight zero does not enter the result.  Millimetres: round(depth * 1000) in [0, 65535].
Label: argmax of the two interpolated logits, tie -> 0, a NaN is the maximum, the first one wins.  Outside a frame: 0 / 0 / 255."""
import torch

U = 2.0 ** -24          # unit round-off of fp32
K = 10                  # see tests/test_frames_post_gpu.py


def san(d, lo, hi):
    d = d.double()
    return torch.where(torch.isnan(d), torch.full_like(d, lo), d.clamp(lo, hi))


def taps(n_out, n_in):
    """(i0, i1, lambda) of every output index: exact integers, lambda the fp64 quotient."""
    d = torch.arange(n_out, dtype=torch.int64)
    n = ((2 * d + 1) * n_in - n_out).clamp(min=0)
    i0 = n // (2 * n_out)
    lam = (n % (2 * n_out)).double() / float(2 * n_out)
    return i0, (i0 + 1).clamp(max=n_in - 1), lam


def lerp(a, b, lam):
    return torch.where(lam == 0, a, (1.0 - lam) * a + lam * b)


def resize(src, fh, fw):
    """src (..., h, w) fp64 -> (..., fh, fw)."""
    h, w = src.shape[-2:]
    y0, y1, ly = taps(fh, h)
    x0, x1, lx = taps(fw, w)
    rows = lerp(src[..., y0, :], src[..., y1, :], ly[:, None])
    return lerp(rows[..., x0], rows[..., x1], lx)


def argmax2(l0, l1):
    return ((l1 > l0) | (torch.isnan(l1) & ~torch.isnan(l0))).to(torch.int64)


def dense_resized(depth, seg, sizes, frame_sizes, out_hw, min_depth, max_depth, twin=0):
    """depth (Bs,H,W) or (Bs,1,H,W), seg (Bs,2,H,W), any float dtype; sizes / frame_sizes: B pairs of ints (sizes None = H x W).
    -> depth (B,Fh,Fw) fp64, mm int64, label int64, margin fp64 = |l0 - l1| of the interpolated logits (inf where one is NaN:
    the rule decides there, not the margin)."""
    seg = seg.detach().cpu().double()
    Bs, _, H, W = seg.shape
    depth = depth.detach().cpu().reshape(Bs, H, W)
    B = Bs - twin
    Fh, Fw = out_hw
    out = torch.zeros(B, Fh, Fw, dtype=torch.float64)
    mm = torch.zeros(B, Fh, Fw, dtype=torch.int64)
    label = torch.full((B, Fh, Fw), 255, dtype=torch.int64)
    margin = torch.full((B, Fh, Fw), float("inf"), dtype=torch.float64)
    for b in range(B):
        h, w = (H, W) if sizes is None else (int(v) for v in sizes[b])
        fh, fw = (int(v) for v in frame_sizes[b])
        if fh == 0 or fw == 0:
            continue
        s = san(depth[b, :h, :w], min_depth, max_depth)
        lg = seg[b, :, :h, :w]
        if twin:
            s = 0.5 * (s + san(depth[b + twin, :h, :w], min_depth, max_depth).flip(-1))
            lg = lg + seg[b + twin, :, :h, :w].flip(-1)
        d = resize(s, fh, fw)
        l = resize(lg, fh, fw)
        out[b, :fh, :fw] = d
        mm[b, :fh, :fw] = torch.round(d * 1000.0).clamp(0, 65535).to(torch.int64)
        label[b, :fh, :fw] = argmax2(l[0], l[1])
        m = (l[0] - l[1]).abs()
        margin[b, :fh, :fw] = torch.where(torch.isnan(m), torch.full_like(m, float("inf")), m)
    return out, mm, label, margin


def dense_plain(depth, seg, sizes, min_depth, max_depth):
    """gwd_dense_postprocess restated: no resize, padding 0 / 0 / 255."""
    seg = seg.detach().cpu().double()
    B, _, H, W = seg.shape
    d = san(depth.detach().cpu().reshape(B, H, W), min_depth, max_depth)
    mm = torch.round(d * 1000.0).clamp(0, 65535).to(torch.int64)
    lab = argmax2(seg[:, 0], seg[:, 1])
    for b in range(B):
        h, w = (H, W) if sizes is None else (int(v) for v in sizes[b])
        inside = torch.zeros(H, W, dtype=torch.bool)
        inside[:h, :w] = True
        d[b][~inside], mm[b][~inside], lab[b][~inside] = 0.0, 0, 255
    return d, mm, lab


# ---------------------------------------------------------------------------------------------------------------- shared inputs
MIN_D, MAX_D = 1e-3, 10.0
SEEDS = (3, 4)
# name -> ((H, W), un-padded sizes, frame sizes, output extent).  12 x 20: no 16-byte source loads; 12 x 24: 16-byte source
# loads, image 0 with aligned mirrored groups (w % 8 == 0), image 1 without; extents that are and are not a multiple of 8 pixels;
# up-scaling, down-scaling and one axis each; output rows of more than one workgroup (more than 2048 pixels by eight, more than
# 256 one by one); a source wider than the LDS stage (4096 columns).
SHAPES = {
    "up_vec": ((12, 20), [(12, 20), (9, 13)], [(31, 47), (17, 40)], (31, 48)),
    "up_px": ((12, 20), [(12, 20), (9, 13)], [(31, 47), (17, 40)], (31, 47)),
    "down_px": ((12, 20), [(12, 20), (9, 13)], [(7, 11), (6, 8)], (7, 11)),
    "down_vec": ((12, 20), [(12, 20), (9, 13)], [(7, 11), (6, 8)], (8, 16)),
    "mixed_vec": ((12, 20), [(12, 20), (9, 13)], [(20, 11), (5, 30)], (20, 32)),
    "src16_vec": ((12, 24), [(12, 24), (9, 13)], [(31, 47), (17, 40)], (31, 48)),
    "src16_px": ((12, 24), [(12, 24), (9, 13)], [(7, 11), (17, 40)], (17, 41)),
    "wide_rows_vec": ((3, 40), [(3, 40), (2, 33)], [(4, 2100), (3, 90)], (4, 2104)),
    "wide_rows_px": ((3, 40), [(3, 40), (2, 33)], [(4, 299), (3, 90)], (4, 299)),
    "unstaged_vec": ((3, 4104), [(3, 4104), (2, 4001)], [(5, 4600), (4, 50)], (5, 4608)),
    "unstaged_px": ((3, 4104), [(3, 4104), (2, 4001)], [(2, 301), (4, 50)], (4, 301)),
}


def inputs(seed, shape, twin):
    """bf16-representable values, so that the fp32 and the bf16 kernels see the same numbers: depth in (-0.5, 10.5) (both clamps
    fire), logits N(0, 1).  Everything outside an image's un-padded (h, w) - its twin's too - is NaN or 1e30."""
    (H, W), sizes, frames, out_hw = SHAPES[shape]
    B = len(sizes)
    Bs = 2 * B if twin else B
    g = torch.Generator().manual_seed(seed)
    depth = (torch.rand(Bs, H, W, generator=g) * 11.0 - 0.5).bfloat16().float()
    seg = torch.randn(Bs, 2, H, W, generator=g).bfloat16().float()
    for i in range(Bs):
        h, w = sizes[i % B]
        pad = torch.ones(H, W, dtype=torch.bool)
        pad[:h, :w] = False
        depth[i][pad] = float("nan") if i % 2 == 0 else 1e30
        seg[i, 0][pad] = 1e30
        seg[i, 1][pad] = float("nan")
    return depth, seg, sizes, frames, out_hw


def label_tolerance(seg, sizes, twin):
    """2 K 2^-24 max |logit| over the un-padded regions, doubled under a twin: how far fp32 can move the margin."""
    B = len(sizes)
    top = max(float(torch.nan_to_num(seg[i, :, :sizes[i % B][0], :sizes[i % B][1]].abs(), nan=0.0).max()) for i in range(seg.shape[0]))
    return 2 * K * U * top * (2 if twin else 1)

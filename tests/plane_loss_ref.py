"""fp64 reference, error bound and fp32 model of the plane loss (csrc/planeloss.hip, gwd_plane_loss_forward / _backward: Sobel
normals of a depth map, point-in-triangle masks, the per-plane population variances of both normal components and their gradient;
fp32 or bf16 depth; CPU only, plain module; the instrument is tests/attn_ref.py's, the masks are oracle/plane_ref.py's, whose
boundary rule is pinned against matplotlib).

A case is (dtype, H, W, triangles, n_planes, min_area, valid kind, gloss).  ``inputs(c)`` draws, seeded from the case text, the depth
(smooth plus noise, so that a normal of the wrong pixel is far outside the bound), builds the valid mask (``all``, ``holes``: every
7th pixel and one 3 x 4 block invalid, ``none``) and, for ``random`` triangles, P small triangles.

* ``launch(c)``: plane_blocks and the trips of the forward's grid-stride loop, the backward's blocks (capped at 2048) and trips.
* ``reference(c, inp)`` -> ({loss, n, mean_x, mean_y, active, count, gdepth}, conds), fp64 from the stored depth: normals = negated
  3 x 3 Sobel cross-correlation with zero padding; a plane counts if j < n_planes and area >= min_area (area: valid pixels inside);
  loss = sum (var_x + var_y) / max(1, active); gdepth = gloss d loss / d depth by fp64 autograd.  As the device does, a plane that is
  counted out keeps its area in n and the plain sums in mean_x / mean_y, a plane beyond n_planes has zeros.  With A_x, A_y the sums
  of the absolute stencil terms of a normal (the device forms each normal in fp32 and sums in fp64):
      mean_x:  cond = sum_pixels A_x / n            loss:  cond = sum_active sum_pixels (A_x^2 + A_y^2) / n / max(1, active)
      gdepth:  cond = |scale| sum_taps (|k_x| G_x + |k_y| G_y) at the pixel the tap reads,  G_x = sum_planes (A_x + |mean_x|) / n
  - the absolute values of the terms the transposed stencil adds.  n, active and the count are compared for equality.
      |got - ref| <= C u (|ref| + (2^-24 / u) cond),  u that of the stored type (fp32 for the loss and the statistics)
* ``model(c, inp, defect=None)``: the kernel's arithmetic: the normals in fp32 in the kernel's order of operations, the sums in fp64,
  the backward's per-pixel plane sums in ascending plane order and the eight taps in row order in fp32.  Defects: ``border_clamped``
  (replicated instead of zero padding), ``bwd_untransposed`` (the stencil applied without the flip), ``inactive_counts`` (a
  counted-out plane's pixels enter the gradient), ``beyond_count`` (planes >= n_planes are used), ``area_off_by_one`` (> instead
  of >=), ``stride_once`` (the backward's second grid-stride trip is skipped).

The constants.  ``measure_c()``: largest |model - ref| / bound over the case list per (output, type); C twice that, one decimal up.
CPU, 2026-10:

@TABLE@

(A single rounding to bf16 gives up to 2.0 in this measure.  The loss and the means are fp32 normals summed in fp64 whatever the
depth's type, so both depth types share their constants; the order of the fp64 sums moves a result by about 2^-29 of the bound's
unit.)  A kernel that needs more than its C has a defect or the bound lacks a
term: neither is repaired by raising C.
"""
import types
import zlib

import torch
import torch.nn.functional as F

from oracle import plane_ref
from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("border_clamped", "bwd_untransposed", "inactive_counts", "beyond_count", "area_off_by_one", "stride_once")
THREADS, FWD_PER_BLOCK, FWD_MAX_BLOCKS, BWD_MAX_BLOCKS, PMAX = 256, 1024, 128, 2048, 64          # csrc/planeloss.hip
KX = ((1.0, 0.0, -1.0), (2.0, 0.0, -2.0), (1.0, 0.0, -1.0))
KY = ((1.0, 2.0, 1.0), (0.0, 0.0, 0.0), (-1.0, -2.0, -1.0))
OUTPUTS = ("loss", "mean_x", "mean_y", "gdepth")
EXACT = ("n", "active", "count")


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def launch(c):
    HW = c.H * c.W
    fb = max(1, min(FWD_MAX_BLOCKS, (HW + FWD_PER_BLOCK - 1) // FWD_PER_BLOCK))
    bb = min(BWD_MAX_BLOCKS, (HW + THREADS - 1) // THREADS)
    return types.SimpleNamespace(HW=HW, fwd_blocks=fb, fwd_trips=(HW + fb * THREADS - 1) // (fb * THREADS), bwd_blocks=bb,
                                 bwd_trips=(HW + bb * THREADS - 1) // (bb * THREADS), tail=HW > BWD_MAX_BLOCKS * THREADS)


def count_inside(tri, H, W, valid=None):
    """Valid pixels inside the triangle ((x, y) x 3), by oracle/plane_ref.points_in_triangle."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    m = plane_ref.points_in_triangle(torch.tensor(tri, dtype=torch.int64).view(3, 2), xs, ys)
    return int(m.sum() if valid is None else (m & valid.bool()).sum())


def area_pair(H, W, x0=3, y0=2):
    """Two right triangles whose pixel counts are m and m - 1 -> (m, triangle of m, triangle of m - 1)."""
    seen = {}
    for s in range(3, 14):
        for t in range(3, 14):
            tri = ((x0, y0), (x0 + s, y0), (x0, y0 + t))
            seen.setdefault(count_inside(tri, H, W), tri)
    for m in sorted(seen, reverse=True):
        if m - 1 in seen and m >= 12:
            return m, seen[m], _shift(seen[m - 1], 14, 0)
    raise AssertionError("no pair of areas m, m - 1")


def _shift(tri, dx, dy):
    return tuple((x + dx, y + dy) for x, y in tri)


def _case(kind, dtype, H, W, tris, n_planes, min_area, valid="all", gloss=1.0, P=None):
    c = types.SimpleNamespace(kind=kind, dtype=dtype, H=H, W=W, tris=tris, n_planes=n_planes, min_area=min_area, valid=valid, gloss=gloss)
    c.P = len(tris) if P is None else P
    c.text = "plane_loss %s %s %dx%d P=%d n_planes=%d min_area=%d valid=%s gloss=%g" % (kind, dtype, H, W, c.P, n_planes, min_area, valid, gloss)
    c.id = c.text.replace(" ", "-")
    return c


def _cover(H, W):
    """A triangle (vertices outside the map) that holds every pixel."""
    return ((-1, -1), (2 * W + 1, -1), (-1, 2 * H + 1))


BIG = (((0, 0), (30, 0), (0, 23)), ((30, 23), (2, 23), (30, 3)), ((4, 2), (28, 6), (10, 22)))      # on a 24 x 31 map


def cases():
    out = []
    m, tri_m, tri_m1 = area_pair(24, 31)
    for dt in ("f32", "bf16"):
        for H, W in ((1, 1), (1, 9), (9, 1), (3, 3)):
            out.append(_case("tiny", dt, H, W, (_cover(H, W), ((0, 0), (W, 0), (0, H))), 2, 1))
        # the first triangle's vertices are three corners of the map: border pixels inside
        # (the crossing rule leaves a triangle's top row outside: the third triangle, vertices outside the map, holds all four borders)
        out.append(_case("corners", dt, 24, 31, (BIG[0], ((5, 5), (25, 8), (12, 20)), _cover(24, 31)), 3, 20))
        out.append(_case("corners", dt, 24, 31, (BIG[0], BIG[1]), 2, 20, valid="holes"))
        out.append(_case("degenerate", dt, 24, 31, (((5, 5), (5, 5), (5, 5)), ((2, 2), (10, 10), (20, 20)), tri_m, tri_m1, BIG[2]), 5, m))
        # three triangles share a block of pixels; the fourth lies inside the first and is counted out by its area
        out.append(_case("overlap", dt, 24, 31, (((1, 1), (29, 3), (8, 22)), ((29, 1), (28, 22), (2, 12)), BIG[2], ((8, 5), (13, 5), (8, 9))),
                         4, 40, gloss=3.0))
        out.append(_case("none_counted", dt, 24, 31, BIG, 0, 20))
        out.append(_case("beyond", dt, 24, 31, (((5, 5), (25, 8), (12, 20)), ((1, 1), (12, 2), (3, 15))) + BIG, 2, 20))
        out.append(_case("random", dt, 40, 53, "random", 64, 5, P=64))
        out.append(_case("invalid", dt, 24, 31, BIG, 3, 20, valid="none"))
    big = (((1022, 512), (300, 512), (1022, 100)), ((0, 0), (1022, 0), (0, 512)), ((200, 500), (900, 40), (1000, 512)))
    out.append(_case("large", "f32", 513, 1023, big, 3, 100, gloss=0.5))
    return out


def rejected():
    """(name, P, H, W, dtype code, return code)."""
    return [("P=65", 65, 8, 8, 0, -1), ("H=32769", 2, 32769, 1, 0, -7), ("dtype", 2, 8, 8, 7, -2)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.text.encode()))
    y = torch.arange(c.H, dtype=torch.float64)[:, None]
    x = torch.arange(c.W, dtype=torch.float64)[None, :]
    smooth = 2.0 + 0.04 * x + 0.03 * y + 0.5 * torch.sin(0.31 * x + 0.2) * torch.cos(0.23 * y) + 0.2 * torch.sin(1.9 * x + 1.3 * y)
    depth = (smooth + 0.05 * torch.randn((c.H, c.W), generator=g, dtype=torch.float64)).to(torch_dtype(c))
    if c.tris == "random":
        x0 = torch.randint(0, c.W - 8, (c.P,), generator=g)
        y0 = torch.randint(0, c.H - 8, (c.P,), generator=g)
        d = torch.randint(0, 9, (c.P, 4), generator=g)
        tri = torch.stack([x0, y0, x0 + 3 + d[:, 0], y0 + d[:, 1], x0 + d[:, 2], y0 + 3 + d[:, 3]], dim=1).to(torch.int64)
    else:
        tri = torch.tensor(c.tris, dtype=torch.int64).view(c.P, 6)
    valid = torch.ones(c.H, c.W, dtype=torch.uint8)
    if c.valid == "none":
        valid.zero_()
    if c.valid == "holes":
        valid.view(-1)[::7] = 0
        valid[10:13, 4:8] = 0
    return {"depth": depth, "valid": valid, "tri": tri, "n_planes": torch.tensor([c.n_planes], dtype=torch.int32),
            "gloss": torch.tensor([c.gloss], dtype=torch.float32)}


# ------------------------------------------------------------------------------------------------------------- reference
def _taps(d, replicate=False):
    p = F.pad(d[None, None], (1, 1, 1, 1), mode="replicate")[0, 0] if replicate else F.pad(d, (1, 1, 1, 1))
    H, W = d.shape
    return [[p[i:i + H, j:j + W] for j in range(3)] for i in range(3)]


def _normals(d, replicate=False):
    """The kernel's expressions, in the dtype of d."""
    (a, b, c), (e, _, f), (g, h, i) = _taps(d, replicate)
    return -((a - c) + 2.0 * (e - f) + (g - i)), -((a + 2.0 * b + c) - (g + 2.0 * h + i))


def masks_of(c, inp):
    """(P, H, W) bool: valid pixels inside each triangle."""
    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=torch.float64), torch.arange(c.W, dtype=torch.float64), indexing="ij")
    return torch.stack([plane_ref.points_in_triangle(inp["tri"][j].view(3, 2), xs, ys) & inp["valid"].bool() for j in range(c.P)])


def _abs_stencil(gx, gy):
    """sum over the taps of |k_x| G_x + |k_y| G_y at the pixel each tap reads (the transposed stencil)."""
    tx, ty = _taps(gx), _taps(gy)
    out = torch.zeros_like(gx)
    for i in range(3):
        for j in range(3):
            out = out + abs(KX[i][j]) * tx[2 - i][2 - j] + abs(KY[i][j]) * ty[2 - i][2 - j]
    return out


def reference(c, inp, masks=None):
    masks = masks_of(c, inp) if masks is None else masks
    d = inp["depth"].double().requires_grad_(True)
    nx, ny = _normals(d)
    (a, b, cc), (e, _, f), (g, h, i) = [[t.detach().abs() for t in row] for row in _taps(d)]
    ax, ay = a + cc + 2 * e + 2 * f + g + i, a + 2 * b + cc + g + 2 * h + i
    P = c.P
    ref = {k: torch.zeros(P, dtype=torch.float64) for k in ("n", "mean_x", "mean_y", "active")}
    cond = {k: torch.zeros(P, dtype=torch.float64) for k in ("mean_x", "mean_y")}
    total, loss_cond, act = d.new_zeros(()), 0.0, 0
    gx, gy = torch.zeros(c.H, c.W, dtype=torch.float64), torch.zeros(c.H, c.W, dtype=torch.float64)
    for j in range(min(c.n_planes, P)):
        m = masks[j]
        n = int(m.sum())
        on = n >= c.min_area
        div = float(n) if on else 1.0
        ref["n"][j], ref["active"][j] = n, float(on)
        ref["mean_x"][j], ref["mean_y"][j] = float(nx.detach()[m].sum()) / div, float(ny.detach()[m].sum()) / div
        cond["mean_x"][j], cond["mean_y"][j] = float(ax[m].sum()) / div, float(ay[m].sum()) / div
        if not on:
            continue
        act += 1
        total = total + ((nx[m] - nx[m].mean()) ** 2).mean() + ((ny[m] - ny[m].mean()) ** 2).mean()
        loss_cond += float((ax[m] ** 2 + ay[m] ** 2).sum()) / n
        gx = gx + m * (ax + abs(ref["mean_x"][j])) / n
        gy = gy + m * (ay + abs(ref["mean_y"][j])) / n
    loss = total / max(1, act)
    gl = float(inp["gloss"])
    grad = torch.autograd.grad(loss * gl, d)[0] if act else torch.zeros_like(d)
    ref.update(loss=loss.detach().reshape(1), count=torch.tensor([float(act)], dtype=torch.float64), gdepth=grad)
    zeros = lambda t: torch.zeros_like(t)
    conds = {"loss": (zeros(ref["loss"]), torch.tensor([loss_cond / max(1, act)], dtype=torch.float64)),
             "mean_x": (zeros(cond["mean_x"]), cond["mean_x"]), "mean_y": (zeros(cond["mean_y"]), cond["mean_y"]),
             "gdepth": (zeros(grad), abs(2.0 * gl / max(1, act)) * _abs_stencil(gx, gy))}
    return ref, conds


# ----------------------------------------------------------------------------------------------------------------- model
def model(c, inp, defect=None, masks=None):
    assert defect is None or defect in DEFECTS
    masks = masks_of(c, inp) if masks is None else masks
    P, H, W = c.P, c.H, c.W
    np_ = P if defect == "beyond_count" else min(c.n_planes, P)
    nx, ny = _normals(inp["depth"].float(), replicate=defect == "border_clamped")           # fp32
    n, mean_x, mean_y, active = (torch.zeros(P, dtype=torch.float64) for _ in range(4))
    tot, cnt = 0.0, 0
    for j in range(np_):
        m = masks[j]
        s = [float(m.sum()), float(nx[m].double().sum()), float((nx[m].double() ** 2).sum()), float(ny[m].double().sum()),
             float((ny[m].double() ** 2).sum())]
        on = s[0] > c.min_area if defect == "area_off_by_one" else s[0] >= c.min_area
        div = s[0] if on else 1.0
        n[j], mean_x[j], mean_y[j], active[j] = s[0], s[1] / div, s[3] / div, float(on)
        if on:
            tot += (s[2] / div - mean_x[j].item() ** 2) + (s[4] / div - mean_y[j].item() ** 2)
            cnt += 1
    loss = torch.tensor([tot / max(cnt, 1)], dtype=torch.float64).float()
    # backward
    gxm, gym, have = torch.zeros(H, W), torch.zeros(H, W), torch.zeros(H, W, dtype=torch.bool)
    for j in range(np_):
        use = bool(active[j]) or (defect == "inactive_counts" and n[j] > 0)
        if not use:
            continue
        cntj = float(n[j])
        inv = torch.tensor(1.0 / cntj, dtype=torch.float64).float()
        mx = (mean_x[j] if active[j] else mean_x[j] / cntj).float()
        my = (mean_y[j] if active[j] else mean_y[j] / cntj).float()
        gxm = torch.where(masks[j], gxm + (nx - mx) * inv, gxm)
        gym = torch.where(masks[j], gym + (ny - my) * inv, gym)
        have |= masks[j]
    scale = torch.tensor(2.0, dtype=torch.float32) * inp["gloss"][0] / torch.tensor(float(max(cnt, 1)), dtype=torch.float32)
    tx, ty = _taps(gxm), _taps(gym)
    acc = torch.zeros(H, W)
    if cnt > 0:
        for i in range(3):
            for jx in range(3):
                if i == 1 and jx == 1:
                    continue
                si, sj = (i, jx) if defect == "bwd_untransposed" else (2 - i, 2 - jx)       # tap (i, jx) was read by pixel q - (i - 1, jx - 1)
                acc = acc - (KX[i][jx] * tx[si][sj] + KY[i][jx] * ty[si][sj])
    gd = (acc * scale).to(torch_dtype(c))
    if defect == "stride_once":
        gd.view(-1)[BWD_MAX_BLOCKS * THREADS:] = float("nan")
    return {"loss": loss, "n": n, "mean_x": mean_x, "mean_y": mean_y, "active": active,
            "count": torch.tensor([float(cnt)], dtype=torch.float64), "gdepth": gd}


def split_stats(stats, P):
    """The device's stats vector (4 P + 1 doubles) -> n, mean_x, mean_y, active, count."""
    s = stats.double().cpu()
    t = s[:4 * P].view(P, 4)
    return {"n": t[:, 0].clone(), "mean_x": t[:, 1].clone(), "mean_y": t[:, 2].clone(), "active": t[:, 3].clone(), "count": s[4 * P:4 * P + 1].clone()}


# ------------------------------------------------------------------------------------------------------------ constants
def key_of(c, name):
    """The loss and the statistics are fp32 / fp64 arithmetic whatever the depth's type: one constant each for both depth types."""
    return ("plane_loss", name, c.dtype) if name == "gdepth" else ("plane_loss", "mean" if name.startswith("mean") else name, "f32")


def unit_of(c, name):
    return U_BF16 if name == "gdepth" and c.dtype == "bf16" else U_F32


def axes_of(name):
    return ("row", "column") if name == "gdepth" else ("plane",)


def check(c, got, inp, ref=None, conds=None, what=None):
    """got: {loss, n, mean_x, mean_y, active, count, gdepth} -> {output: worst ratio}."""
    if ref is None:
        ref, conds = reference(c, inp)
    what = what or c.text
    for name in EXACT:
        assert torch.equal(got[name].double().cpu(), ref[name]), "%s %s: got %r, reference %r" % (what, name, got[name].tolist(), ref[name].tolist())
    worst = {}
    for name in OUTPUTS:
        worst[name] = assert_elementwise(got[name], ref[name], conds[name], C[key_of(c, name)], axes_of(name), u=unit_of(c, name),
                                         what="%s %s" % (what, name))
    if ref["count"][0] == 0:
        assert float(got["loss"][0]) == 0.0 and bool((got["gdepth"] == 0).all()), "%s: no plane counts, yet the loss or a gradient is not 0" % what
    return worst


def measure_c(case_list=None):
    worst = {}
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        masks = masks_of(c, inp)
        ref, conds = reference(c, inp, masks)
        got = model(c, inp, masks=masks)
        for name in OUTPUTS:
            r = float(ratio(got[name], ref[name], conds[name], unit_of(c, name)).max())
            worst[key_of(c, name)] = max(worst.get(key_of(c, name), 0.0), r)
    return worst


def format_table(worst):
    lines = ["    operation    output   type   model max   C", "    ----------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-10s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("plane_loss", "gdepth", "bf16"): 1.949,
    ("plane_loss", "gdepth", "f32"): 1.096,
    ("plane_loss", "loss", "f32"): 0.097,
    ("plane_loss", "mean", "f32"): 0.445,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))

"""Sequential fp64 reference of the device LSAP (csrc/lsap.hip, gwd_lsap) and its case list: the comparison is EXACT (CPU only, plain
module).

A case is (Q, the target counts of the B images, cost kind) with layers = 2 and PAD = 5 padding columns behind the last image.
``inputs(c)`` draws, seeded from the case text, cost (2, B, Q, sum T + 5) fp32 - distinct per (layer, image) - and the column offsets.
Cost kinds: ``uniform`` (5 rand - 1: a unique optimum, scipy's own assignment), ``int012`` (integers 0, 1, 2: many optimal
matchings), ``const`` (one value per (layer, image): nothing but the tie rule decides), ``nan_some`` (40 % NaN) and ``inf_row`` (query 0
costs +inf everywhere), the last two as in tests/test_lsap_host.py.

* ``launch(c)``: the dispatch of gwd_lsap restated - NW = 1 (64 lanes) up to Q = 256 and 4 (256 lanes) beyond - and per image the rows
  nr = min(Q, T), the columns nc = max(Q, T), by_query = T > Q and the columns per lane ceil(nc / (64 NW)).
* ``reference(c, inp)`` = ``model(c, inp)``: the same shortest-augmenting-path search, one row after another, in plain numpy fp64.
  Rows are the smaller side; a non-finite cost is read as 1e30; a reduced cost is ((minVal + c) - u_i) - v_j, left to right as in the
  kernel; the next column is the minimum of the open columns under the total order of ``better()``: (reduced cost, a free column
  first, the lowest index).  Because that order is total, its minimum does not depend on the order in which lanes and waves are
  reduced, so the device's assignment must EQUAL this one, ties included - the only witness of the cross-lane and cross-wave
  reduction (a wrong reduction still returns a valid matching, and on costs without ties usually the optimal one).
* ``model(c, inp, defect)`` carries the defects: ``tie_highest_index`` (the highest index wins a tie), ``no_sink_preference`` (a free
  column is not preferred), ``strides_swapped`` (row and column stride exchanged when T > Q), ``padding_unwritten`` (the columns
  behind the last image keep their bytes), ``offset_ignored`` (every image reads and writes from column 0), ``surplus_minus_one``
  (a target without a query holds -1 instead of Q).
* ``check_matching(c, inp, got)`` does not use the reference code: every image holds min(Q, T) distinct queries, surplus targets and
  padding columns hold Q, and the fp64 cost sum equals scipy.optimize.linear_sum_assignment's - exactly for ``int012`` and ``const``
  (sums of small multiples of 1/4 are exact), within 1e-12 relative for ``uniform`` (where the assignment itself is scipy's, too); not
  for the non-finite kinds, whose matching the kernel's header calls arbitrary but valid.
* ``rejected()``: the return codes.

The 1024 limits stay with tests/test_lsap_wide_gpu.py; col_offsets outside the table are not fed."""
import types
import zlib

import numpy as np

DEFECTS = ("tie_highest_index", "no_sink_preference", "strides_swapped", "padding_unwritten", "offset_ignored", "surplus_minus_one")
KINDS = ("uniform", "int012", "const", "nan_some", "inf_row")
LAYERS, PAD, SENTINEL = 2, 5, -7
MAXN, ONE_WAVE_Q, BIG = 1024, 256, 1e30                    # csrc/lsap.hip
QS = (1, 2, 63, 64, 65, 255, 256, 257)
T_LIMIT = 260


def launch(c):
    nw = 1 if c.Q <= ONE_WAVE_Q else 4
    nt = 64 * nw
    images = []
    for T in c.sizes:
        nr, nc = min(c.Q, T), max(c.Q, T)
        images.append(types.SimpleNamespace(T=T, by_query=T > c.Q, nr=nr, nc=nc, per_lane=(nc + nt - 1) // nt, out_trips=(T + nt - 1) // nt))
    return types.SimpleNamespace(NW=nw, NT=nt, blocks=LAYERS * len(c.sizes), images=images, sumT=sum(c.sizes) + PAD)


def sizes_of(Q):
    """T in {0, 1, Q - 1, Q, Q + 1} (at most 260), every one an image of the same problem; the empty image in the middle."""
    ts = sorted({t for t in (1, Q - 1, Q, Q + 1) if 0 < t <= T_LIMIT})
    return tuple(ts[:1] + [0] + ts[1:])


def _case(Q, sizes, kind):
    c = types.SimpleNamespace(Q=Q, sizes=tuple(sizes), kind=kind, B=len(sizes))
    c.text = "lsap Q=%d T=%s cost=%s" % (Q, ",".join(str(t) for t in sizes), kind)
    c.id = c.text.replace(" ", "-")
    return c


def cases():
    out = [_case(Q, sizes_of(Q), kind) for Q in QS for kind in KINDS]
    out += [_case(Q, (64, 0, 65, 130), kind) for Q in (2, 20) for kind in KINDS]        # by-query: one, two, three columns per lane
    return out


def rejected():
    """(name, (layers, B, Q, sum_targets, max_targets), return code)."""
    return [("Q=1025", (1, 1, 1025, 4, 4), -4), ("max_targets=1025", (1, 1, 4, 4, 1025), -4), ("sum_targets=0", (1, 1, 4, 0, 0), -1)]


def inputs(c):
    rng = np.random.default_rng(zlib.crc32(c.text.encode()))
    sumT = sum(c.sizes) + PAD
    off = np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int32)
    shape = (LAYERS, c.B, c.Q, sumT)
    cost = (rng.random(shape) * 5 - 1).astype(np.float32)
    if c.kind == "int012":
        cost = rng.integers(0, 3, shape).astype(np.float32)
    if c.kind == "const":
        cost[:] = (0.25 * (1 + np.arange(LAYERS * c.B, dtype=np.float32))).reshape(LAYERS, c.B, 1, 1)
    if c.kind == "nan_some":
        cost[rng.random(shape) < 0.4] = np.nan
    if c.kind == "inf_row":
        cost[:, :, 0, :] = np.inf
    return {"cost": cost, "off": off}


# ----------------------------------------------------------------------------------------------------- the sequential search
def _solve(M, defect=None):
    """M (nr, nc) fp64, nr <= nc -> (col4row, row4col)."""
    nr, nc = M.shape
    u, v = np.zeros(nr), np.zeros(nc)
    row4col, col4row = np.full(nc, -1), np.full(nr, -1)
    cols = np.arange(nc)
    for cur in range(nr):
        sp, closed, path, in_tree = np.full(nc, np.inf), np.zeros(nc, bool), np.full(nc, -1), np.zeros(nr, bool)
        min_val, i, sink = 0.0, cur, -1
        for _ in range(cur + 1):
            in_tree[i] = True
            r = ((min_val + M[i]) - u[i]) - v
            upd = ~closed & (r < sp)
            sp[upd] = r[upd]
            path[upd] = i
            s = np.where(closed, np.inf, sp)
            cand = ~closed & (s == s.min())
            assert cand.any()
            if defect != "no_sink_preference" and (cand & (row4col < 0)).any():
                cand &= row4col < 0
            j = int(cols[cand][-1] if defect == "tie_highest_index" else cols[cand][0])
            min_val = sp[j]
            closed[j] = True
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        assert sink >= 0
        u[cur] += min_val
        for r_ in np.nonzero(in_tree)[0]:
            if r_ != cur:
                u[r_] += min_val - sp[col4row[r_]]
        v[closed] -= min_val - sp[closed]
        j = sink
        while True:
            r_ = path[j]
            row4col[j] = r_
            col4row[r_], j = j, col4row[r_]
            if r_ == cur:
                break
    return col4row, row4col


def model(c, inp, defect=None):
    """-> query_of_target (LAYERS, sum T + PAD) int32; columns that are not written hold SENTINEL."""
    assert defect is None or defect in DEFECTS
    cost, off = inp["cost"], inp["off"]
    sumT = cost.shape[-1]
    out = np.full((LAYERS, sumT), SENTINEL, np.int32)
    flat = cost.reshape(-1)
    for layer in range(LAYERS):
        for b, T in enumerate(c.sizes):
            c0 = 0 if defect == "offset_ignored" else int(off[b])
            if T > 0:
                base = ((layer * c.B + b) * c.Q) * sumT + c0                      # element (q, t) at flat[base + q sumT + t]
                q, t = np.arange(c.Q)[:, None], np.arange(T)[None, :]
                idx = base + (q + t * sumT if defect == "strides_swapped" and T > c.Q else q * sumT + t)
                blk = flat[np.minimum(idx, flat.size - 1)]                         # (Q, T); (the swapped read leaves the block: kept inside the tensor)
                blk = np.where(np.isfinite(blk), blk.astype(np.float64), BIG)
                if T > c.Q:
                    col4row, row4col = _solve(blk, defect)                          # rows = queries
                    res = row4col
                else:
                    col4row, row4col = _solve(blk.T.copy(), defect)                 # rows = targets
                    res = col4row
                none = -1 if defect == "surplus_minus_one" else c.Q
                out[layer, c0:c0 + T] = np.where((res >= 0) & (res < c.Q), res, none)
        if defect != "padding_unwritten":
            out[layer, int(off[-1]):] = c.Q
    return out


def reference(c, inp):
    return model(c, inp)


# ----------------------------------------------------------------------------------------------- the bar without the reference
def check_matching(c, inp, got):
    from scipy.optimize import linear_sum_assignment
    cost, off = inp["cost"], inp["off"]
    assert got.shape == (LAYERS, cost.shape[-1]) and (got[:, int(off[-1]):] == c.Q).all(), c.text + ": padding columns"
    for layer in range(LAYERS):
        for b, T in enumerate(c.sizes):
            g = got[layer, off[b]:off[b + 1]]
            m = g[g < c.Q]
            assert ((g >= 0) & (g <= c.Q)).all() and len(m) == min(c.Q, T) and len(set(m.tolist())) == len(m), (c.text, layer, b)
            if T == 0 or c.kind in ("nan_some", "inf_row"):
                continue
            blk = cost[layer, b, :, off[b]:off[b + 1]].astype(np.float64)
            qi, ti = linear_sum_assignment(blk)
            want = blk[qi, ti].sum()
            ts = np.nonzero(g < c.Q)[0]
            have = blk[g[ts], ts].sum()
            if c.kind == "uniform":
                assert abs(have - want) <= 1e-12 * abs(want), (c.text, layer, b, have, want)
                full = np.full(T, c.Q)
                full[ti] = qi
                assert (g == full).all(), (c.text, layer, b)
            else:
                assert have == want, (c.text, layer, b, have, want)

// Line scoring geometry shared by the device kernel (csrc/linescore.hip) and a host build (tests/linescore_host.cpp): the pair
// test and the interval update of L-CNN's line NMS (evaluation/eval_post_online.py:17-91 of the reference) and the endpoint
// distance of msTPFP (evaluation/lcnn/metric.py:194-200), as plain scalar functions.
//
// PRECISION IS A DECISION.  The reference's arithmetic inside pline / plambda depends on the NumPy version it runs under (fp32
// scalars under NumPy 2 promotion, f64 through float(dd) under 1.x), so there is no single literal behaviour to match.  Pinned
// here: the coordinates are scaled to pixels in fp32 (as the reference does), promoted to f64, and everything after that is f64 -
// what the reference's functions compute when they are handed float64 arrays (tests/golden/line_score.npz is made that way).
// No contraction: a * b + c stays two roundings, as NumPy has it.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define LS_HD __host__ __device__ __forceinline__
#else
#define LS_HD inline
#endif

// Python's two-argument max / min: the first operand unless the second is strictly greater / smaller
LS_HD double ls_pymax(double a, double b) { return b > a ? b : a; }
LS_HD double ls_pymin(double a, double b) { return b < a ? b : a; }

// plambda (:37-41): the position of (x, y) along the line (x1, y1) -> (x2, y2); max(1e-9, dd) keeps a zero-length line finite
LS_HD double ls_plambda(double x1, double y1, double x2, double y2, double x, double y) {
    const double px = x2 - x1, py = y2 - y1;
    const double dd = px * px + py * py;
    return ((x - x1) * px + (y - y1) * py) / ls_pymax(1e-9, dd);
}

// pline (:17-24): squared distance of (x, y) from the infinite line through (x1, y1), (x2, y2)
LS_HD double ls_pline(double x1, double y1, double x2, double y2, double x, double y) {
    const double px = x2 - x1, py = y2 - y1;
    const double dd = px * px + py * py;
    const double u = ((x - x1) * px + (y - y1) * py) / ls_pymax(1e-9, dd);
    const double dx = x1 + u * px - x, dy = y1 + u * py - y;
    return dx * dx + dy * dy;
}

// p + (q - p) * s, one coordinate (:88).  s = 1 does NOT give q back exactly, so the end point goes through this too.
LS_HD double ls_along(double p, double q, double s) { return p + (q - p) * s; }

// The part of postprocess()'s inner loop that depends on the pair alone (:49-62, tol = 0): line i = (p, q), selected line (a, b)
// (already clipped).  False: the pair is further apart than the threshold (the `continue` of :56).  True: la <= lb are the
// positions of a and b along (p, q).
LS_HD bool ls_pair(const double p[2], const double q[2], const double a[2], const double b[2], double thr2, double &la, double &lb) {
    const double d = ls_pymin(ls_pymax(ls_pline(p[0], p[1], q[0], q[1], a[0], a[1]), ls_pline(p[0], p[1], q[0], q[1], b[0], b[1])),
                              ls_pymax(ls_pline(a[0], a[1], b[0], b[1], p[0], p[1]), ls_pline(a[0], a[1], b[0], b[1], q[0], q[1])));
    if (d > thr2) return false;
    la = ls_plambda(p[0], p[1], q[0], q[1], a[0], a[1]);
    lb = ls_plambda(p[0], p[1], q[0], q[1], b[0], b[1]);
    if (la > lb) {
        const double t = la;
        la = lb;
        lb = t;
    }
    return true;
}

// The order-dependent part (:64-84, do_clip = False): [start, end] of line i against one selected line's [la, lb].
// True = the reference's `break` (covered, or nothing left).  A line is kept iff !(start >= end) after the walk (:86).
LS_HD bool ls_interval(double &start, double &end, double la, double lb) {
    if (start < la && lb < end) return false;              // case 1: strictly inside, skip
    if (lb < start || la > end) return false;              // disjoint
    if (la <= start && end <= lb) {                        // cover
        start = 10.0;
        return true;
    }
    if (la <= start && start <= lb) start = lb;            // case 2
    if (la <= end && end <= lb) end = la;                  // case 3
    return start >= end;
}

// msTPFP's distance (metric.py:195-198): squared endpoint distances of line l = (y1, x1, y2, x2) to g, the better of both orders
LS_HD double ls_match(const double l[4], const double g[4]) {
    const double a0 = l[0] - g[0], a1 = l[1] - g[1], b0 = l[2] - g[2], b1 = l[3] - g[3];
    const double c0 = l[0] - g[2], c1 = l[1] - g[3], e0 = l[2] - g[0], e1 = l[3] - g[1];
    const double same = (a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1), swapped = (c0 * c0 + c1 * c1) + (e0 * e0 + e1 * e1);
    return swapped < same ? swapped : same;                // np.minimum on numbers
}

// Linear sum assignment on the device for the line matcher (src/models/matcher.py:71-74 calls
// scipy.optimize.linear_sum_assignment on the host, 6x per step, each a device->host sync).
// One workgroup per (decoder layer, image) problem: T targets x Q queries, both up to 1024, solved by the same
// shortest-augmenting-path algorithm scipy uses (Crouse 2016), in double precision like scipy.  The ROWS of the search are the
// smaller side, as in scipy: targets when T <= Q (every target gets a distinct query), queries when T > Q (every query gets a
// distinct target, the surplus targets receive the dummy query Q like padding columns).  The candidate scan over the columns is
// spread over the lanes of 1 wave (Q <= 256) or 4 waves; the optimum is unique unless costs tie exactly.
//
// Termination does not depend on the data: a non-finite cost is read as BIG, so every reduced cost is finite; every loop below has a
// trip count fixed by Q and T on entry, and every LDS index that comes out of a reduction or a table is clamped before use.  A
// search that does not find a free column within its bound (impossible with finite costs) ends the solve; rows without a column
// come back as the dummy query Q.
#ifndef GWD_LSAP_HOST          // tests/lsap_host.cpp compiles this file for the CPU and supplies the device vocabulary itself
#include "common.h"
#endif

namespace {

constexpr int MAXN = 1024;               // bound on Q and on the targets of one image
// stands in for NaN / +-inf costs.  It only keeps the arithmetic finite: once a dual has absorbed a BIG, costs of order 1 fall below its
// ulp (~1e14), so the matching of such a matrix is valid (distinct pairs) but arbitrary, not the optimum over its finite entries
constexpr double BIG = 1e30;

__device__ __forceinline__ double cost_at(const float *C, size_t idx) {
    const float c = C[idx];
    return isfinite(c) ? (double)c : BIG;
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// lowest cost; among equals prefer an unassigned column (a new sink), then the lowest index
__device__ __forceinline__ bool better(double s, int f, int j, double best, int bf, int bj) {
    return s < best || (s == best && (f > bf || (f == bf && j < bj)));
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void lsap_kernel(const float *__restrict__ cost, const int *__restrict__ col_off,
                                                       int32_t *__restrict__ query_of_target, int B, int Q, int sumT) {
    constexpr int NT = 64 * NW;
    __shared__ double v[MAXN], sp[MAXN], u[MAXN];
    __shared__ int path[MAXN], row4col[MAXN], col4row[MAXN];
    __shared__ unsigned char SC[MAXN], SR[MAXN];
    __shared__ double wbest[NW];
    __shared__ int wj[NW], wfree[NW];
    const int layer = blockIdx.x / B, b = blockIdx.x % B, tid = threadIdx.x;
    // the counts are device data: never index past the LDS tables or the cost block (the host checks them too)
    const int c0 = clampi(col_off[b], 0, sumT);
    const int T = clampi(col_off[b + 1] - c0, 0, min(MAXN, sumT - c0));
    const float *C = cost + ((size_t)layer * B + b) * Q * sumT + c0;      // element (q, t) at C[q * sumT + t]
    const bool by_query = T > Q;                                          // rows = queries, columns = targets
    const int nr = by_query ? Q : T, nc = by_query ? T : Q;               // nr <= nc <= MAXN
    const size_t rs = by_query ? (size_t)sumT : 1, cs = by_query ? 1 : (size_t)sumT;   // element (row i, column j) at C[i * rs + j * cs]
    // each of the three fills: nc (nr) / NT trips
    for (int j = tid; j < nc; j += NT) {
        v[j] = 0.0;
        row4col[j] = -1;
    }
    for (int i = tid; i < nr; i += NT) {
        u[i] = 0.0;
        col4row[i] = -1;
    }
    __syncthreads();
    bool ok = true;
    // one augmentation per row: nr trips (`ok` only ends it early)
    for (int cur = 0; cur < nr && ok; ++cur) {
        for (int j = tid; j < nc; j += NT) {         // nc / NT trips
            sp[j] = INFINITY;
            SC[j] = 0;
            path[j] = -1;
        }
        for (int i = tid; i < nr; i += NT) SR[i] = 0;    // nr / NT trips
        __syncthreads();
        double minVal = 0.0;
        int i = cur, sink = -1;
        // every trip closes one more column; only the `cur` columns assigned so far are no sink, so trip cur + 1 at the latest
        // finds one: at most cur + 1 <= nr trips
        for (int it = 0; it <= cur && sink < 0; ++it) {
            if (tid == 0) SR[i] = 1;
            double best = INFINITY;
            int bj = 0x7fffffff, bf = 0;
            const double ui = u[i];
            for (int j = tid; j < nc; j += NT) {      // nc / NT trips
                if (SC[j]) continue;
                const double r = minVal + cost_at(C, (size_t)i * rs + (size_t)j * cs) - ui - v[j];
                if (r < sp[j]) {
                    sp[j] = r;
                    path[j] = i;
                }
                const double s = sp[j];
                const int f = row4col[j] < 0;
                if (better(s, f, j, best, bf, bj)) {
                    best = s;
                    bj = j;
                    bf = f;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {        // 6 trips
                const double ob = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bj, o, 64), of = __shfl_xor(bf, o, 64);
                if (better(ob, of, oj, best, bf, bj)) {
                    best = ob;
                    bj = oj;
                    bf = of;
                }
            }
            if (NW > 1) {
                if ((tid & 63) == 0) {
                    wbest[tid >> 6] = best;
                    wj[tid >> 6] = bj;
                    wfree[tid >> 6] = bf;
                }
                __syncthreads();
                best = wbest[0];
                bj = wj[0];
                bf = wfree[0];
#pragma unroll
                for (int w = 1; w < NW; ++w)          // NW - 1 trips
                    if (better(wbest[w], wfree[w], wj[w], best, bf, bj)) {
                        best = wbest[w];
                        bj = wj[w];
                        bf = wfree[w];
                    }
            }
            if (bj >= nc) {                           // no open column left (uniform over the workgroup): give the solve up
                ok = false;
                break;
            }
            minVal = best;
            const int j = clampi(bj, 0, nc - 1);
            __syncthreads();
            if (tid == 0) SC[j] = 1;
            const int r4 = row4col[j];
            if (r4 < 0) sink = j; else i = clampi(r4, 0, nr - 1);
            __syncthreads();
        }
        if (sink < 0) ok = false;
        if (!ok) break;                               // uniform: every thread holds the same sink / ok
        // dual update
        if (tid == 0) u[cur] += minVal;
        for (int r = tid; r < nr; r += NT)            // nr / NT trips
            if (SR[r] && r != cur) u[r] += minVal - sp[clampi(col4row[r], 0, nc - 1)];
        for (int j = tid; j < nc; j += NT)            // nc / NT trips
            if (SC[j]) v[j] -= minVal - sp[j];
        __syncthreads();
        if (tid == 0) {                               // augment along the path
            int j = sink;
            // the path alternates between distinct rows and ends at row cur: at most nr trips
            for (int it = 0; it < nr && j >= 0; ++it) {
                const int r = clampi(path[j], 0, nr - 1);
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                j = prev < nc ? prev : -1;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    int32_t *out = query_of_target + (size_t)layer * sumT + c0;
    // T / NT trips; a target without a query (surplus when T > Q, or a solve given up) sits on the dummy query Q
    for (int t = tid; t < T; t += NT) {
        const int q = by_query ? row4col[t] : col4row[t];
        out[t] = (q >= 0 && q < Q) ? q : Q;
    }
    if (b == B - 1)                      // padding columns of a fixed-capacity target table: the dummy query slot Q; <= sumT / NT trips
        for (int t = clampi(col_off[B], 0, sumT) + tid; t < sumT; t += NT) query_of_target[(size_t)layer * sumT + t] = Q;
}

}  // namespace

#ifndef GWD_LSAP_HOST
extern "C" int gwd_lsap(const float *cost, const int32_t *col_offsets, int32_t *query_of_target, int32_t layers, int32_t B,
                        int32_t Q, int32_t sum_targets, int32_t max_targets, void *stream) {
    if (!cost || !col_offsets || !query_of_target || layers <= 0 || B <= 0 || Q <= 0 || sum_targets <= 0) return -1;
    if (Q > MAXN || max_targets > MAXN) return -4;
    // by Q alone: the per-image counts are device data and max_targets is usually just the table's capacity.  Up to 256 queries one
    // wave scans the columns (16 per lane at most when an image has 1024 targets); beyond, four waves share them
    if (Q <= 256)
        lsap_kernel<1><<<layers * B, 64, 0, (hipStream_t)stream>>>(cost, col_offsets, query_of_target, B, Q, sum_targets);
    else
        lsap_kernel<4><<<layers * B, 256, 0, (hipStream_t)stream>>>(cost, col_offsets, query_of_target, B, Q, sum_targets);
    GWD_CHECK_LAUNCH();
    return 0;
}
#endif

// Glass regions on the device: from the per-pixel results of InferenceSession.predict_frames (labels uint8, depth_mm uint16,
// [B][Fh][Fw], top-left aligned frames of different sizes, sizes on the device) to objects - connected components of the glass
// pixels, exact integer records of the largest of them, a least-squares plane in inverse depth per region and the depth every
// region's plane predicts.  No host sync, no memset, no floating-point atomics; every phase is its own launch, so a kernel
// boundary is the only thing any thread ever waits for.
//
// gwd_glass_regions
//   cc_init_kernel      parent[i] of a glass pixel i = y * fw + x (FRAME raster index) = the first pixel of its horizontal run
//                       inside its aligned 64-pixel segment (one wave, one ballot); -1 for every other pixel of the frame.
//   cc_merge_kernel     lock-free unions against the row above and across segment edges.  Invariant: parent[i] <= i, and
//                       parent[a] changes only while a is a root (compare-and-swap a -> b with b < a), so every link joins two
//                       pixels of one component, no link is ever lost, and the root of a set is its smallest raster index.
//                       find() strictly lowers its index in every iteration; a failed swap means another thread's swap
//                       succeeded and the retry starts from a strictly lower index: no iteration waits for anyone.
//   cc_flatten_kernel   parent[i] = root, area[root] += pixels: one integer atomic per (wave, root), the first root a workgroup
//                       meets collected in LDS (a large component would otherwise take every add on ONE address).
//   cc_candidates_kernel  roots counted (region_total), roots with area >= min_area appended to the candidate list.
//   cc_select_kernel    one workgroup per image: the max_regions largest by (area desc, anchor asc) - the key is unique, so the
//                       order candidates arrived in changes nothing; more candidates than the list holds: region_count = -1.
//   cc_records_kernel   region_map and the integer records of the kept regions: LDS per workgroup, one wave-aggregated add per
//                       wave whose kept pixels share a region, then one global integer atomic per touched field and workgroup.
//   cc_finish_kernel    the public records in rank order.
// gwd_region_planes     moments in fixed pieces (row y belongs to workgroup y % nb, a wave owns 64 neighbours of a row), one
//                       partial record per workgroup, folded in ascending order; solve; a second pass of the same shape for rms.
//                       The fit itself is planefit.h, shared with fusion.hip.
// gwd_depth_planar      the copy of the depth with the pixels of fitted regions rewritten.
#include "common.h"
#include "depthmm.h"
#include "planefit.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxB = 16;
constexpr int kMaxR = GWD_REGION_MAX;
constexpr int kRec = GWD_REGION_RECORD;                   // int64 fields of a record
constexpr int kRows = 16;                                 // rows one workgroup of the flatten, candidate and record passes walks
constexpr int kPlaneBlocks = 64;                          // workgroups per image of the moment passes, at most
constexpr int kNI = kFitNI, kND = kFitND;                 // integer / fp64 moments of a partial record (planefit.h)
enum { F_AREA = 0, F_X0, F_Y0, F_X1, F_Y1, F_ANCHOR, F_SX, F_SY, F_ND, F_SMM, F_MINMM, F_MAXMM };

struct Layout {                                           // byte offsets into the workspace, every one a multiple of 16
    int64_t counters, sel, raw, partial, cand, parent, area, total;
};
__host__ __device__ inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
int64_t partial_offset(int64_t B) { return 128 + up16(B * kMaxR * 4) + B * kMaxR * kRec * 8; }      // needs neither the frame nor the list size
Layout layout(int64_t B, int64_t Fh, int64_t Fw, int64_t maxcand) {
    Layout l;
    l.counters = 0;                                       // [2][16] int32: candidates seen, components found
    l.sel = 128;                                          // [B][32] int32 anchors in rank order
    l.raw = l.sel + up16(B * kMaxR * 4);                  // [B][32][12] int64 accumulators
    l.partial = l.raw + B * kMaxR * kRec * 8;             // [B][kPlaneBlocks][32][10] 8-byte values (gwd_region_planes)
    l.cand = l.partial + B * kPlaneBlocks * kMaxR * (kNI + kND) * 8;       // [B][maxcand] int32
    l.parent = l.cand + up16(B * maxcand * 4);            // [B][Fh * Fw] int32
    l.area = l.parent + up16(B * Fh * Fw * 4);            // [B][Fh * Fw] int32
    l.total = l.area + up16(B * Fh * Fw * 4);
    return l;
}

__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// every iteration strictly lowers a (0 <= p < a) or leaves: at most a iterations whatever the plane holds
__device__ __forceinline__ int find_root(const int *P, int a) {
    for (;;) {
        const int p = ld(P + a);
        if (p >= a || p < 0) return a;
        a = p;
    }
}

// every iteration returns or strictly lowers a + b; parent[a] is written only while it still equals a
__device__ __forceinline__ void unite(int *P, int a, int b) {
    for (;;) {
        a = find_root(P, a);
        b = find_root(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expected = a;
        if (__hip_atomic_compare_exchange_strong(P + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (expected >= a || expected < 0) return;        // cannot happen (parent[a] < a once a is no root); never loop on it
        a = expected;
    }
}

struct CcArgs {
    const uint8_t *labels;
    const uint16_t *depth_mm;
    const int32_t *sizes;
    int32_t *counters, *sel, *cand, *parent, *area;
    long long *raw;
    uint8_t *region_map;
    int32_t *region_count, *region_total;
    long long *records;
    int64_t plane;
    int32_t B, Fh, Fw, max_regions, min_area, conn8, maxcand, lo_mm, hi_mm;
};

// thread = pixel (x, y) of image b; a wave = 64 neighbours of one row starting at a multiple of 64
#define PIXEL_THREAD()                                                 \
    const int b = blockIdx.z, y = blockIdx.y;                           \
    const int x = blockIdx.x * kThreads + threadIdx.x;                  \
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);                   \
    if (y >= f.fh) return;                                              \
    const bool in = x < f.fw;                                           \
    const uint8_t *__restrict__ L = a.labels + b * a.plane;             \
    int *__restrict__ P = a.parent + b * a.plane;                       \
    int *__restrict__ A = a.area + b * a.plane;                         \
    const int i = y * f.fw + x;                                         \
    (void)L; (void)P; (void)A; (void)i

__global__ __launch_bounds__(kThreads) void cc_init_kernel(const CcArgs a) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 2) a.counters[threadIdx.x * kMaxB + blockIdx.z] = 0;
    PIXEL_THREAD();
    const bool g = in && L[(int64_t)y * a.Fw + x] == 1;
    const unsigned long long m = __ballot(g);
    if (!in) return;
    A[i] = 0;
    if (!g) { P[i] = -1; return; }
    const int lane = threadIdx.x & 63;
    const unsigned long long starts = m & ~(m << 1);
    const unsigned long long below = starts & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));      // never 0: a glass lane has a start at or below it
    P[i] = i - lane + (63 - __clzll((long long)below));
}

__global__ __launch_bounds__(kThreads) void cc_merge_kernel(const CcArgs a) {
    PIXEL_THREAD();
    if (!in || L[(int64_t)y * a.Fw + x] != 1) return;
    const uint8_t *row = L + (int64_t)y * a.Fw;
    const bool left = x > 0 && row[x - 1] == 1;
    if (left && (x & 63) == 0) unite(P, i, i - 1);        // a run cut by the segment edge
    if (y == 0) return;
    const uint8_t *above = row - a.Fw;
    const bool up = above[x] == 1, ul = x > 0 && above[x - 1] == 1, ur = x + 1 < f.fw && above[x + 1] == 1;
    if (up) {
        if (!(left && ul)) unite(P, i, i - f.fw);         // otherwise the left neighbour joins the same two runs
    } else if (a.conn8) {
        if (ul && !left) unite(P, i, i - f.fw - 1);
        if (ur) unite(P, i, i - f.fw + 1);
    }
}

// thread = column x of a chunk of kRows rows of image b: the loops below have uniform bounds, so every lane reaches the ballots
#define CHUNK_THREAD()                                                 \
    const int b = blockIdx.z, y0 = blockIdx.y * kRows, lane = threadIdx.x & 63; \
    const int x = blockIdx.x * kThreads + threadIdx.x;                  \
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);                   \
    const int y1 = min(y0 + kRows, f.fh);                               \
    const uint8_t *__restrict__ L = a.labels + b * a.plane;             \
    int *__restrict__ P = a.parent + b * a.plane;                       \
    int *__restrict__ A = a.area + b * a.plane;                         \
    (void)L; (void)P; (void)A; (void)lane

// parent[i] = root (an atomicMin: a parent only ever falls, and the root is below every other member, so pixels flattened earlier
// shorten the walks of the later ones), area[root] += pixels.  One add per (wave, root); the adds to the first root a workgroup
// meets - a large component is met by most of them - are kept in LDS and leave as ONE global add per workgroup.
__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(const CcArgs a) {
    __shared__ int own_root, own_count;
    CHUNK_THREAD();
    if (threadIdx.x == 0) { own_root = -1; own_count = 0; }
    __syncthreads();
    for (int y = y0; y < y1; ++y) {
        const int i = y * f.fw + x;
        const bool g = x < f.fw && L[(int64_t)y * a.Fw + x] == 1;
        int r = -1;
        if (g) {
            r = find_root(P, i);
            if (r != i) __hip_atomic_fetch_min(P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned long long todo = __ballot(g);
        while (todo) {                                    // one round per root present in the wave
            const int first = __builtin_ctzll(todo);
            const int r0 = __shfl(r, first, 64);
            const unsigned long long mine = __ballot(g && r == r0);
            todo &= ~mine;
            if (lane == first) {
                const int cnt = __popcll(mine);
                const int seen = atomicCAS(&own_root, -1, r0);
                if (seen == -1 || seen == r0) atomicAdd(&own_count, cnt);
                else atomicAdd(A + r0, cnt);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && own_count) atomicAdd(A + own_root, own_count);
}

__global__ __launch_bounds__(kThreads) void cc_candidates_kernel(const CcArgs a) {
    __shared__ int roots;
    CHUNK_THREAD();
    if (threadIdx.x == 0) roots = 0;
    __syncthreads();
    int mine = 0;
    for (int y = y0; y < y1; ++y) {
        const int i = y * f.fw + x;
        if (x >= f.fw || P[i] != i) continue;
        ++mine;
        if (A[i] < a.min_area) continue;
        const int slot = atomicAdd(a.counters + b, 1);
        if (slot < a.maxcand) a.cand[(int64_t)b * a.maxcand + slot] = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&roots, mine);
    __syncthreads();
    if (threadIdx.x == 0 && roots) atomicAdd(a.counters + kMaxB + b, roots);
}

__global__ __launch_bounds__(kThreads) void cc_select_kernel(const CcArgs a) {
    __shared__ unsigned long long wmax[4];
    __shared__ unsigned long long prev_s;
    __shared__ int chosen[kMaxR];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.counters[b];
    int *__restrict__ A = a.area + b * a.plane;
    const int *__restrict__ C = a.cand + (int64_t)b * a.maxcand;
    for (int k = threadIdx.x; k < kMaxR * kRec; k += kThreads) {
        const int fld = k % kRec;
        a.raw[(int64_t)b * kMaxR * kRec + k] = (fld == F_X0 || fld == F_Y0 || fld == F_MINMM) ? (1ll << 40) : (fld == F_X1 || fld == F_Y1 || fld == F_MAXMM) ? -1ll : 0ll;
    }
    if (threadIdx.x == 0) a.region_total[b] = a.counters[kMaxB + b];
    const bool refused = n > a.maxcand;
    const int K = refused ? 0 : min(n, a.max_regions);
    if (threadIdx.x == 0) {
        a.region_count[b] = refused ? -1 : K;
        prev_s = ~0ull;
    }
    __syncthreads();
    for (int r = 0; r < K; ++r) {                         // the largest key below the one chosen last; keys are unique
        const unsigned long long prev = prev_s;
        unsigned long long best = 0;
        for (int k = threadIdx.x; k < n; k += kThreads) {
            const int anchor = C[k];
            const unsigned long long key = ((unsigned long long)(unsigned)A[anchor] << 32) | (0xffffffffu - (unsigned)anchor);
            if (key < prev && key > best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o, 64);
            best = v > best ? v : best;
        }
        if (lane == 0) wmax[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long m = wmax[0];
            for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
            prev_s = m;
            chosen[r] = (int)(0xffffffffu - (unsigned)(m & 0xffffffffull));
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < kMaxR) {
        const int r = threadIdx.x;
        a.sel[b * kMaxR + r] = r < K ? chosen[r] : -1;
        if (r < K) A[chosen[r]] = -(r + 1);               // the areas have been read: the root's entry now names its rank
    }
}

__global__ __launch_bounds__(kThreads) void cc_records_kernel(const CcArgs a) {
    __shared__ unsigned long long sadd[kMaxR][5];        // area, sum_x, sum_y, n_depth, sum_mm
    __shared__ int smin[kMaxR][3], smax[kMaxR][3];        // x, y, mm
    const int b = blockIdx.z, x = blockIdx.x * kThreads + threadIdx.x, y0 = blockIdx.y * kRows, lane = threadIdx.x & 63;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    const int *__restrict__ P = a.parent + b * a.plane;
    const int *__restrict__ A = a.area + b * a.plane;
    const uint16_t *__restrict__ D = a.depth_mm + b * a.plane;
    uint8_t *__restrict__ M = a.region_map + b * a.plane;
    for (int k = threadIdx.x; k < kMaxR * 5; k += kThreads) sadd[k / 5][k % 5] = 0ull;
    for (int k = threadIdx.x; k < kMaxR * 3; k += kThreads) { smin[k / 3][k % 3] = 1 << 30; smax[k / 3][k % 3] = -1; }
    __syncthreads();
    bool any = false;
    for (int y = y0; y < y0 + kRows && y < a.Fh; ++y) {   // uniform bounds: every lane of a wave takes part in the ballots
        int rank = 0, mm = 0;
        if (y < f.fh && x < f.fw) {
            const int r = P[y * f.fw + x];
            if (r >= 0) {
                const int v = A[r];
                rank = v < 0 ? min(-v, kMaxR) : 0;
            }
            if (rank) mm = D[(int64_t)y * a.Fw + x];
        }
        if (x < a.Fw) M[(int64_t)y * a.Fw + x] = (uint8_t)rank;
        const unsigned long long m = __ballot(rank > 0);
        if (!m) continue;
        any = true;
        const int first = __shfl(rank, __builtin_ctzll(m), 64);
        const bool ok = rank > 0 && mm >= a.lo_mm && mm <= a.hi_mm;
        if (__ballot(rank > 0 && rank != first) == 0ull) {                        // one region in this wave: reduce, then one lane adds
            int sx = rank ? x : 0, nd = ok ? 1 : 0, smm = ok ? mm : 0;
            int xl = rank ? x : 1 << 30, xh = rank ? x : -1, ml = ok ? mm : 1 << 30, mh = ok ? mm : -1;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                sx += __shfl_xor(sx, o, 64); nd += __shfl_xor(nd, o, 64); smm += __shfl_xor(smm, o, 64);
                xl = min(xl, __shfl_xor(xl, o, 64)); xh = max(xh, __shfl_xor(xh, o, 64));
                ml = min(ml, __shfl_xor(ml, o, 64)); mh = max(mh, __shfl_xor(mh, o, 64));
            }
            if (lane == 0) {
                const int r = first - 1, cnt = __popcll(m);
                atomicAdd(&sadd[r][0], (unsigned long long)cnt);
                atomicAdd(&sadd[r][1], (unsigned long long)sx);
                atomicAdd(&sadd[r][2], (unsigned long long)cnt * (unsigned long long)y);
                atomicAdd(&sadd[r][3], (unsigned long long)nd);
                atomicAdd(&sadd[r][4], (unsigned long long)smm);
                atomicMin(&smin[r][0], xl); atomicMax(&smax[r][0], xh);
                atomicMin(&smin[r][1], y); atomicMax(&smax[r][1], y);
                if (nd) { atomicMin(&smin[r][2], ml); atomicMax(&smax[r][2], mh); }
            }
        } else if (rank > 0) {
            const int r = rank - 1;
            atomicAdd(&sadd[r][0], 1ull);
            atomicAdd(&sadd[r][1], (unsigned long long)x);
            atomicAdd(&sadd[r][2], (unsigned long long)y);
            atomicMin(&smin[r][0], x); atomicMax(&smax[r][0], x);
            atomicMin(&smin[r][1], y); atomicMax(&smax[r][1], y);
            if (ok) {
                atomicAdd(&sadd[r][3], 1ull);
                atomicAdd(&sadd[r][4], (unsigned long long)mm);
                atomicMin(&smin[r][2], mm); atomicMax(&smax[r][2], mm);
            }
        }
    }
    if (!__syncthreads_or(any ? 1 : 0)) return;
    long long *raw = a.raw + (int64_t)b * kMaxR * kRec;
    for (int k = threadIdx.x; k < kMaxR * kRec; k += kThreads) {                  // integer atomics: their order changes no bit
        const int r = k / kRec, fld = k - r * kRec;
        if (sadd[r][0] == 0ull) continue;
        long long *dst = raw + k;
        switch (fld) {
            case F_AREA: atomicAdd((unsigned long long *)dst, sadd[r][0]); break;
            case F_SX: atomicAdd((unsigned long long *)dst, sadd[r][1]); break;
            case F_SY: atomicAdd((unsigned long long *)dst, sadd[r][2]); break;
            case F_ND: if (sadd[r][3]) atomicAdd((unsigned long long *)dst, sadd[r][3]); break;
            case F_SMM: if (sadd[r][4]) atomicAdd((unsigned long long *)dst, sadd[r][4]); break;
            case F_X0: atomicMin(dst, (long long)smin[r][0]); break;
            case F_Y0: atomicMin(dst, (long long)smin[r][1]); break;
            case F_X1: atomicMax(dst, (long long)smax[r][0]); break;
            case F_Y1: atomicMax(dst, (long long)smax[r][1]); break;
            case F_MINMM: if (sadd[r][3]) atomicMin(dst, (long long)smin[r][2]); break;
            case F_MAXMM: if (sadd[r][3]) atomicMax(dst, (long long)smax[r][2]); break;
            default: break;
        }
    }
}

__global__ __launch_bounds__(kThreads) void cc_finish_kernel(const CcArgs a) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= a.B * a.max_regions * kRec) return;
    const int fld = t % kRec, r = (t / kRec) % a.max_regions, b = t / (kRec * a.max_regions);
    const int K = a.region_count[b];
    long long v = 0;
    if (r < K) {
        const long long *raw = a.raw + ((int64_t)b * kMaxR + r) * kRec;
        v = raw[fld];
        if (fld == F_ANCHOR) v = a.sel[b * kMaxR + r];
        if ((fld == F_MINMM || fld == F_MAXMM) && raw[F_ND] == 0) v = 0;
    }
    a.records[t] = v;
}

// ------------------------------------------------------------------------------------------------ planes
struct PlaneArgs {
    const uint8_t *region_map;
    const uint16_t *depth_mm;
    const int32_t *sizes, *region_count;
    const long long *records;
    double *planes;
    long long *partial;                                   // [B][nb][32][kNI int64 | kND f64]
    int64_t plane;
    int32_t B, Fh, Fw, max_regions, lo_mm, hi_mm, nb;
};

// RESID 0: the ten moments of every region, coordinates relative to the region's (x0, y0); 1: the sum of squared residuals
template <int RESID>
__global__ __launch_bounds__(kThreads) void plane_moments_kernel(const PlaneArgs a) {
#pragma clang fp contract(off)
    __shared__ long long pi[4][kMaxR][kNI];
    __shared__ double pd[4][kMaxR][kND];
    __shared__ int ox[kMaxR], oy[kMaxR];
    __shared__ double ca[kMaxR], cb[kMaxR], cg[kMaxR];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    const int K = min(max(a.region_count[b], 0), a.max_regions);
    for (int k = threadIdx.x; k < 4 * kMaxR * kNI; k += kThreads) (&pi[0][0][0])[k] = 0;
    for (int k = threadIdx.x; k < 4 * kMaxR * kND; k += kThreads) (&pd[0][0][0])[k] = 0.0;
    if ((int)threadIdx.x < kMaxR) {
        const int r = threadIdx.x;
        const long long *rec = a.records + ((int64_t)b * a.max_regions + r) * kRec;
        ox[r] = r < K ? (int)rec[F_X0] : 0;
        oy[r] = r < K ? (int)rec[F_Y0] : 0;
        const double *pl = a.planes + ((int64_t)b * a.max_regions + r) * 6;
        const bool fit = RESID && r < K && pl[5] == 0.0;
        ca[r] = fit ? pl[0] : 0.0; cb[r] = fit ? pl[1] : 0.0; cg[r] = fit ? pl[2] : 0.0;
    }
    __syncthreads();
    const uint8_t *__restrict__ M = a.region_map + b * a.plane;
    const uint16_t *__restrict__ D = a.depth_mm + b * a.plane;
    for (int y = blk; y < f.fh; y += a.nb) {
        for (int xt = 0; xt < f.fw; xt += kThreads) {     // uniform bounds: every lane of a wave reaches the ballots
            const int x = xt + threadIdx.x;
            int rank = 0, mm = 0;
            if (x < f.fw) {
                rank = M[(int64_t)y * a.Fw + x];
                mm = D[(int64_t)y * a.Fw + x];
                if (rank > K || mm < a.lo_mm || mm > a.hi_mm) rank = 0;
            }
            unsigned long long todo = __ballot(rank > 0);
            while (todo) {                                // one round per region present in the wave, in lane order
                const int r = __shfl(rank, __builtin_ctzll(todo), 64);
                const bool mine = rank == r;
                todo &= ~__ballot(mine);
                const double w = mine ? 1000.0 / (double)mm : 0.0;
                if (RESID) {
                    fit_add_residual(mine ? fit_residual(w, ca[r - 1], cb[r - 1], cg[r - 1], x, y) : 0.0, lane, pd[wave][r - 1]);
                } else {
                    const long long dx = mine ? x - ox[r - 1] : 0, dy = mine ? y - oy[r - 1] : 0;
                    fit_add_moments(mine, dx, dy, w, lane, pi[wave][r - 1], pd[wave][r - 1]);
                }
            }
        }
    }
    __syncthreads();
    long long *out = a.partial + ((int64_t)b * kPlaneBlocks + blk) * kMaxR * (kNI + kND);
    fit_store_partial(pi, pd, out, kMaxR, threadIdx.x, kThreads);
}

// one wave per (region, image): folds the workgroups' partial records in ascending order, then one thread solves
template <int RESID>
__global__ __launch_bounds__(64) void plane_solve_kernel(const PlaneArgs a) {
#pragma clang fp contract(off)
    __shared__ long long si[kNI];
    __shared__ double sd[kND];
    const int r = blockIdx.x, b = blockIdx.y, q = threadIdx.x;
    if (r >= a.max_regions) return;
    const int K = min(max(a.region_count[b], 0), a.max_regions);
    double *pl = a.planes + ((int64_t)b * a.max_regions + r) * 6;
    if (r >= K) {
        if (!RESID && q < 6) pl[q] = 0.0;
        return;
    }
    const long long *part = a.partial + (int64_t)b * kPlaneBlocks * kMaxR * (kNI + kND) + r * (kNI + kND);
    fit_fold(part, a.nb, (int64_t)kMaxR * (kNI + kND), q, si, sd);
    __syncthreads();
    if (q != 0) return;
    if (RESID) {
        if (pl[5] == 0.0) pl[3] = sqrt(sd[0] / pl[4]);
        return;
    }
    const long long *rec = a.records + ((int64_t)b * a.max_regions + r) * kRec;
    const PlaneFit fit = fit_solve(si, sd, rec[F_X0], rec[F_Y0]);
    pl[0] = fit.alpha;
    pl[1] = fit.beta;
    pl[2] = fit.gamma;
    pl[3] = __builtin_nan("");                            // of a fitted plane the residual pass writes it
    pl[4] = fit.n;
    pl[5] = fit.flat ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------------ planar depth
struct PlanarArgs {
    const uint8_t *region_map;
    const uint16_t *depth_mm;
    const float *depth;                                   // may be null: millimetres / 1000
    const int32_t *sizes, *region_count;
    const double *planes;
    float *out;
    uint16_t *out_mm;
    int64_t plane;
    int32_t B, Fh, Fw, max_regions;
    float dmin, dmax;
};

__global__ __launch_bounds__(kThreads) void depth_planar_kernel(const PlanarArgs a) {
#pragma clang fp contract(off)
    __shared__ double ca[kMaxR], cb[kMaxR], cg[kMaxR];
    __shared__ int fit[kMaxR];
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * kThreads + threadIdx.x;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    if ((int)threadIdx.x < kMaxR) {
        const int r = threadIdx.x;
        const int K = min(max(a.region_count[b], 0), a.max_regions);
        const double *pl = a.planes + ((int64_t)b * a.max_regions + (r < a.max_regions ? r : 0)) * 6;
        fit[r] = r < K && pl[5] == 0.0;
        ca[r] = pl[0]; cb[r] = pl[1]; cg[r] = pl[2];
    }
    __syncthreads();
    if (x >= a.Fw) return;
    const int64_t at = b * a.plane + (int64_t)y * a.Fw + x;
    float v = 0.f;
    unsigned short mm = 0;
    if (y < f.fh && x < f.fw) {
        mm = a.depth_mm[at];
        v = a.depth ? a.depth[at] : __fdiv_rn((float)mm, 1000.0f);
        const int rank = a.region_map[at];
        if (rank > 0 && rank <= kMaxR && fit[rank - 1]) {
            const double den = (ca[rank - 1] * (double)x + cb[rank - 1] * (double)y) + cg[rank - 1];
            if (den > 0.0) {
                double z = 1.0 / den;
                z = z < (double)a.dmin ? (double)a.dmin : z;
                z = z > (double)a.dmax ? (double)a.dmax : z;
                v = (float)z;
                mm = to_mm(v);
            }
        }
    }
    a.out[at] = v;
    a.out_mm[at] = mm;
}

bool bad_dims(int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions) {
    return B < 1 || B > kMaxB || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384 || max_regions < 1 || max_regions > kMaxR;
}
int plane_blocks(int Fh) { return Fh < kPlaneBlocks ? Fh : kPlaneBlocks; }

}  // namespace

// bytes of gwd_query_workspace(GWD_WS_REGIONS, {B, Fh, Fw, max_candidates}) (optim.hip)
int64_t gwd_regions_workspace_bytes(int64_t B, int64_t Fh, int64_t Fw, int64_t maxcand) {
    if (B < 1 || B > kMaxB || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384 || maxcand < 1 || maxcand > (1 << 24)) return -1;
    return layout(B, Fh, Fw, maxcand).total;
}

extern "C" int gwd_glass_regions(const uint8_t *labels, const uint16_t *depth_mm, const int32_t *sizes, int32_t B, int32_t Fh,
                                 int32_t Fw, int32_t max_regions, int32_t min_area, int32_t connectivity, int32_t max_candidates,
                                 int32_t lo_mm, int32_t hi_mm, void *workspace, uint8_t *region_map, int32_t *region_count,
                                 int32_t *region_total, int64_t *records, void *stream) {
    if (!labels || !depth_mm || !sizes || !workspace || !region_map || !region_count || !region_total || !records) return -1;
    if (bad_dims(B, Fh, Fw, max_regions) || min_area < 1 || max_candidates < 1 || max_candidates > (1 << 24)) return -1;
    if (lo_mm < 1 || hi_mm > 65535 || lo_mm > hi_mm) return -1;
    if (connectivity != 4 && connectivity != 8) return -2;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)depth_mm & 1) || ((uintptr_t)sizes & 3) || ((uintptr_t)region_count & 3) ||
        ((uintptr_t)region_total & 3) || ((uintptr_t)records & 7))
        return -3;
    const Layout l = layout(B, Fh, Fw, max_candidates);
    char *ws = (char *)workspace;
    CcArgs a;
    a.labels = labels; a.depth_mm = depth_mm; a.sizes = sizes;
    a.counters = (int32_t *)(ws + l.counters); a.sel = (int32_t *)(ws + l.sel); a.cand = (int32_t *)(ws + l.cand);
    a.parent = (int32_t *)(ws + l.parent); a.area = (int32_t *)(ws + l.area); a.raw = (long long *)(ws + l.raw);
    a.region_map = region_map; a.region_count = region_count; a.region_total = region_total; a.records = (long long *)records;
    a.plane = (int64_t)Fh * Fw;
    a.B = B; a.Fh = Fh; a.Fw = Fw; a.max_regions = max_regions; a.min_area = min_area; a.conn8 = connectivity == 8;
    a.maxcand = max_candidates; a.lo_mm = lo_mm; a.hi_mm = hi_mm;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((Fw + kThreads - 1) / kThreads, Fh, B);
    cc_init_kernel<<<grid, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cc_merge_kernel<<<grid, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    const dim3 chunks((Fw + kThreads - 1) / kThreads, (Fh + kRows - 1) / kRows, B);
    cc_flatten_kernel<<<chunks, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cc_candidates_kernel<<<chunks, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cc_select_kernel<<<B, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cc_records_kernel<<<chunks, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cc_finish_kernel<<<(B * max_regions * kRec + kThreads - 1) / kThreads, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_region_planes(const uint8_t *region_map, const uint16_t *depth_mm, const int32_t *sizes,
                                 const int32_t *region_count, const int64_t *records, int32_t B, int32_t Fh, int32_t Fw,
                                 int32_t max_regions, int32_t lo_mm, int32_t hi_mm, void *workspace, double *planes,
                                 void *stream) {
    if (!region_map || !depth_mm || !sizes || !region_count || !records || !workspace || !planes) return -1;
    if (bad_dims(B, Fh, Fw, max_regions)) return -1;
    if (lo_mm < 1 || hi_mm > 65535 || lo_mm > hi_mm) return -1;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)depth_mm & 1) || ((uintptr_t)sizes & 3) || ((uintptr_t)region_count & 3) ||
        ((uintptr_t)records & 7) || ((uintptr_t)planes & 7))
        return -3;
    PlaneArgs a;
    a.region_map = region_map; a.depth_mm = depth_mm; a.sizes = sizes; a.region_count = region_count;
    a.records = (const long long *)records; a.planes = planes;
    a.partial = (long long *)((char *)workspace + partial_offset(B));
    a.plane = (int64_t)Fh * Fw;
    a.B = B; a.Fh = Fh; a.Fw = Fw; a.max_regions = max_regions; a.lo_mm = lo_mm; a.hi_mm = hi_mm; a.nb = plane_blocks(Fh);
    const hipStream_t s = (hipStream_t)stream;
    plane_moments_kernel<0><<<dim3(a.nb, B), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    plane_solve_kernel<0><<<dim3(max_regions, B), 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    plane_moments_kernel<1><<<dim3(a.nb, B), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    plane_solve_kernel<1><<<dim3(max_regions, B), 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_depth_planar(const uint8_t *region_map, const uint16_t *depth_mm, const float *depth, const int32_t *sizes,
                                const int32_t *region_count, const double *planes, int32_t B, int32_t Fh, int32_t Fw,
                                int32_t max_regions, float min_depth, float max_depth, float *depth_planar,
                                uint16_t *depth_planar_mm, void *stream) {
    if (!region_map || !depth_mm || !sizes || !region_count || !planes || !depth_planar || !depth_planar_mm) return -1;
    if (bad_dims(B, Fh, Fw, max_regions) || !(min_depth < max_depth) || !(min_depth > 0.f)) return -1;
    if (((uintptr_t)depth_mm & 1) || ((uintptr_t)depth & 3) || ((uintptr_t)sizes & 3) || ((uintptr_t)region_count & 3) ||
        ((uintptr_t)planes & 7) || ((uintptr_t)depth_planar & 3) || ((uintptr_t)depth_planar_mm & 1))
        return -3;
    PlanarArgs a;
    a.region_map = region_map; a.depth_mm = depth_mm; a.depth = depth; a.sizes = sizes; a.region_count = region_count;
    a.planes = planes; a.out = depth_planar; a.out_mm = depth_planar_mm;
    a.plane = (int64_t)Fh * Fw;
    a.B = B; a.Fh = Fh; a.Fw = Fw; a.max_regions = max_regions; a.dmin = min_depth; a.dmax = max_depth;
    depth_planar_kernel<<<dim3((Fw + kThreads - 1) / kThreads, Fh, B), kThreads, 0, (hipStream_t)stream>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

// Dense metrics at FRAME size: what InferenceSession.predict_frames returns (fp32 depth and uint8 labels, [B][Fh][Fw], top-left
// aligned frames of different sizes) scored against the ground truth as the data set stores it - millimetres in 16 or 32 bits and
// the raw label plane of each frame, read in place - with the per-pixel arithmetic of eval_partial_kernel (evalterms.h), broken
// down by region: all / glass / non-glass / up to eight GT-depth bins.  8 bytes per pixel (4 + 1 prediction, 2 + 1 ground truth).
//
// ONE launch, no memset, no floating-point atomics.  A frame is cut into `nb` workgroups by its pixel count alone and the grid has
// one SLICE of nb workgroups per pair of regions: slice 0 keeps (glass, non-glass) and the confusion counts, slice 1 + j keeps
// bins (2j, 2j + 1); "all" is glass + non-glass, formed in the fold.  A thread therefore holds two accumulator sets (eight int32
// counters and twelve f64 sums), never R x 10.  Every workgroup writes one partial record; the workgroup that draws a frame's
// last ticket folds the frame's records in a fixed tree over their indices and writes its sums / measures / confusion; the
// workgroup that draws the call's last ticket adds the measures to the running totals in image order and puts the tickets back
// to zero.
//
// Batch invariance: logical pixel i = y * fw + x of a frame belongs to unit i / 8, unit u to thread u % 256 of workgroup
// (u / 256) % nb, which takes its units in ascending order and the pixels of a unit in ascending order - on the 16-byte path
// (a unit is eight neighbours of one row) and on the element-wise path alike, so the slot, the other frames, Fh x Fw and the
// alignment of the planes change no bit of a frame's record.
#include "common.h"
#include "evalterms.h"

namespace {

constexpr int NSUM = GWD_EVAL_NSUM;
constexpr int kThreads = 256;
constexpr int kUnit = 8;                                  // pixels of one thread step
constexpr int kMaxBlocks = 256;                           // workgroups of one frame and slice, at most
constexpr int kMaxSlices = 1 + GWD_EVAL_FRAMES_MAX_BINS / 2;
constexpr int kRec = 2 * NSUM;                            // f64 values of a partial record: two accumulator sets
constexpr int kTicketBytes = 128;                         // GWD_EVAL_FRAMES_BATCH frame tickets + the call's, padded

static_assert(GWD_EVAL_FRAMES_WS_BYTES == kTicketBytes + (int64_t)GWD_EVAL_FRAMES_BATCH * kMaxBlocks * 4 * 8 +
                                              (int64_t)GWD_EVAL_FRAMES_BATCH * kMaxSlices * kMaxBlocks * kRec * 8,
              "workspace layout");

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct FramesArgs {
    gwd_frame_eval_job j[GWD_EVAL_FRAMES_BATCH];
    int32_t block0[GWD_EVAL_FRAMES_BATCH], nb[GWD_EVAL_FRAMES_BATCH], vec[GWD_EVAL_FRAMES_BATCH];
    const float *depth;
    const uint8_t *label;
    int64_t plane, offset;                                // Fh * Fw; first image record written
    int32_t Fw, n, gt_bytes, n_bins, slices;
    float dmin, dmax;
    float edges[GWD_EVAL_FRAMES_MAX_BINS + 2];            // one spare, so that the pair (2j, 2j + 1) always has three edges
    unsigned *tickets;
    long long *pconf;
    double *psum;
    double *sums, *measures, *running;
    long long *conf, *confusion;
};

// publish what this workgroup stored, draw a ticket; true in every thread of the workgroup that drew `last`.  Stores are drained
// by every wave, one lane releases at agent scope (the partial records may sit in another XCD's L2) and the drawing workgroup
// acquires before any of its threads reads them.
__device__ __forceinline__ bool draw_ticket(unsigned *ticket, unsigned last, int *flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = t == last ? 1 : 0;
    }
    __syncthreads();
    return *flag != 0;
}

__global__ __launch_bounds__(kThreads) void eval_frames_kernel(const FramesArgs a) {
    __shared__ double shd[4][12];
    __shared__ int shi[4][12];
    __shared__ double fold[kMaxSlices * kRec];
    __shared__ double foldw[4][kRec];
    __shared__ long long foldc[4], foldcw[4][4];
    __shared__ double stage[GWD_EVAL_FRAMES_BATCH * (GWD_EVAL_FRAMES_MAX_BINS + 3) * NSUM];
    __shared__ long long stagec[GWD_EVAL_FRAMES_BATCH * 4];
    __shared__ double reg[GWD_EVAL_FRAMES_MAX_BINS + 3][NSUM];
    __shared__ int flag;

    int ji = 0;
#pragma unroll 1
    for (int k = 1; k < a.n; ++k)
        if ((int)blockIdx.x >= a.block0[k]) ji = k;
    const gwd_frame_eval_job job = a.j[ji];
    const int nb = a.nb[ji], local = blockIdx.x - a.block0[ji];
    const int slice = local / nb, blk = local - slice * nb;
    const bool vec = a.vec[ji] != 0, wide = a.gt_bytes == 4;
    const int fw = job.fw;
    const int64_t npix = (int64_t)job.fh * fw, nunits = (npix + kUnit - 1) / kUnit;
    const float *__restrict__ pd = a.depth + ji * a.plane;
    const uint8_t *__restrict__ pl = a.label + ji * a.plane;
    const uint8_t *__restrict__ gl = job.gt_label;
    const uint16_t *__restrict__ g16 = (const uint16_t *)job.gt_depth_mm;
    const int32_t *__restrict__ g32 = (const int32_t *)job.gt_depth_mm;
    const float dmin = a.dmin, dmax = a.dmax;
    // slice 0: set A = glass, set B = non-glass.  slice 1 + j: set A = bin 2j = [e0, e1), set B = bin 2j + 1 = [e1, e2)
    const int binA = 2 * (slice - 1);
    const float e0 = slice ? a.edges[binA] : 0.f, e1 = slice ? a.edges[binA + 1] : 0.f, e2 = slice ? a.edges[binA + 2] : 0.f;
    const bool hasB = slice == 0 || binA + 1 < a.n_bins;

    double sa[6], sb[6];
    int ca[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0}, cf[4] = {0, 0, 0, 0};       // per-thread pixel counts stay far below 2^31
#pragma unroll
    for (int k = 0; k < 6; ++k) sa[k] = sb[k] = 0.0;

    for (int64_t u = (int64_t)blk * kThreads + threadIdx.x; u < nunits; u += (int64_t)nb * kThreads) {
        const int64_t i0 = u * kUnit;
        float p[kUnit];
        int mm[kUnit];
        unsigned lp[kUnit], lt[kUnit];
        unsigned live = 0;
        if (vec) {                                       // fw % 8 == 0: the unit is eight neighbours of one row, all inside the frame
            const int64_t y = i0 / fw, x = i0 - y * fw, at = y * a.Fw + x;
            const f32x4 p0 = *(const f32x4 *)(pd + at), p1 = *(const f32x4 *)(pd + at + 4);
            const u32x2 l = *(const u32x2 *)(pl + at), t = *(const u32x2 *)(gl + i0);
            p[0] = p0.x; p[1] = p0.y; p[2] = p0.z; p[3] = p0.w; p[4] = p1.x; p[5] = p1.y; p[6] = p1.z; p[7] = p1.w;
            if (wide) {
                const i32x4 m0 = *(const i32x4 *)(g32 + i0), m1 = *(const i32x4 *)(g32 + i0 + 4);
                mm[0] = m0.x; mm[1] = m0.y; mm[2] = m0.z; mm[3] = m0.w; mm[4] = m1.x; mm[5] = m1.y; mm[6] = m1.z; mm[7] = m1.w;
            } else {
                const u16x8 m = *(const u16x8 *)(g16 + i0);
                mm[0] = m.s0; mm[1] = m.s1; mm[2] = m.s2; mm[3] = m.s3; mm[4] = m.s4; mm[5] = m.s5; mm[6] = m.s6; mm[7] = m.s7;
            }
#pragma unroll
            for (int k = 0; k < kUnit; ++k) {
                lp[k] = ((k < 4 ? l.x : l.y) >> (8 * (k & 3))) & 255u;
                lt[k] = ((k < 4 ? t.x : t.y) >> (8 * (k & 3))) & 255u;
            }
            live = 255u;
        } else {
            int64_t y = i0 / fw;
            int x = (int)(i0 - y * fw) - 1;
#pragma unroll
            for (int k = 0; k < kUnit; ++k) {
                const int64_t i = i0 + k;
                p[k] = 0.f; mm[k] = 0; lp[k] = 255u; lt[k] = 0u;
                if (++x == fw) { x = 0; ++y; }
                if (i < npix) {
                    const int64_t at = y * a.Fw + x;
                    p[k] = pd[at];
                    lp[k] = pl[at];
                    lt[k] = gl[i];
                    mm[k] = wide ? g32[i] : (int)g16[i];
                    live |= 1u << k;
                }
            }
        }
#pragma unroll 1                                          // one copy of the arithmetic: the unit's values are picked by selects
        for (int k = 0; k < kUnit; ++k) {
            if (!((live >> k) & 1u)) continue;
            const bool glass = lt[k] > 0u;                                  // glassrgbd_norhint.py:275
            if (slice == 0) {
                const unsigned c = (glass ? 2u : 0u) + lp[k];               // a predicted label above 1 matches no entry
#pragma unroll
                for (int q = 0; q < 4; ++q) cf[q] += (lp[k] < 2u && c == (unsigned)q) ? 1 : 0;
            }
            const float g = __fdiv_rn((float)mm[k], 1000.0f);               // :273
            if (!eval_valid(g, dmin, dmax)) continue;
            const bool inA = slice == 0 ? glass : (g >= e0 && g < e1);
            const bool inB = slice == 0 ? !glass : (hasB && g >= e1 && g < e2);
            if (!(inA || inB)) continue;
            float t[NSUM];
            eval_terms(g, eval_clamp(p[k], dmin, dmax), t);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int hit = t[q] != 0.0f ? 1 : 0;
                ca[q] += inA ? hit : 0;
                cb[q] += inB ? hit : 0;
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const double d = (double)t[4 + q];
                sa[q] += inA ? d : 0.0;
                sb[q] += inB ? d : 0.0;
            }
        }
    }

    // workgroup record: [set][count, d1, d2, d3, six sums] as f64 (the counts are exact) + the four confusion counts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double va = wave_sum_d(sa[q]), vb = wave_sum_d(sb[q]);
        if (lane == 0) { shd[wave][q] = va; shd[wave][6 + q] = vb; }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        int v = q < 4 ? ca[q & 3] : (q < 8 ? cb[q & 3] : cf[q & 3]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) shi[wave][q] = v;
    }
    __syncthreads();
    const int64_t rec = ((int64_t)ji * kMaxSlices + slice) * kMaxBlocks + blk;
    if (threadIdx.x < 12) {
        const int q = threadIdx.x, set = q / 6, w = q - set * 6;
        a.psum[rec * kRec + set * NSUM + 4 + w] = (shd[0][q] + shd[1][q]) + (shd[2][q] + shd[3][q]);
    }
    if (threadIdx.x >= 64 && threadIdx.x < 76) {
        const int q = threadIdx.x - 64;
        const long long v = (long long)shi[0][q] + shi[1][q] + shi[2][q] + shi[3][q];
        if (q < 8) a.psum[rec * kRec + (q >> 2) * NSUM + (q & 3)] = (double)v;
        else if (slice == 0) a.pconf[((int64_t)ji * kMaxBlocks + blk) * 4 + (q & 3)] = v;
    }

    // ---- the frame's last workgroup folds its records
    if (!draw_ticket(a.tickets + ji, (unsigned)(a.slices * nb - 1), &flag)) return;
    const int R = 3 + a.n_bins;
    // thread j takes record j (zeros beyond nb): every load is in flight at once, then a fixed butterfly over the 64 lanes and
    // the four waves in order - the association depends on nothing but the record's index
    for (int sl = 0; sl < a.slices; ++sl) {
        double *ps = a.psum + (((int64_t)ji * kMaxSlices + sl) * kMaxBlocks + threadIdx.x) * kRec;
        double v[kRec];
#pragma unroll
        for (int k = 0; k < kRec; ++k) v[k] = (int)threadIdx.x < nb ? ps[k] : 0.0;
#pragma unroll
        for (int k = 0; k < kRec; ++k) {
            const double d = wave_sum_d(v[k]);
            if (lane == 0) foldw[wave][k] = d;
        }
        __syncthreads();
        if (threadIdx.x < kRec) fold[sl * kRec + threadIdx.x] = (foldw[0][threadIdx.x] + foldw[1][threadIdx.x]) + (foldw[2][threadIdx.x] + foldw[3][threadIdx.x]);
        __syncthreads();
    }
    {
        long long *pc = a.pconf + ((int64_t)ji * kMaxBlocks + threadIdx.x) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long long c = (int)threadIdx.x < nb ? pc[k] : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0) foldcw[wave][k] = c;
        }
        __syncthreads();
        if (threadIdx.x < 4) foldc[threadIdx.x] = foldcw[0][threadIdx.x] + foldcw[1][threadIdx.x] + foldcw[2][threadIdx.x] + foldcw[3][threadIdx.x];
    }
    __syncthreads();
    const int64_t img = a.offset + ji;
    if (threadIdx.x < R * NSUM) {
        const int r = threadIdx.x / NSUM, k = threadIdx.x - r * NSUM;
        const double v = r == 0 ? fold[k] + fold[NSUM + k] : (r < 3 ? fold[(r - 1) * NSUM + k] : fold[kRec + (r - 3) * NSUM + k]);
        reg[r][k] = v;
        a.sums[(img * R + r) * NSUM + k] = v;
    }
    if (threadIdx.x >= 128 && threadIdx.x < 132) a.conf[img * 4 + (threadIdx.x - 128)] = foldc[threadIdx.x - 128];
    __syncthreads();
    if (threadIdx.x < R) {
        double s[NSUM], m[9];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s[k] = reg[threadIdx.x][k];
        eval_measures(s, m);
#pragma unroll
        for (int k = 0; k < 9; ++k) a.measures[(img * R + threadIdx.x) * 9 + k] = m[k];
    }

    // ---- the call's last workgroup: running totals in image order (engine_glassrgbd.py:262-263), skipping empty regions
    if (!draw_ticket(a.tickets + GWD_EVAL_FRAMES_BATCH, (unsigned)(a.n - 1), &flag)) return;
    for (int i = threadIdx.x; i < a.n * R * NSUM; i += kThreads) {                 // the call's records into LDS, all loads in flight
        const int b = i / (R * NSUM), rem = i - b * (R * NSUM), r = rem / NSUM, k = rem - r * NSUM;
        const int64_t at = (a.offset + b) * R + r;
        stage[i] = k < 9 ? a.measures[at * 9 + k] : a.sums[at * NSUM];               // [b][r][nine measures, the pixel count]
    }
    if (threadIdx.x < a.n * 4) stagec[threadIdx.x] = a.conf[a.offset * 4 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < R) {
        const int r = threadIdx.x;
        double run[NSUM];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) run[k] = a.running[r * NSUM + k];
        for (int b = 0; b < a.n; ++b) {
            const double *m = stage + (b * R + r) * NSUM;
            if (m[9] != 0.0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) run[k] += m[k];
                run[9] += 1.0;
            }
        }
#pragma unroll
        for (int k = 0; k < NSUM; ++k) a.running[r * NSUM + k] = run[k];
    }
    if (threadIdx.x >= 128 && threadIdx.x < 132) {
        const int c = threadIdx.x - 128;
        long long v = a.confusion[c];
        for (int b = 0; b < a.n; ++b) v += stagec[b * 4 + c];
        a.confusion[c] = v;
    }
    if (threadIdx.x >= 192 && threadIdx.x < 192 + GWD_EVAL_FRAMES_BATCH + 1)     // every ticket of this call has been drawn
        __hip_atomic_store(a.tickets + (threadIdx.x - 192), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int frame_blocks(int64_t npix) {                          // a function of the frame's pixel count alone
    const int64_t nb = (npix + kThreads * kUnit - 1) / (kThreads * kUnit);
    return (int)(nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb));
}

}  // namespace

extern "C" int gwd_eval_frames(const gwd_frame_eval_job *jobs, int32_t n_jobs, const float *depth, const uint8_t *label, int32_t Fh,
                               int32_t Fw, int32_t gt_bytes, float min_depth, float max_depth, const float *bin_edges,
                               int32_t n_bins, void *workspace, int64_t image_offset, double *sums, double *measures,
                               int64_t *conf, double *running, int64_t *confusion, void *stream) {
    if (!jobs || n_jobs < 1 || n_jobs > GWD_EVAL_FRAMES_BATCH || !depth || !label || Fh < 1 || Fw < 1) return -1;
    if (!workspace || ((uintptr_t)workspace & 15) || image_offset < 0 || !sums || !measures || !conf || !running || !confusion) return -1;
    if (n_bins < 0 || n_bins > GWD_EVAL_FRAMES_MAX_BINS || (n_bins > 0 && !bin_edges)) return -1;
    if (!(min_depth < max_depth)) return -1;
    if (gt_bytes != 2 && gt_bytes != 4) return -2;
    FramesArgs a;
    for (int k = 0; k < GWD_EVAL_FRAMES_MAX_BINS + 2; ++k) a.edges[k] = 0.f;
    for (int k = 0; k <= n_bins && n_bins > 0; ++k) {
        if (bin_edges[k] != bin_edges[k] || (k > 0 && bin_edges[k] < bin_edges[k - 1])) return -1;
        a.edges[k] = bin_edges[k];
    }
    a.slices = 1 + (n_bins + 1) / 2;
    int total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const gwd_frame_eval_job &j = jobs[i];
        if (!j.gt_depth_mm || !j.gt_label || j.fh < 1 || j.fw < 1 || j.fh > Fh || j.fw > Fw) return -1;
        if ((uintptr_t)j.gt_depth_mm & (uintptr_t)(gt_bytes - 1)) return -3;
        a.j[i] = j;
        a.nb[i] = frame_blocks((int64_t)j.fh * j.fw);
        a.block0[i] = total;
        a.vec[i] = Fw % 8 == 0 && j.fw % 8 == 0 && !((uintptr_t)depth & 15) && !((uintptr_t)label & 7) &&
                   !((uintptr_t)j.gt_depth_mm & 15) && !((uintptr_t)j.gt_label & 7);
        total += a.nb[i] * a.slices;
    }
    for (int i = n_jobs; i < GWD_EVAL_FRAMES_BATCH; ++i) {
        a.j[i] = gwd_frame_eval_job{nullptr, nullptr, 0, 0};
        a.nb[i] = a.block0[i] = a.vec[i] = 0;
    }
    a.depth = depth;
    a.label = label;
    a.plane = (int64_t)Fh * Fw;
    a.offset = image_offset;
    a.Fw = Fw;
    a.n = n_jobs;
    a.gt_bytes = gt_bytes;
    a.n_bins = n_bins;
    a.dmin = min_depth;
    a.dmax = max_depth;
    a.tickets = (unsigned *)workspace;
    a.pconf = (long long *)((char *)workspace + kTicketBytes);
    a.psum = (double *)((char *)workspace + kTicketBytes + (int64_t)GWD_EVAL_FRAMES_BATCH * kMaxBlocks * 4 * 8);
    a.sums = sums;
    a.measures = measures;
    a.running = running;
    a.conf = (long long *)conf;
    a.confusion = (long long *)confusion;
    eval_frames_kernel<<<total, kThreads, 0, (hipStream_t)stream>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

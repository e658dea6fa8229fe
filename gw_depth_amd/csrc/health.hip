// Guarded optimizer step: per-segment statistics of a flat fp32 buffer (sum of squares of the finite elements, largest finite
// magnitude, number of non-finite elements), the decision whether the step is applied, and AdamW reading that decision.
// One streaming pass over the buffer (the pass sqnorm_kernel makes), no atomics, no memset: every sum has one fixed order.
#include "common.h"
#include "adamw.h"

namespace {

constexpr int STAT_THREADS = 256;

struct Acc {
    double sumsq;
    float absmax;
    int nonfinite;
};

__device__ __forceinline__ void take(Acc &a, float v) {
    const bool finite = (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
    const double d = finite ? (double)v : 0.0;
    a.sumsq = fma(d, d, a.sumsq);                       // fp32 x fp32 is exact in fp64: one rounding, the add's
    a.absmax = fmaxf(a.absmax, finite ? fabsf(v) : 0.f);
    a.nonfinite += finite ? 0 : 1;
}

// all 64 lanes end with the same value: a + b is commutative, so both partners of an xor step form the same sum
__device__ __forceinline__ Acc wave_fold(Acc a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.sumsq += __shfl_xor(a.sumsq, o, 64);
        a.absmax = fmaxf(a.absmax, __shfl_xor(a.absmax, o, 64));
        a.nonfinite += __shfl_xor(a.nonfinite, o, 64);
    }
    return a;
}

// One workgroup per piece.  Thread t takes the float4 vectors t, t + 256, ... of the piece in that order, the waves fold by a fixed
// butterfly and wave 0..3 are added in that order: partial[c] depends on the piece's values alone.
__global__ __launch_bounds__(STAT_THREADS) void chunk_stats_kernel(const float *__restrict__ x, const gwd_health_chunk *__restrict__ chunks,
                                                                   gwd_segment_record *__restrict__ partial) {
    __shared__ double sh_s[STAT_THREADS / 64];
    __shared__ float sh_m[STAT_THREADS / 64];
    __shared__ int sh_n[STAT_THREADS / 64];
    const gwd_health_chunk ch = chunks[blockIdx.x];
    const float *px = x + ch.begin;                      // 16-byte aligned: begin is a multiple of 8 elements
    const int n4 = ch.len >> 2;
    const f32x4 *p4 = (const f32x4 *)px;
    Acc a = {0.0, 0.f, 0};
    int i = threadIdx.x;
    for (; i + 3 * STAT_THREADS < n4; i += 4 * STAT_THREADS) {      // four loads in flight per lane
        const f32x4 v0 = p4[i], v1 = p4[i + STAT_THREADS], v2 = p4[i + 2 * STAT_THREADS], v3 = p4[i + 3 * STAT_THREADS];
#pragma unroll
        for (int k = 0; k < 4; ++k) take(a, v0[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) take(a, v1[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) take(a, v2[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) take(a, v3[k]);
    }
    for (; i < n4; i += STAT_THREADS) {
        const f32x4 v = p4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) take(a, v[k]);
    }
    if ((int)threadIdx.x < (ch.len & 3)) take(a, px[n4 * 4 + threadIdx.x]);     // ragged end, element by element
    a = wave_fold(a);
    if ((threadIdx.x & 63) == 0) {
        sh_s[threadIdx.x >> 6] = a.sumsq;
        sh_m[threadIdx.x >> 6] = a.absmax;
        sh_n[threadIdx.x >> 6] = a.nonfinite;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        gwd_segment_record r;
        r.sumsq = ((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3];
        r.absmax = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
        r.nonfinite = sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3];
        partial[blockIdx.x] = r;
    }
}

__device__ __forceinline__ double lane_value(double v, int l) {      // l is a constant once the caller's loop is unrolled: v_readlane
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// a += the 64 records the lanes hold, sumsq in lane order 0, 1, 2, ... (a lane without a record holds zeros: + 0.0 changes nothing, the
// sums are >= +0).  All 64 lanes must be active; the result is wave-uniform.
__device__ __forceinline__ void add_in_lane_order(Acc &a, const gwd_segment_record &r) {
#pragma unroll
    for (int l = 0; l < 64; ++l) a.sumsq += lane_value(r.sumsq, l);
    a.absmax = fmaxf(a.absmax, wave_max(r.absmax));
    int nf = r.nonfinite;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
    a.nonfinite += nf;
}

// sum of rec[0 .. n) in ASCENDING index order, by one wave: 256 records are fetched at a time (four loads in flight per lane: the
// kernel is one wave, so the rounds' load latencies are all it waits for), then added 64 by 64
__device__ __forceinline__ Acc ordered_fold(const gwd_segment_record *__restrict__ rec, int n) {
    const int lane = threadIdx.x & 63;
    Acc a = {0.0, 0.f, 0};
    for (int base = 0; base < n; base += 256) {           // n is wave-uniform
        gwd_segment_record r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = base + 64 * j + lane;
            r[j] = gwd_segment_record{0.0, 0.f, 0};
            if (idx < n) r[j] = rec[idx];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) add_in_lane_order(a, r[j]);
    }
    return a;
}

// First piece whose segment is >= s (the table is in segment order), found by the whole wave: 64 probes per round, so a table of
// 4096 pieces takes two dependent loads where a binary search takes twelve.  Every round shrinks the span: it ends.
__device__ __forceinline__ int first_chunk_of(const gwd_health_chunk *__restrict__ chunks, int n_chunks, int s) {
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = n_chunks;                            // the answer lies in [lo, hi]
    while (hi > lo) {
        const int step = (hi - lo + 63) / 64;
        const int p = lo + lane * step;
        const bool less = p < hi && chunks[p].segment < s;             // monotone in p: true for the first k lanes
        const int k = __popcll(__ballot(less));
        if (k == 0) return lo;
        const int nhi = min(lo + k * step, hi);
        lo = lo + (k - 1) * step + 1;
        hi = nhi;
    }
    return lo;
}

// One wave per segment: its pieces follow each other in the table, and they are added in that order.
__global__ __launch_bounds__(STAT_THREADS) void segment_fold_kernel(const gwd_health_chunk *__restrict__ chunks, int n_chunks,
                                                                    const gwd_segment_record *__restrict__ partial,
                                                                    gwd_segment_record *__restrict__ out, int S) {
    const int s = blockIdx.x * (STAT_THREADS / 64) + (threadIdx.x >> 6);
    if (s >= S) return;                                   // whole waves leave: s is wave-uniform
    const int lane = threadIdx.x & 63;
    Acc a = {0.0, 0.f, 0};
    for (int base = first_chunk_of(chunks, n_chunks, s);; base += 64) {
        const int idx = base + lane;
        const bool mine = idx < n_chunks && chunks[idx].segment == s;
        gwd_segment_record r = {0.0, 0.f, 0};
        if (mine) r = partial[idx];
        add_in_lane_order(a, r);
        if (__ballot(mine) != ~0ull) break;               // the segment's pieces ended inside these 64 (idx < n_chunks bounds the loop)
    }
    if (lane == 0) {
        gwd_segment_record r;
        r.sumsq = a.sumsq;
        r.absmax = a.absmax;
        r.nonfinite = a.nonfinite;
        out[s] = r;
    }
}

__global__ __launch_bounds__(64) void health_decide_kernel(const gwd_segment_record *__restrict__ stats, int S, const float *__restrict__ loss,
                                                           gwd_health_ctl *__restrict__ ctl, gwd_health_record *__restrict__ ring, int ring_len,
                                                           int *__restrict__ bad, double b1, double b2, float max_norm, float grad_scale) {
    const Acc a = ordered_fold(stats, S);
    const int apply = a.nonfinite == 0 ? 1 : 0;
    if (!apply)
        for (int s = threadIdx.x; s < S; s += 64) bad[s] = stats[s].nonfinite;
    if (threadIdx.x != 0) return;
    gwd_health_ctl c = *ctl;
    c.sq = a.sumsq;
    c.nonfinite_total = a.nonfinite;
    c.apply = apply;
    c.applied += apply;
    c.skipped += 1 - apply;
    c.streak = apply ? 0 : c.streak + 1;
    if (apply) {
        const double t = (double)c.applied;
        c.bc1 = (float)(1.0 - pow(b1, t));
        c.bc2 = (float)(1.0 - pow(b2, t));
    }
    float clip = 1.0f;
    if (max_norm > 0.f) {
        // as adamw_kernel: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
        const float total = (float)sqrt(c.sq) * grad_scale;
        clip = fminf(max_norm / (total + 1e-6f), 1.0f);
    }
    c.clip_coef = clip;
    const float lv = loss ? loss[0] : 0.f;
    c.loss = lv;
    c.loss_finite = (loss && (__float_as_uint(lv) & 0x7f800000u) != 0x7f800000u) ? 1 : 0;
    c.reserved = 0;
    *ctl = c;
    gwd_health_record r;
    r.step = c.applied + c.skipped;
    r.grad_norm = sqrt(c.sq) * (double)grad_scale;
    r.clip_coef = clip;
    r.loss = lv;
    r.apply = apply;
    r.nonfinite_total = a.nonfinite;
    ring[(r.step - 1) % ring_len] = r;
}

// adamw_kernel of optim.hip (the same two functions of adamw.h), with sq / bc1 / bc2 read from the control block
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                            float *__restrict__ v, __bf16 *__restrict__ p16,
                                                            const gwd_health_ctl *__restrict__ ctl, int64_t n, float lr, float b1, float b2,
                                                            float eps, float wd, float max_norm, float grad_scale) {
    if (ctl->apply == 0) return;
    const float bc1 = ctl->bc1, bc2 = ctl->bc2;
    const float coef = adamw_coef(&ctl->sq, max_norm, grad_scale);
    const float step = lr / bc1, rs2 = rsqrtf(bc2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_element(pi, g[i], mi, vi, coef, lr, b1, b2, eps, wd, step, rs2);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (p16) p16[i] = (__bf16)pi;
    }
}

}  // namespace

static_assert(sizeof(gwd_segment_record) == 16 && sizeof(gwd_health_chunk) == 16, "health records are 16 bytes");
static_assert(sizeof(gwd_health_ctl) == 64 && sizeof(gwd_health_record) == 32, "control block 64 bytes, ring record 32");

int64_t gwd_health_workspace_bytes(int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks > INT32_MAX) return -1;
    return (n_chunks < 1 ? 1 : n_chunks) * (int64_t)sizeof(gwd_segment_record);
}

extern "C" int gwd_segment_stats(const float *x, const int64_t *seg_begin, const int64_t *seg_end, int32_t S, const gwd_health_chunk *chunks,
                                 int32_t n_chunks, void *partial, gwd_segment_record *out, void *stream) {
    if (!x || !seg_begin || !seg_end || !chunks || !partial || !out || S < 1 || n_chunks < 0) return -1;
    if (((uintptr_t)x & 15) != 0 || ((uintptr_t)partial & 7) != 0 || ((uintptr_t)out & 7) != 0) return -3;
    if (n_chunks > 0) {
        chunk_stats_kernel<<<n_chunks, STAT_THREADS, 0, (hipStream_t)stream>>>(x, chunks, (gwd_segment_record *)partial);
        GWD_CHECK_LAUNCH();
    }
    const int per = STAT_THREADS / 64;
    segment_fold_kernel<<<(S + per - 1) / per, STAT_THREADS, 0, (hipStream_t)stream>>>(chunks, n_chunks, (const gwd_segment_record *)partial,
                                                                                       out, S);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_health_decide(const gwd_segment_record *stats, int32_t S, const float *loss, gwd_health_ctl *ctl, gwd_health_record *ring,
                                 int32_t ring_len, int32_t *bad, double beta1, double beta2, float max_norm, float grad_scale, void *stream) {
    if (!stats || !ctl || !ring || !bad || S < 1 || ring_len < 1) return -1;
    health_decide_kernel<<<1, 64, 0, (hipStream_t)stream>>>(stats, S, loss, ctl, ring, ring_len, bad, beta1, beta2, max_norm, grad_scale);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_adamw_step_guarded(float *p, const float *g, float *m, float *v, void *p_bf16, const gwd_health_ctl *ctl, int64_t n,
                                      float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                      void *stream) {
    if (!p || !g || !m || !v || !ctl || n < 0) return -1;
    if (n == 0) return 0;
    int64_t b = (n + 255) / 256;
    const int grid = (int)(b > 4096 ? 4096 : b);
    adamw_guarded_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p, g, m, v, (__bf16 *)p_bf16, ctl, n, lr, beta1, beta2, eps, weight_decay,
                                                                max_norm, grad_scale);
    GWD_CHECK_LAUNCH();
    return 0;
}

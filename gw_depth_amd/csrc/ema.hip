// Exponential moving average of the fp32 master weights inside the AdamW pass, and the in-place exchange of weights and average.
//
// adamw_ema_kernel is adamw_kernel / adamw_guarded_kernel (the same two functions of adamw.h) plus one more fp32 stream:
//     ema' = fmaf(omd, p' - ema, ema),    omd = (float)(1 - d),    d = warmup ? min(decay, (1 + t) / (10 + t)) : decay   (fp64)
// 38 bytes per element: p, g, m, v, ema read; p, m, v, ema and the bf16 shadow written.  Purely bandwidth-bound, so the body moves
// 16 bytes per lane and stream (8 for the shadow) with EMA_UNROLL vectors of every stream in flight per lane; a scalar head runs
// up to the first 16-byte boundary and a scalar tail follows the body, through the same element function.  All fp32 ranges of a call
// share their offset from a 16-byte boundary (they are slices of flat buffers at equal offsets) and the shadow sits at the same
// ELEMENT offset from an 8-byte boundary: the entry points return -3 otherwise.  No atomics, no memset, no workspace.
#include "common.h"
#include "adamw.h"

namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_UNROLL = 2;          // float4 vectors per lane, stream and pass
constexpr int EMA_MAX_BLOCKS = 1024;   // 4 workgroups per CU: 16 waves x 64 lanes x 10 loads x 16 B = 160 KiB in flight per CU
static_assert((int64_t)EMA_MAX_BLOCKS * EMA_THREADS * EMA_UNROLL * 4 == GWD_EMA_PASS, "GWD_EMA_PASS is the element count of one pass");

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

struct Ranges {
    int head;          // elements before the first 16-byte boundary (0..3, at most n)
    int tail;          // elements behind the last whole vector (0..3)
    int64_t nvec;      // float4 vectors of the body
};

__host__ __device__ inline Ranges split(uintptr_t p, int64_t n) {
    Ranges r;
    const int64_t h = (int64_t)(((16 - (p & 15)) & 15) >> 2);
    r.head = (int)(h < n ? h : n);
    r.nvec = (n - r.head) >> 2;
    r.tail = (int)((n - r.head) & 3);
    return r;
}

__device__ __forceinline__ float ema_one_minus_decay(double decay, int warmup, int64_t t) {
    double d = decay;
    if (warmup) d = fmin(decay, (1.0 + (double)t) / (10.0 + (double)t));
    return (float)(1.0 - d);
}

__device__ __forceinline__ float ema_element(float omd, float pn, float e) {
#pragma clang fp contract(off)
    return __builtin_fmaf(omd, pn - e, e);         // p' == ema keeps ema bit for bit
}

__global__ __launch_bounds__(EMA_THREADS) void adamw_ema_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                                float *__restrict__ v, __bf16 *__restrict__ p16, float *__restrict__ ema,
                                                                const double *__restrict__ sq, const gwd_health_ctl *__restrict__ ctl,
                                                                int64_t n, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                                float bc2, float max_norm, float grad_scale, double ema_decay,
                                                                int ema_warmup, int64_t ema_t) {
    int64_t t = ema_t;
    if (ctl) {                                     // the guarded step: nothing is stored when the device decided to skip
        if (ctl->apply == 0) return;
        bc1 = ctl->bc1;
        bc2 = ctl->bc2;
        sq = &ctl->sq;
        t = ctl->applied - ema_t;
    }
    const float coef = adamw_coef(sq, max_norm, grad_scale);
    const float step = lr / bc1, rs2 = rsqrtf(bc2);
    const float omd = ema_one_minus_decay(ema_decay, ema_warmup, t);
    const Ranges r = split((uintptr_t)p, n);

    if (blockIdx.x == 0 && (int)threadIdx.x < 8) {              // lanes 0..3: the head, lanes 4..7: the tail
        const int k = threadIdx.x & 3;
        const bool is_tail = threadIdx.x >= 4;
        if (k < (is_tail ? r.tail : r.head)) {
            const int64_t i = is_tail ? r.head + 4 * r.nvec + k : k;
            float pi = p[i], mi = m[i], vi = v[i];
            adamw_element(pi, g[i], mi, vi, coef, lr, b1, b2, eps, wd, step, rs2);
            ema[i] = ema_element(omd, pi, ema[i]);
            p[i] = pi;
            m[i] = mi;
            v[i] = vi;
            if (p16) p16[i] = (__bf16)pi;
        }
    }

    f32x4 *p4 = (f32x4 *)(p + r.head), *m4 = (f32x4 *)(m + r.head), *v4 = (f32x4 *)(v + r.head), *e4 = (f32x4 *)(ema + r.head);
    const f32x4 *g4 = (const f32x4 *)(g + r.head);
    bf16x4 *s4 = p16 ? (bf16x4 *)(p16 + r.head) : nullptr;
    const int64_t G = (int64_t)gridDim.x * EMA_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x; base < r.nvec; base += G * EMA_UNROLL) {
        f32x4 P[EMA_UNROLL], Gr[EMA_UNROLL], M[EMA_UNROLL], V[EMA_UNROLL], E[EMA_UNROLL];
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            const int64_t i = base + u * G;
            if (i < r.nvec) {
                P[u] = p4[i];
                Gr[u] = g4[i];
                M[u] = m4[i];
                V[u] = v4[i];
                E[u] = e4[i];
            }
        }
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            const int64_t i = base + u * G;
            if (i < r.nvec) {
                bf16x4 S;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pi = P[u][k], mi = M[u][k], vi = V[u][k];
                    adamw_element(pi, Gr[u][k], mi, vi, coef, lr, b1, b2, eps, wd, step, rs2);
                    E[u][k] = ema_element(omd, pi, E[u][k]);
                    P[u][k] = pi;
                    M[u][k] = mi;
                    V[u][k] = vi;
                    S[k] = (__bf16)pi;
                }
                p4[i] = P[u];
                m4[i] = M[u];
                v4[i] = V[u];
                e4[i] = E[u];
                if (s4) s4[i] = S;
            }
        }
    }
}

__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(float *__restrict__ p, float *__restrict__ ema, __bf16 *__restrict__ p16,
                                                               int64_t n) {
    const Ranges r = split((uintptr_t)p, n);
    if (blockIdx.x == 0 && (int)threadIdx.x < 8) {
        const int k = threadIdx.x & 3;
        const bool is_tail = threadIdx.x >= 4;
        if (k < (is_tail ? r.tail : r.head)) {
            const int64_t i = is_tail ? r.head + 4 * r.nvec + k : k;
            const float pi = p[i], ei = ema[i];
            p[i] = ei;
            ema[i] = pi;
            if (p16) p16[i] = (__bf16)ei;
        }
    }
    f32x4 *p4 = (f32x4 *)(p + r.head), *e4 = (f32x4 *)(ema + r.head);
    bf16x4 *s4 = p16 ? (bf16x4 *)(p16 + r.head) : nullptr;
    const int64_t G = (int64_t)gridDim.x * EMA_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x; base < r.nvec; base += G * EMA_UNROLL) {
        f32x4 P[EMA_UNROLL], E[EMA_UNROLL];
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            const int64_t i = base + u * G;
            if (i < r.nvec) {
                P[u] = p4[i];
                E[u] = e4[i];
            }
        }
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            const int64_t i = base + u * G;
            if (i < r.nvec) {
                p4[i] = E[u];
                e4[i] = P[u];
                if (s4) {
                    bf16x4 S;
#pragma unroll
                    for (int k = 0; k < 4; ++k) S[k] = (__bf16)E[u][k];
                    s4[i] = S;
                }
            }
        }
    }
}

// every fp32 range at p's offset from a 16-byte boundary, the shadow at the same element offset from an 8-byte boundary
bool same_offsets(const void *p, const void *const *f32s, int k, const void *p16) {
    const uintptr_t off = (uintptr_t)p & 15;
    if (off & 3) return false;
    for (int i = 0; i < k; ++i)
        if (((uintptr_t)f32s[i] & 15) != off) return false;
    return !p16 || ((uintptr_t)p16 & 7) == off / 2;
}

int grid_for(int64_t n) {
    const int64_t per = (int64_t)EMA_THREADS * EMA_UNROLL * 4;
    const int64_t b = (n + per - 1) / per;
    return (int)(b > EMA_MAX_BLOCKS ? EMA_MAX_BLOCKS : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int gwd_adamw_step_ema(float *p, const float *g, float *m, float *v, void *p_bf16, float *ema, const double *sq,
                                  const gwd_health_ctl *ctl, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  float bias_corr1, float bias_corr2, float max_norm, float grad_scale, double ema_decay,
                                  int32_t ema_warmup, int64_t ema_t, void *stream) {
    if (!p || !g || !m || !v || !ema || n < 0 || !(ema_decay > 0.0 && ema_decay < 1.0)) return -1;
    if (n == 0) return 0;
    const void *f32s[4] = {g, m, v, ema};
    if (!same_offsets(p, f32s, 4, p_bf16)) return -3;
    adamw_ema_kernel<<<grid_for(n), EMA_THREADS, 0, (hipStream_t)stream>>>(p, g, m, v, (__bf16 *)p_bf16, ema, sq, ctl, n, lr, beta1, beta2, eps,
                                                                          weight_decay, bias_corr1, bias_corr2, max_norm, grad_scale,
                                                                          ema_decay, ema_warmup, ema_t);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_ema_swap(float *p, float *ema, void *p_bf16, int64_t n, void *stream) {
    if (!p || !ema || n < 0) return -1;
    if (n == 0) return 0;
    const void *f32s[1] = {ema};
    if (!same_offsets(p, f32s, 1, p_bf16)) return -3;
    ema_swap_kernel<<<grid_for(n), EMA_THREADS, 0, (hipStream_t)stream>>>(p, ema, (__bf16 *)p_bf16, n);
    GWD_CHECK_LAUNCH();
    return 0;
}

// Geometric part of the input pipeline on decoded images (second slice): the resizes, flips and crops of
// /root/reference/src/datasets/transforms_depth.py:59-372 as table-driven integer kernels, bit-exact with what the reference gets from
// Pillow through torchvision:
//   * RGB images: Image.resize(BILINEAR) = two separable passes over uint8 data with Pillow's fixed-point coefficients (22 fractional
//     bits, support scaled by max(1, in / out): the built-in antialiasing), each pass rounding to uint8 - gwd_resample_u8_pass.  The
//     coefficient and bound tables come from the caller (a few hundred doubles per image side, computed on the host exactly as
//     Pillow's precompute_coeffs / normalize_coeffs_8bpc do); a flip or a crop before the resize is an index map of the SOURCE
//     (base + step * i), so flip -> crop -> resize is one read of the original image.
//   * depth (int32 mm) and label (uint8) maps: Image.resize(NEAREST), flips, crops = one gather through per-axis index tables
//     (Pillow accumulates the source coordinate in double precision; the caller reproduces that on the host) - gwd_gather2d.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

// dst[o][j][c] (axis 0) or dst[j][o][c] (axis 1): o = output index along the resampled axis, j = index along the other axis
__global__ void resample_u8_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ bounds,
                                   const int32_t *__restrict__ kk, int ksize, int axis, int n_out, int other, int C, int64_t row_stride,
                                   int base0, int step0, int base1, int step1) {
    const int64_t total = (int64_t)n_out * other * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        int64_t r = i / C;
        int o, j;
        if (axis == 1) {                        // horizontal: dst [other rows][n_out][C]
            o = (int)(r % n_out);
            j = (int)(r / n_out);
        } else {                                // vertical: dst [n_out][other cols][C]
            j = (int)(r % other);
            o = (int)(r / other);
        }
        const int first = bounds[2 * o], cnt = bounds[2 * o + 1];
        const int32_t *k = kk + (size_t)o * ksize;
        int ss = 1 << (PRECISION_BITS - 1);
        const int64_t jo = (int64_t)base1 + (int64_t)step1 * j;
        for (int t = 0; t < cnt; ++t) {
            const int64_t a = (int64_t)base0 + (int64_t)step0 * (first + t);
            const int64_t off = axis == 1 ? (jo * row_stride + a * C + c) : (a * row_stride + jo * C + c);
            ss += (int)src[off] * k[t];
        }
        ss >>= PRECISION_BITS;
        dst[i] = (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
    }
}

template <int EB>
__global__ void gather2d_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ ytab,
                                const int32_t *__restrict__ xtab, int oh, int ow, int64_t row_stride_bytes) {
    const int64_t total = (int64_t)oh * ow;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % ow), y = (int)(i / ow);
        const uint8_t *p = src + (int64_t)ytab[y] * row_stride_bytes + (int64_t)xtab[x] * EB;
        uint8_t *q = dst + i * EB;
#pragma unroll
        for (int b = 0; b < EB; ++b) q[b] = p[b];
    }
}

// ---- grouped forms: the passes of a whole BATCH of frames in one launch each.  The job records travel by value in the kernel
// arguments (as gwd_colsum_batch's do), a workgroup finds its job through the block0 prefix, and every job's tables sit at int32
// offsets inside one device buffer the caller uploaded once.  One thread per output PIXEL: its C bytes share the bounds, the
// coefficients and the address arithmetic.
constexpr int JOB_BLOCKS_MAX = 4096;       // per job; a job with more pixels than 256 * this strides over them

struct ResampleBatch {
    gwd_resample_job j[GWD_AUGMENT_BATCH];
    int n;
};

template <int C, int AXIS>
__global__ __launch_bounds__(256) void resample_u8_batch_kernel(const ResampleBatch b, const int32_t *__restrict__ tables) {
    int ji = 0;
#pragma unroll 1
    for (int k = 1; k < b.n; ++k)
        if ((int)blockIdx.x >= b.j[k].block0) ji = k;
    const gwd_resample_job job = b.j[ji];
    const int32_t *__restrict__ bounds = tables + job.bounds_off;
    const int32_t *__restrict__ kk = tables + job.kk_off;
    const uint8_t *__restrict__ src = job.src;
    const int n_out = job.n_out, other = job.other;
    const int total = n_out * other;                                          // < 2^31: checked on the host
    const int64_t rs = job.src_row_stride;
    const int64_t tap_stride = AXIS == 1 ? (int64_t)job.step0 * C : (int64_t)job.step0 * rs;
    for (int p = ((int)blockIdx.x - job.block0) * 256 + (int)threadIdx.x; p < total; p += job.blocks * 256) {
        int o, j;
        if (AXIS == 1) {                        // horizontal: dst [other rows][n_out][C]
            j = p / n_out;
            o = p - j * n_out;
        } else {                                // vertical: dst [n_out][other cols][C]
            o = p / other;
            j = p - o * other;
        }
        const int first = bounds[2 * o], cnt = bounds[2 * o + 1];
        const int32_t *k = kk + (int64_t)o * job.ksize;
        const int64_t a0 = (int64_t)job.base0 + (int64_t)job.step0 * first;
        const int64_t jo = (int64_t)job.base1 + (int64_t)job.step1 * j;
        const uint8_t *q = src + (AXIS == 1 ? jo * rs + a0 * C : a0 * rs + jo * C);
        int ss[C];
#pragma unroll
        for (int c = 0; c < C; ++c) ss[c] = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) {
            const int w = k[t];
#pragma unroll
            for (int c = 0; c < C; ++c) ss[c] += (int)q[c] * w;
            q += tap_stride;
        }
        uint8_t *d = job.dst + (int64_t)p * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int v = ss[c] >> PRECISION_BITS;
            d[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
}

struct GatherBatch {
    gwd_gather_job j[GWD_GATHER_BATCH];
    int n;
};

__global__ __launch_bounds__(256) void gather2d_batch_kernel(const GatherBatch b, const int32_t *__restrict__ tables) {
    int ji = 0;
#pragma unroll 1
    for (int k = 1; k < b.n; ++k)
        if ((int)blockIdx.x >= b.j[k].block0) ji = k;
    const gwd_gather_job job = b.j[ji];
    const int32_t *__restrict__ ytab = tables + job.ytab_off;
    const int32_t *__restrict__ xtab = tables + job.xtab_off;
    const uint8_t *__restrict__ src = (const uint8_t *)job.src;
    uint8_t *__restrict__ dst = (uint8_t *)job.dst;
    const int ow = job.ow, eb = job.elem_bytes;
    const int total = job.oh * ow;                                            // < 2^31: checked on the host
    for (int p = ((int)blockIdx.x - job.block0) * 256 + (int)threadIdx.x; p < total; p += job.blocks * 256) {
        const int y = p / ow, x = p - y * ow;
        const uint8_t *s = src + (int64_t)ytab[y] * job.src_row_stride_bytes + (int64_t)xtab[x] * eb;
        uint8_t *d = dst + (int64_t)p * eb;
        if (eb == 4) {                          // 2- and 4-byte elements are aligned to their size (checked on the host)
            *(uint32_t *)d = *(const uint32_t *)s;
        } else if (eb == 2) {
            *(uint16_t *)d = *(const uint16_t *)s;
        } else {
            d[0] = s[0];
            if (eb == 3) {
                d[1] = s[1];
                d[2] = s[2];
            }
        }
    }
}

inline int job_blocks(int64_t pixels) {
    const int64_t nb = (pixels + 255) / 256;
    return (int)(nb > JOB_BLOCKS_MAX ? JOB_BLOCKS_MAX : nb);
}

}  // namespace

extern "C" int gwd_resample_u8_pass_batch(const gwd_resample_job *jobs, int32_t n, int32_t axis, int32_t C, const int32_t *tables,
                                          int64_t table_len, void *stream) {
    if (!jobs || n <= 0 || n > GWD_AUGMENT_BATCH || !tables || table_len <= 0 || (axis != 0 && axis != 1) || C <= 0) return -1;
    if (C > 4) return -4;
    ResampleBatch b;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        gwd_resample_job j = jobs[i];
        if (!j.src || !j.dst || j.ksize <= 0 || j.n_out <= 0 || j.other <= 0) return -1;
        if ((j.step0 != 1 && j.step0 != -1) || (j.step1 != 1 && j.step1 != -1)) return -1;
        if ((int64_t)j.n_out * j.other >= (1LL << 31)) return -7;
        if (j.bounds_off < 0 || j.kk_off < 0 || (int64_t)j.bounds_off + 2 * (int64_t)j.n_out > table_len ||
            (int64_t)j.kk_off + (int64_t)j.n_out * j.ksize > table_len)
            return -3;
        j.blocks = job_blocks((int64_t)j.n_out * j.other);
        j.block0 = total;
        total += j.blocks;
        b.j[i] = j;
    }
    b.n = n;
    hipStream_t s = (hipStream_t)stream;
#define GWD_RESAMPLE_BATCH_LAUNCH(CC)                                                                  \
    if (axis == 1) resample_u8_batch_kernel<CC, 1><<<total, 256, 0, s>>>(b, tables);                  \
    else resample_u8_batch_kernel<CC, 0><<<total, 256, 0, s>>>(b, tables)
    switch (C) {
        case 1: GWD_RESAMPLE_BATCH_LAUNCH(1); break;
        case 2: GWD_RESAMPLE_BATCH_LAUNCH(2); break;
        case 3: GWD_RESAMPLE_BATCH_LAUNCH(3); break;
        default: GWD_RESAMPLE_BATCH_LAUNCH(4); break;
    }
#undef GWD_RESAMPLE_BATCH_LAUNCH
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_gather2d_batch(const gwd_gather_job *jobs, int32_t n, const int32_t *tables, int64_t table_len, void *stream) {
    if (!jobs || n <= 0 || n > GWD_GATHER_BATCH || !tables || table_len <= 0) return -1;
    GatherBatch b;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        gwd_gather_job j = jobs[i];
        if (!j.src || !j.dst || j.oh <= 0 || j.ow <= 0) return -1;
        if (j.elem_bytes < 1 || j.elem_bytes > 4) return -4;
        if ((int64_t)j.oh * j.ow >= (1LL << 31)) return -7;
        if ((j.elem_bytes == 2 || j.elem_bytes == 4) &&
            (((uintptr_t)j.src | (uintptr_t)j.dst | (uintptr_t)j.src_row_stride_bytes) & (uintptr_t)(j.elem_bytes - 1)))
            return -1;
        if (j.ytab_off < 0 || j.xtab_off < 0 || (int64_t)j.ytab_off + j.oh > table_len || (int64_t)j.xtab_off + j.ow > table_len) return -3;
        j.blocks = job_blocks((int64_t)j.oh * j.ow);
        j.block0 = total;
        total += j.blocks;
        b.j[i] = j;
    }
    b.n = n;
    gather2d_batch_kernel<<<total, 256, 0, (hipStream_t)stream>>>(b, tables);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_resample_u8_pass(const uint8_t *src, uint8_t *dst, const int32_t *bounds, const int32_t *kk, int32_t ksize, int32_t axis,
                                    int32_t n_out, int32_t other, int32_t C, int64_t src_row_stride, int32_t base0, int32_t step0,
                                    int32_t base1, int32_t step1, void *stream) {
    if (!src || !dst || !bounds || !kk || ksize <= 0 || n_out <= 0 || other <= 0 || C <= 0 || (axis != 0 && axis != 1)) return -1;
    if ((step0 != 1 && step0 != -1) || (step1 != 1 && step1 != -1)) return -1;
    const int64_t total = (int64_t)n_out * other * C;
    resample_u8_kernel<<<flat_grid(total, 8192), 256, 0, (hipStream_t)stream>>>(src, dst, bounds, kk, ksize, axis, n_out, other, C, src_row_stride, base0,
                                                                          step0, base1, step1);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_gather2d(const void *src, void *dst, const int32_t *ytab, const int32_t *xtab, int32_t oh, int32_t ow,
                            int64_t src_row_stride_bytes, int32_t elem_bytes, void *stream) {
    if (!src || !dst || !ytab || !xtab || oh <= 0 || ow <= 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const int g = flat_grid((int64_t)oh * ow, 8192);
    const uint8_t *sp = (const uint8_t *)src;
    uint8_t *dp = (uint8_t *)dst;
    switch (elem_bytes) {
        case 1: gather2d_kernel<1><<<g, 256, 0, s>>>(sp, dp, ytab, xtab, oh, ow, src_row_stride_bytes); break;
        case 2: gather2d_kernel<2><<<g, 256, 0, s>>>(sp, dp, ytab, xtab, oh, ow, src_row_stride_bytes); break;
        case 3: gather2d_kernel<3><<<g, 256, 0, s>>>(sp, dp, ytab, xtab, oh, ow, src_row_stride_bytes); break;
        case 4: gather2d_kernel<4><<<g, 256, 0, s>>>(sp, dp, ytab, xtab, oh, ow, src_row_stride_bytes); break;
        default: return -4;
    }
    GWD_CHECK_LAUNCH();
    return 0;
}

// Inference post-processing on the device, behind the forward on the caller's stream (no allocation, no sync, no atomics):
//
// dense_post_*_kernel  the clamp of src/engine_glassrgbd.py:249-252, the millimetre form of the data set's depth PNGs
//                      (src/datasets/glassrgbd_norhint.py:273) and the argmax over the two segmentation logits, as ONE streaming
//                      pass over the full-resolution outputs; padding (outside an image's un-padded (h, w)) is written as
//                      depth 0 / millimetres 0 / label 255 (the ignore value of src/util/metrics.py).
// line_post_kernel     PostProcess_Line 'prediction' (src/models/glassrgbd.py:470-477) for two classes, plus the queries ordered by
//                      score (descending, equal scores by lower index) and the number of scores above a threshold.
#include "common.h"
#include "depthmm.h"          // to_mm: metres -> the PNGs' millimetres

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

constexpr int PX = 8;            // pixels per thread of the vector kernel: 16 B of bf16 in, 2 x 16 B of fp32 out, 16 B of uint16, 8 B of labels
constexpr int LINE_MAXQ = 1024;

__device__ __forceinline__ void load8(const float *p, float (&v)[8]) {
    const f32x4 a = *(const f32x4 *)p, b = *(const f32x4 *)(p + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = a[k], v[4 + k] = b[k];
}
__device__ __forceinline__ void load8(const __bf16 *p, float (&v)[8]) {
    const bf16x8 a = *(const bf16x8 *)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)a[k];
}

// engine_glassrgbd.py:249-252 in that order: a NaN fails both comparisons and is caught last; +inf is > max, -inf is < min
__device__ __forceinline__ float clamp_depth(float p, float dmin, float dmax) {
    if (p < dmin) p = dmin;
    if (p > dmax) p = dmax;
    if (p != p) p = dmin;
    return p;
}
// torch.argmax over (l0, l1): the first maximum wins, a NaN counts as the maximum
__device__ __forceinline__ int argmax2(float l0, float l1) { return (l1 > l0 || (l1 != l1 && l0 == l0)) ? 1 : 0; }

// SEG_MODE 1: logits interleaved per pixel (pixel stride 2, class stride 1: the model's pixel-major map);
//          2: planar (pixel stride 1, class stride seg_sc: NCHW).
// Needs W % 8 == 0 (a thread's 8 pixels lie in one row), 16-byte aligned bases and image strides that keep them so; the host
// wrapper checks and falls back to the scalar kernel.
template <typename TD, typename TS, int SEG_MODE>
__global__ __launch_bounds__(256) void dense_post_vec_kernel(const TD *__restrict__ depth, const TS *__restrict__ seg, int64_t seg_sb,
                                                             int64_t seg_sc, const int32_t *__restrict__ sizes,
                                                             float *__restrict__ depth_out, unsigned short *__restrict__ depth_mm,
                                                             unsigned char *__restrict__ label, uint32_t groups, uint32_t gpr,
                                                             uint32_t H, float dmin, float dmax) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= groups) return;
    const uint32_t row = g / gpr, x0 = (g - row * gpr) * PX;
    const uint32_t b = row / H, y = row - b * H;
    const uint32_t W = gpr * PX;
    const int32_t h = sizes ? sizes[2 * b] : (int32_t)H, w = sizes ? sizes[2 * b + 1] : (int32_t)W;
    const int64_t pix = (int64_t)y * W + x0, at = (int64_t)b * H * W + pix;
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
    u16x8 mm = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned int lab[2] = {0xffffffffu, 0xffffffffu};
    if ((int32_t)y < h && (int32_t)x0 < w) {            // a group wholly in the padding reads nothing
        float d[8], l0[8], l1[8];
        load8(depth + at, d);
        if constexpr (SEG_MODE == 1) {
            float a[8], c[8];
            const TS *p = seg + (int64_t)b * seg_sb + pix * 2;
            load8(p, a);
            load8(p + 8, c);
#pragma unroll
            for (int k = 0; k < 4; ++k) l0[k] = a[2 * k], l1[k] = a[2 * k + 1], l0[4 + k] = c[2 * k], l1[4 + k] = c[2 * k + 1];
        } else {
            const TS *p = seg + (int64_t)b * seg_sb + pix;
            load8(p, l0);
            load8(p + seg_sc, l1);
        }
        lab[0] = lab[1] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool in = (int32_t)(x0 + k) < w;
            const float v = in ? clamp_depth(d[k], dmin, dmax) : 0.0f;
            if (k < 4) d0[k] = v; else d1[k - 4] = v;
            mm[k] = in ? to_mm(v) : (unsigned short)0;
            lab[k >> 2] |= (in ? (unsigned int)argmax2(l0[k], l1[k]) : 255u) << (8 * (k & 3));
        }
    }
    *(f32x4 *)(depth_out + at) = d0;
    *(f32x4 *)(depth_out + at + 4) = d1;
    if (depth_mm) *(u16x8 *)(depth_mm + at) = mm;
    const u32x2 lv = {lab[0], lab[1]};
    *(u32x2 *)(label + at) = lv;
}

// any shape, any strides, any alignment: one pixel per thread and step
template <typename TD, typename TS>
__global__ __launch_bounds__(256) void dense_post_scalar_kernel(const TD *__restrict__ depth, const TS *__restrict__ seg, int64_t seg_sb,
                                                                int64_t seg_sp, int64_t seg_sc, const int32_t *__restrict__ sizes,
                                                                float *__restrict__ depth_out, unsigned short *__restrict__ depth_mm,
                                                                unsigned char *__restrict__ label, int64_t total, int32_t H, int32_t W,
                                                                float dmin, float dmax) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / HW, pix = i - b * HW;
        const int32_t y = (int32_t)(pix / W), x = (int32_t)(pix - (int64_t)y * W);
        const int32_t h = sizes ? sizes[2 * b] : H, w = sizes ? sizes[2 * b + 1] : W;
        float v = 0.0f;
        unsigned short mm = 0;
        unsigned char lb = 255;
        if (y < h && x < w) {
            v = clamp_depth(to_f32(depth[i]), dmin, dmax);
            mm = to_mm(v);
            const TS *p = seg + b * seg_sb + pix * seg_sp;
            lb = (unsigned char)argmax2(to_f32(p[0]), to_f32(p[seg_sc]));
        }
        depth_out[i] = v;
        if (depth_mm) depth_mm[i] = mm;
        label[i] = lb;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dense_post_resized_kernel: the pass above with a bilinear resize (F.interpolate(mode="bilinear", align_corners=False) over the
// un-padded h x w region) to a per-image output size, and an optional mirrored twin averaged in.  A workgroup owns (a piece of) ONE
// output row, so the two source rows and the row weight are uniform over it: it first blends the two source rows column by column
// (sanitised depth, both logits; the twin read mirrored inside w) into LDS, then every thread blends two LDS columns per pixel.
// Source widths beyond RS_STAGE_COLS skip the LDS and read their taps from memory (STAGE = false), with the same arithmetic.
constexpr int RS_MAX_DIM = 16384;      // (2 * d + 1) * in stays below 2^30
constexpr int RS_STAGE_COLS = 4096;    // 3 fp32 rows of that many columns: 48 KiB of LDS

// a tap with weight zero is not read into the result: the identity resize is the plain pass bit for bit, whatever the neighbour holds
__device__ __forceinline__ float lerp_rs(float a, float b, float l) { return l == 0.0f ? a : (1.0f - l) * a + l * b; }

template <typename TD, typename TS>
struct ResizedSource {
    const TD *d0, *d1, *e0, *e1;       // depth rows y0, y1 of the image and of its twin
    const TS *s0, *s1, *t0, *t1;       // logit rows likewise
    int64_t sp, sc;
    int32_t w;
    bool twin;
    float ly, dmin, dmax;

    // source column x of the output row: the two rows blended by ly
    __device__ __forceinline__ void column(int32_t x, float &s, float &l0, float &l1) const {
        float a0 = clamp_depth(to_f32(d0[x]), dmin, dmax), a1 = clamp_depth(to_f32(d1[x]), dmin, dmax);
        float p0 = to_f32(s0[x * sp]), p1 = to_f32(s0[x * sp + sc]), q0 = to_f32(s1[x * sp]), q1 = to_f32(s1[x * sp + sc]);
        if (twin) {
            const int64_t m = w - 1 - x;
            a0 = 0.5f * (a0 + clamp_depth(to_f32(e0[m]), dmin, dmax));
            a1 = 0.5f * (a1 + clamp_depth(to_f32(e1[m]), dmin, dmax));
            p0 += to_f32(t0[m * sp]), p1 += to_f32(t0[m * sp + sc]), q0 += to_f32(t1[m * sp]), q1 += to_f32(t1[m * sp + sc]);
        }
        s = lerp_rs(a0, a1, ly), l0 = lerp_rs(p0, q0, ly), l1 = lerp_rs(p1, q1, ly);
    }
};

// 8 consecutive pixels of a logit row from 16-byte loads: seg_mode 1 interleaved, 2 planar
template <typename TS>
__device__ __forceinline__ void logits8(const TS *row, int64_t c, int seg_mode, int64_t sc, float (&l0)[8], float (&l1)[8]) {
    if (seg_mode == 1) {
        float a[8], b[8];
        load8(row + c * 2, a);
        load8(row + c * 2 + 8, b);
#pragma unroll
        for (int k = 0; k < 4; ++k) l0[k] = a[2 * k], l1[k] = a[2 * k + 1], l0[4 + k] = b[2 * k], l1[4 + k] = b[2 * k + 1];
    } else {
        load8(row + c, l0);
        load8(row + c + sc, l1);
    }
}

// PXN 8: Fw % 8 == 0 and aligned outputs, a thread stores 8 pixels of one row as 16 + 16 + 16 + 8 bytes; PXN 1: any output.
// seg_mode != 0: W % 8 == 0 and aligned sources, the staging reads 16 bytes at a time (host-checked).
// LDS: 3 * lds_cols floats when STAGE (lds_cols = W rounded up to 8).
template <typename TD, typename TS, int PXN, bool STAGE>
__global__ __launch_bounds__(256) void dense_post_resized_kernel(const TD *__restrict__ depth, const TS *__restrict__ seg, int64_t seg_sb,
                                                                 int64_t seg_sp, int64_t seg_sc, int seg_mode,
                                                                 const int32_t *__restrict__ sizes, const int32_t *__restrict__ frame_sizes,
                                                                 int32_t twin, float *__restrict__ depth_out,
                                                                 unsigned short *__restrict__ depth_mm, unsigned char *__restrict__ label,
                                                                 uint32_t chunks, int32_t H, int32_t W, int32_t Fh, int32_t Fw,
                                                                 int32_t lds_cols, float dmin, float dmax) {
    extern __shared__ float rs_lds[];
    const uint32_t rowg = blockIdx.x / chunks, chunk = blockIdx.x - rowg * chunks;
    const int32_t b = (int32_t)(rowg / (uint32_t)Fh), dy = (int32_t)(rowg - (uint32_t)b * (uint32_t)Fh);
    // device data: clamped to the allocated extents, so that no value of it reaches outside the buffers
    const int32_t h = sizes ? min(max(sizes[2 * b], 1), H) : H, w = sizes ? min(max(sizes[2 * b + 1], 1), W) : W;
    const int32_t fh = min(max(frame_sizes[2 * b], 0), Fh), fw = min(max(frame_sizes[2 * b + 1], 0), Fw);
    const bool row_in = dy < fh && fw > 0;
    float *sd = rs_lds, *sl0 = rs_lds + lds_cols, *sl1 = rs_lds + 2 * lds_cols;
    ResizedSource<TD, TS> src;
    if (row_in) {
        const uint32_t ny = (uint32_t)max((2 * dy + 1) * h - fh, 0), dy2 = 2u * (uint32_t)fh;
        const uint32_t y0 = ny / dy2, y1 = min(y0 + 1u, (uint32_t)h - 1u);
        const int64_t b2 = b + twin, rp = (int64_t)W * seg_sp;
        src.d0 = depth + ((int64_t)b * H + y0) * W, src.d1 = depth + ((int64_t)b * H + y1) * W;
        src.e0 = depth + (b2 * H + y0) * W, src.e1 = depth + (b2 * H + y1) * W;
        src.s0 = seg + b * seg_sb + y0 * rp, src.s1 = seg + b * seg_sb + y1 * rp;
        src.t0 = seg + b2 * seg_sb + y0 * rp, src.t1 = seg + b2 * seg_sb + y1 * rp;
        src.sp = seg_sp, src.sc = seg_sc, src.w = w, src.twin = twin != 0, src.dmin = dmin, src.dmax = dmax;
        src.ly = __fdiv_rn((float)(ny - y0 * dy2), (float)dy2);
        if constexpr (STAGE) {
            if (seg_mode != 0) {
                const bool twin8 = src.twin && (w & 7) == 0;           // the mirrored groups are aligned groups too
                for (int32_t c = threadIdx.x * 8; c < w; c += blockDim.x * 8) {      // c + 8 <= W: columns >= w are staged, never read
                    float a0[8], a1[8], p0[8], p1[8], q0[8], q1[8];
                    load8(src.d0 + c, a0);
                    load8(src.d1 + c, a1);
                    logits8(src.s0, c, seg_mode, seg_sc, p0, p1);
                    logits8(src.s1, c, seg_mode, seg_sc, q0, q1);
#pragma unroll
                    for (int k = 0; k < 8; ++k) a0[k] = clamp_depth(a0[k], dmin, dmax), a1[k] = clamp_depth(a1[k], dmin, dmax);
                    if (twin8) {
                        const int32_t m = w - 8 - c;                   // columns m .. m + 7 mirror c + 7 .. c
                        float e0[8], e1[8], t00[8], t01[8], t10[8], t11[8];
                        load8(src.e0 + m, e0);
                        load8(src.e1 + m, e1);
                        logits8(src.t0, m, seg_mode, seg_sc, t00, t01);
                        logits8(src.t1, m, seg_mode, seg_sc, t10, t11);
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            a0[k] = 0.5f * (a0[k] + clamp_depth(e0[7 - k], dmin, dmax));
                            a1[k] = 0.5f * (a1[k] + clamp_depth(e1[7 - k], dmin, dmax));
                            p0[k] += t00[7 - k], p1[k] += t01[7 - k], q0[k] += t10[7 - k], q1[k] += t11[7 - k];
                        }
                    } else if (src.twin) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const int64_t m = w - 1 - (c + k);
                            if (m >= 0) {
                                a0[k] = 0.5f * (a0[k] + clamp_depth(to_f32(src.e0[m]), dmin, dmax));
                                a1[k] = 0.5f * (a1[k] + clamp_depth(to_f32(src.e1[m]), dmin, dmax));
                                p0[k] += to_f32(src.t0[m * seg_sp]), p1[k] += to_f32(src.t0[m * seg_sp + seg_sc]);
                                q0[k] += to_f32(src.t1[m * seg_sp]), q1[k] += to_f32(src.t1[m * seg_sp + seg_sc]);
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        sd[c + k] = lerp_rs(a0[k], a1[k], src.ly);
                        sl0[c + k] = lerp_rs(p0[k], q0[k], src.ly);
                        sl1[c + k] = lerp_rs(p1[k], q1[k], src.ly);
                    }
                }
            } else {
                for (int32_t c = threadIdx.x; c < w; c += blockDim.x) src.column(c, sd[c], sl0[c], sl1[c]);
            }
        }
    }
    if constexpr (STAGE) __syncthreads();
    const uint32_t x0 = (chunk * blockDim.x + threadIdx.x) * PXN;
    if (x0 >= (uint32_t)Fw) return;
    float dv[PXN];
    unsigned short mv[PXN];
    unsigned int lv[PXN];
#pragma unroll
    for (int k = 0; k < PXN; ++k) dv[k] = 0.0f, mv[k] = 0, lv[k] = 255u;
    if (row_in && x0 < (uint32_t)fw) {
        // n = max((2 x + 1) w - fw, 0) = q * 2 fw + r, carried from pixel to pixel without a division: q = -1 stands for n < 0
        const uint32_t dx2 = 2u * (uint32_t)fw, step_q = (2u * (uint32_t)w) / dx2, step_r = 2u * (uint32_t)w - step_q * dx2;
        const int32_t m0 = (int32_t)((2u * x0 + 1u) * (uint32_t)w) - fw;
        int32_t q = m0 < 0 ? -1 : (int32_t)((uint32_t)m0 / dx2);
        uint32_t r = m0 < 0 ? (uint32_t)(m0 + (int32_t)dx2) : (uint32_t)m0 - (uint32_t)q * dx2;
        const float fdx2 = (float)dx2;
#pragma unroll
        for (int k = 0; k < PXN; ++k) {
            if (x0 + k < (uint32_t)fw) {
                const int32_t i0 = min(max(q, 0), w - 1), i1 = min(i0 + 1, w - 1);
                const float lx = q < 0 ? 0.0f : __fdiv_rn((float)r, fdx2);
                float sa, la0, la1, sb, lb0, lb1;
                if constexpr (STAGE) {
                    sa = sd[i0], la0 = sl0[i0], la1 = sl1[i0], sb = sd[i1], lb0 = sl0[i1], lb1 = sl1[i1];
                } else {
                    src.column(i0, sa, la0, la1);
                    src.column(i1, sb, lb0, lb1);
                }
                dv[k] = fminf(fmaxf(lerp_rs(sa, sb, lx), dmin), dmax);     // a blend of equal samples may round one ulp past them
                mv[k] = to_mm(dv[k]);
                lv[k] = (unsigned int)argmax2(lerp_rs(la0, lb0, lx), lerp_rs(la1, lb1, lx));
            }
            r += step_r;
            const bool carry = r >= dx2;
            r -= carry ? dx2 : 0u;
            q += (int32_t)step_q + (carry ? 1 : 0);
        }
    }
    const int64_t at = ((int64_t)b * Fh + dy) * Fw + x0;
    if constexpr (PXN == 8) {
        const f32x4 d0 = {dv[0], dv[1], dv[2], dv[3]}, d1 = {dv[4], dv[5], dv[6], dv[7]};
        *(f32x4 *)(depth_out + at) = d0;
        *(f32x4 *)(depth_out + at + 4) = d1;
        if (depth_mm) {
            const u16x8 mm = {mv[0], mv[1], mv[2], mv[3], mv[4], mv[5], mv[6], mv[7]};
            *(u16x8 *)(depth_mm + at) = mm;
        }
        const u32x2 lab = {lv[0] | lv[1] << 8 | lv[2] << 16 | lv[3] << 24, lv[4] | lv[5] << 8 | lv[6] << 16 | lv[7] << 24};
        *(u32x2 *)(label + at) = lab;
    } else {
        depth_out[at] = dv[0];
        if (depth_mm) depth_mm[at] = mv[0];
        label[at] = (unsigned char)lv[0];
    }
}

// One workgroup per image.  The order comes from ranks: query i goes to the place given by the number of queries that beat it
// (higher key, or equal key and lower index) - a total order, so the ranks are a permutation of 0..Q-1 whatever the scores hold.
// Every thread reads the same key of the table at a time: LDS broadcasts, Q * ceil(Q / 256) reads per thread.
__global__ __launch_bounds__(256) void line_post_kernel(const float *__restrict__ logits, const float *__restrict__ lines,
                                                        const int32_t *__restrict__ sizes, float *__restrict__ scores,
                                                        float *__restrict__ lines_px, int32_t *__restrict__ order,
                                                        int32_t *__restrict__ count, int32_t Q, int32_t ld, float thresh) {
    __shared__ uint32_t key[LINE_MAXQ];
    __shared__ int cnt[4];
    const int b = blockIdx.x;
    const float h = (float)sizes[2 * b], w = (float)sizes[2 * b + 1];
    int above = 0;
    for (int q = threadIdx.x; q < Q; q += 256) {
        const int64_t at = (int64_t)b * Q + q;
        const float l0 = logits[at * 2], l1 = logits[at * 2 + 1];
        const float m = fmaxf(l0, l1), e0 = expf(l0 - m), e1 = expf(l1 - m);
        const float s = (l0 != l0 || l1 != l1) ? __builtin_nanf("") : __fdiv_rn(e0, e0 + e1);     // fmaxf drops a NaN, softmax keeps it
        scores[at] = s;
        key[q] = score_key(s);
        above += s > thresh ? 1 : 0;
        const float *src = lines + at * ld;
        const f32x4 px = {src[0] * w, src[1] * h, src[2] * w, src[3] * h};
        *(f32x4 *)(lines_px + at * 4) = px;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = above;
    __syncthreads();
    if (threadIdx.x == 0) count[b] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    for (int q = threadIdx.x; q < Q; q += 256) {
        const uint32_t mine = key[q];
        int rank = 0;
        for (int j = 0; j < Q; ++j) {
            const uint32_t k = key[j];
            rank += (k > mine || (k == mine && j < q)) ? 1 : 0;
        }
        order[(int64_t)b * Q + rank] = q;
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gwd_dense_postprocess(const void *depth, const void *seg_logits, int64_t seg_sb, int64_t seg_sp, int64_t seg_sc,
                                     const int32_t *sizes, float *depth_out, uint16_t *depth_mm, uint8_t *label, int32_t B, int32_t H,
                                     int32_t W, float min_depth, float max_depth, int32_t depth_dtype, int32_t seg_dtype,
                                     void *stream) {
    if (B <= 0 || H <= 0 || W <= 0 || !depth || !seg_logits || !depth_out || !label) return -1;
    if ((depth_dtype != GWD_F32 && depth_dtype != GWD_BF16) || (seg_dtype != GWD_F32 && seg_dtype != GWD_BF16)) return -2;
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
    hipStream_t s = (hipStream_t)stream;
    const int seg_mode = (seg_sp == 2 && seg_sc == 1) ? 1 : ((seg_sp == 1 && seg_sc % 8 == 0) ? 2 : 0);
    const bool vec = W % PX == 0 && seg_mode != 0 && seg_sb % 8 == 0 && total / PX < (int64_t)1 << 31 && aligned16(depth) &&
                     aligned16(seg_logits) && aligned16(depth_out) && aligned16(depth_mm) && ((uintptr_t)label & 7) == 0;
    if (vec) {
        const uint32_t groups = (uint32_t)(total / PX), gpr = (uint32_t)(W / PX);
        const uint32_t nb = (groups + 255u) / 256u;
#define DENSE_VEC(TD, TS)                                                                                                              \
    do {                                                                                                                               \
        if (seg_mode == 1)                                                                                                             \
            dense_post_vec_kernel<TD, TS, 1><<<nb, 256, 0, s>>>((const TD *)depth, (const TS *)seg_logits, seg_sb, seg_sc, sizes,       \
                                                                depth_out, depth_mm, label, groups, gpr, (uint32_t)H, min_depth, max_depth); \
        else                                                                                                                           \
            dense_post_vec_kernel<TD, TS, 2><<<nb, 256, 0, s>>>((const TD *)depth, (const TS *)seg_logits, seg_sb, seg_sc, sizes,       \
                                                                depth_out, depth_mm, label, groups, gpr, (uint32_t)H, min_depth, max_depth); \
    } while (0)
        if (depth_dtype == GWD_F32 && seg_dtype == GWD_F32) DENSE_VEC(float, float);
        else if (depth_dtype == GWD_F32) DENSE_VEC(float, __bf16);
        else if (seg_dtype == GWD_F32) DENSE_VEC(__bf16, float);
        else DENSE_VEC(__bf16, __bf16);
#undef DENSE_VEC
    } else {
        int64_t nb64 = (total + 255) / 256;
        const int nb = (int)(nb64 > 65536 ? 65536 : nb64);
#define DENSE_SCALAR(TD, TS)                                                                                                        \
    dense_post_scalar_kernel<TD, TS><<<nb, 256, 0, s>>>((const TD *)depth, (const TS *)seg_logits, seg_sb, seg_sp, seg_sc, sizes,    \
                                                        depth_out, depth_mm, label, total, H, W, min_depth, max_depth)
        if (depth_dtype == GWD_F32 && seg_dtype == GWD_F32) DENSE_SCALAR(float, float);
        else if (depth_dtype == GWD_F32) DENSE_SCALAR(float, __bf16);
        else if (seg_dtype == GWD_F32) DENSE_SCALAR(__bf16, float);
        else DENSE_SCALAR(__bf16, __bf16);
#undef DENSE_SCALAR
    }
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_dense_postprocess_resized(const void *depth, const void *seg_logits, int64_t seg_sb, int64_t seg_sp, int64_t seg_sc,
                                             const int32_t *sizes, const int32_t *frame_sizes, int32_t twin, float *depth_out,
                                             uint16_t *depth_mm, uint8_t *label, int32_t B, int32_t H, int32_t W, int32_t Fh, int32_t Fw,
                                             float min_depth, float max_depth, int32_t depth_dtype, int32_t seg_dtype, void *stream) {
    if (B <= 0 || H <= 0 || W <= 0 || Fh <= 0 || Fw <= 0 || twin < 0 || !depth || !seg_logits || !frame_sizes || !depth_out || !label)
        return -1;
    if (H > RS_MAX_DIM || W > RS_MAX_DIM || Fh > RS_MAX_DIM || Fw > RS_MAX_DIM) return -1;
    if ((depth_dtype != GWD_F32 && depth_dtype != GWD_BF16) || (seg_dtype != GWD_F32 && seg_dtype != GWD_BF16)) return -2;
    hipStream_t s = (hipStream_t)stream;
    int seg_mode = (seg_sp == 2 && seg_sc == 1) ? 1 : ((seg_sp == 1 && seg_sc % 8 == 0) ? 2 : 0);
    if (W % 8 != 0 || seg_sb % 8 != 0 || !aligned16(depth) || !aligned16(seg_logits)) seg_mode = 0;
    const bool vec = Fw % PX == 0 && aligned16(depth_out) && aligned16(depth_mm) && ((uintptr_t)label & 7) == 0;
    const bool stage = W <= RS_STAGE_COLS;
    const uint32_t per_row = (uint32_t)(vec ? Fw / PX : Fw);                 // threads that an output row takes
    const uint32_t nt = per_row >= 256u ? 256u : (per_row + 63u) / 64u * 64u, chunks = (per_row + nt - 1u) / nt;
    const int64_t nb64 = (int64_t)B * Fh * chunks;
    if (nb64 >= (int64_t)1 << 31) return -1;
    const uint32_t nb = (uint32_t)nb64;
    const int32_t lds_cols = (W + 7) / 8 * 8;
    const size_t lds = stage ? (size_t)3 * lds_cols * sizeof(float) : 0;
#define DENSE_RS(TD, TS, PXN, STAGE)                                                                                                   \
    dense_post_resized_kernel<TD, TS, PXN, STAGE><<<nb, nt, lds, s>>>((const TD *)depth, (const TS *)seg_logits, seg_sb, seg_sp,        \
                                                                      seg_sc, seg_mode, sizes, frame_sizes, twin, depth_out, depth_mm, \
                                                                      label, chunks, H, W, Fh, Fw, lds_cols, min_depth, max_depth)
#define DENSE_RS_SHAPE(TD, TS)                                                                                                         \
    do {                                                                                                                               \
        if (vec && stage) DENSE_RS(TD, TS, 8, true);                                                                                   \
        else if (vec) DENSE_RS(TD, TS, 8, false);                                                                                      \
        else if (stage) DENSE_RS(TD, TS, 1, true);                                                                                     \
        else DENSE_RS(TD, TS, 1, false);                                                                                               \
    } while (0)
    if (depth_dtype == GWD_F32 && seg_dtype == GWD_F32) DENSE_RS_SHAPE(float, float);
    else if (depth_dtype == GWD_F32) DENSE_RS_SHAPE(float, __bf16);
    else if (seg_dtype == GWD_F32) DENSE_RS_SHAPE(__bf16, float);
    else DENSE_RS_SHAPE(__bf16, __bf16);
#undef DENSE_RS_SHAPE
#undef DENSE_RS
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_line_postprocess(const float *logits, const float *lines, const int32_t *sizes, float *scores, float *lines_px,
                                    int32_t *order, int32_t *count, int32_t B, int32_t Q, int32_t ld, float thresh, void *stream) {
    if (B <= 0 || Q <= 0 || !logits || !lines || !sizes || !scores || !lines_px || !order || !count) return -1;
    if (ld != 4 && ld != 6) return -1;
    if (Q > LINE_MAXQ) return -2;
    if (!aligned16(lines_px)) return -1;
    line_post_kernel<<<B, 256, 0, (hipStream_t)stream>>>(logits, lines, sizes, scores, lines_px, order, count, Q, ld, thresh);
    GWD_CHECK_LAUNCH();
    return 0;
}

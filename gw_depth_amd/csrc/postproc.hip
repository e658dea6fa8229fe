// Inference post-processing on the device, behind the forward on the caller's stream (no allocation, no sync, no atomics):
//
// dense_post_*_kernel  the clamp of src/engine_glassrgbd.py:249-252, the millimetre form of the data set's depth PNGs
//                      (src/datasets/glassrgbd_norhint.py:273) and the argmax over the two segmentation logits, as ONE streaming
//                      pass over the full-resolution outputs; padding (outside an image's un-padded (h, w)) is written as
//                      depth 0 / millimetres 0 / label 255 (the ignore value of src/util/metrics.py).
// line_post_kernel     PostProcess_Line 'prediction' (src/models/glassrgbd.py:470-477) for two classes, plus the queries ordered by
//                      score (descending, equal scores by lower index) and the number of scores above a threshold.
#include "common.h"

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
// rint(metres * 1000) as the PNGs hold it, saturated to the uint16 range
__device__ __forceinline__ unsigned short to_mm(float d) {
    const float mm = rintf(d * 1000.0f);
    return (unsigned short)fminf(fmaxf(mm, 0.0f), 65535.0f);
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

// ascending order of the keys = ascending order of the floats, a NaN above everything (torch.sort's rule)
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0xffffffffu;
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
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

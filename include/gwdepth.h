/* gwdepth.h — C ABI of libgwdepth_hip.so: hand-written gfx950 (MI355X) kernels for the GW-Depth
 * train step.
 *
 * The reference (ViktorLiang/GW-Depth) has no FFI/plugin boundary: it is 100 % PyTorch and every
 * device operation is an ATen call.  Each entry point below therefore replaces an
 * ATen operator sequence at the cited reference call sites; the host side (the gw_depth_amd Python package) binds
 * them with ctypes and wraps them in torch.autograd.Function objects.
 *
 * Conventions:
 *   - plain C, no torch types; raw device pointers, explicit sizes, dtype enum, caller's hipStream_t
 *     passed as void*;
 *   - return 0 on success, negative = invalid argument / unsupported shape, positive = hipError_t;
 *   - never allocate or free caller memory, never synchronise the device, no mutable global state;
 *   - activation tensors are NHWC ("pixel-major": [B][H][W][C], a Linear input is [rows][C]);
 *   - convolution / linear weights are [Cout][KH][KW][Cin] (a Linear weight is [out][in] as in torch).
 */
#ifndef GWDEPTH_H
#define GWDEPTH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GWD_VERSION 10

enum { GWD_F32 = 0, GWD_BF16 = 1 };
enum { GWD_ACT_NONE = 0, GWD_ACT_RELU = 1, GWD_ACT_GELU = 2, GWD_ACT_ELU = 3, GWD_ACT_SIGMOID = 4 };
/* how output pixel (oh,ow) and tap (kh,kw) map to an input pixel */
enum {
    GWD_GATHER_CONV = 0,      /* ih = oh*stride - pad + kh                                     */
    GWD_GATHER_TRANSPOSED = 1,/* ih = (oh + pad - kh)/stride when divisible (data gradient)    */
    GWD_GATHER_UPSAMPLED = 2  /* stride 1 over a nearest-upsampled (Hv,Wv) view of the input   */
};

typedef struct {
    const void *x;        /* [B][Hi][Wi][Cin]                                                   */
    const void *w;        /* [Cout][KH][KW][Cin]                                                */
    void *y;              /* [B][Ho][Wo][Cout]                                                  */
    void *z;              /* optional copy of the value BEFORE the activation (for GELU bwd)    */
    const float *scale;   /* optional per-Cout multiplier (FrozenBN scale)                      */
    const float *shift;   /* optional per-Cout addend (bias / FrozenBN shift)                   */
    const void *residual; /* optional [B][Ho][Wo][Cout] added before the activation             */
    const void *zero_page;/* optional: >= 64 zero bytes of device memory.  Enables the LDS-DMA     */
                          /* pipeline (out-of-image taps are fetched from it instead of branching) */
    const void *mult;     /* optional [B][Ho][Wo][Cout] element-wise multiplier applied AFTER the    */
                          /* activation (dropout keep-mask / (1-p)); with it, `residual` is added    */
                          /* after the multiply instead of before the activation:                    */
                          /*   y = act_scale * act(conv + shift) * mult + residual                   */
                          /* (x + dropout(sublayer(x)) of src/models/transformer.py:149-162,212-233)  */
    const void *gate;     /* optional [B][Ho][Wo][Cout], with gate_act: the LAST step of the epilogue multiplies the   */
                          /* result by act'(.) of an activation whose OUTPUT is `gate` (ReLU: gate > 0, ELU with       */
                          /* alpha 1: gate > 0 ? 1 : gate + 1).  For a data-gradient launch this is the backward of    */
                          /* the activation that produced the layer's input (gate = that input, which the layer keeps  */
                          /* for its weight gradient anyway): the producer then skips its own activation-backward pass */
    int32_t B, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
    int32_t gather;       /* GWD_GATHER_*                                                       */
    int32_t Hv, Wv;       /* virtual input size for GWD_GATHER_UPSAMPLED                        */
    int32_t act;          /* GWD_ACT_*                                                          */
    float act_scale;      /* y = act_scale * act(v)  (max_depth * sigmoid)                      */
    int32_t dtype;        /* GWD_F32 / GWD_BF16 for x, w, y, z, residual, mult, gate            */
    int32_t gate_act;     /* GWD_ACT_RELU or GWD_ACT_ELU when gate != NULL, else ignored         */
    /* ConvLn mode (src/models/points/points_sample.py:12-25: conv -> LayerNorm over channels [-> GELU]), when ln_mean != NULL:   */
    /*   y = act(LN(conv) * scale + shift) + residual,  LN over the first ln_C of the Cout channels of a row (eps 1e-5; channels   */
    /*   ln_C .. Cout-1 are zero padding and come out as zeros; scale / shift = gamma / beta with ln_C entries, both required;     */
    /*   act NONE or GELU; the residual is added AFTER the activation, as gwd_layernorm_forward adds it).  z (optional) receives   */
    /*   the convolution itself, ln_mean / ln_rstd [B*Ho*Wo] the row statistics - exactly what gwd_layernorm_backward takes.      */
    /*   gwd_conv_forward returns -4 when it has no fused kernel for the shape (bf16, LDS-DMA route, a whole row inside one tile:  */
    /*   Cout <= 64 or Cout == 160); the caller then runs the convolution and gwd_layernorm_forward separately.                  */
    float *ln_mean;
    float *ln_rstd;
    int32_t ln_C;
    int32_t reserved;
    /* gwd_conv_wgrad / gwd_conv_wgrad_batch only (ignored elsewhere), may be NULL: dbias[Cout] fp32, ACCUMULATED (atomics, caller       */
    /* zeroes): dbias[n] += sum over the output pixels of y[pixel][n] - the bias gradient of the layer, from the dY tiles the weight  */
    /* gradient stages anyway instead of a gwd_colsum pass over the same map.  Only the LDS-DMA weight-gradient kernels do it: ask    */
    /* gwd_conv_wgrad_takes_bias first; a descriptor it answers 0 for is refused with -4 (nothing launched, never silently dropped).  */
    float *dbias;
} gwd_conv_desc;

int gwd_version(void);
const char *gwd_arch(void);

/* Scratch sizes.  The library never allocates: the two entry points that need scratch take a caller-provided buffer,
 * and this tells the caller how many BYTES it must hold (fully overwritten by the call, no initialisation needed).
 *   GWD_WS_INORM_GELU      dims = {B, S, C}        -> `part` of gwd_inorm_gelu_forward / _backward
 *   GWD_WS_RESAMPLE_BWD    dims = {B, Ho, Ws, C}   -> `tmp`  of gwd_resample_backward_sep
 *   GWD_WS_EVAL            dims = {B, H*W}         -> `workspace` of gwd_eval_accumulate
 *   GWD_WS_PLANE           dims = {P, H*W}         -> `workspace` of gwd_plane_loss_forward
 *   GWD_WS_HEALTH          dims = {n_chunks}       -> `partial` of gwd_segment_stats
 *   GWD_WS_REGIONS         dims = {B, Fh, Fw, max_candidates} -> `workspace` of gwd_glass_regions / gwd_region_planes
 *   GWD_WS_FUSION          dims = {B, Fh, Fw}      -> `workspace` of gwd_fusion_ring / gwd_fusion_planes
 *   GWD_WS_CLOUD           dims = {B, Fh, Fw, stride} -> `workspace` of gwd_point_cloud
 *   GWD_WS_SCENE           dims = {rows, max_voxels} -> `workspace` of gwd_scene_integrate (a cloud of `rows` rows) / gwd_scene_extract
 *   GWD_WS_VIEW            dims = {V, Fh, Fw}      -> `workspace` of gwd_cloud_view (the z-buffer)
 * Returns -1 for an unknown op or a wrong dimension count.                                                     */
enum { GWD_WS_INORM_GELU = 0, GWD_WS_RESAMPLE_BWD = 1, GWD_WS_EVAL = 2, GWD_WS_PLANE = 3, GWD_WS_HEALTH = 4, GWD_WS_REGIONS = 5,
       GWD_WS_FUSION = 6, GWD_WS_CLOUD = 7, GWD_WS_SCENE = 8, GWD_WS_VIEW = 9 };
int64_t gwd_query_workspace(int32_t op, const int64_t *dims, int32_t ndims);

/* Implicit-GEMM convolution on MFMA with fused epilogue y = act(scale*conv(x,w) + shift + residual).
 * Also the Linear layer (KH=KW=1, Hi=Wi=1, B=rows) and, with GWD_GATHER_TRANSPOSED and
 * the transposed weights of gwd_weight_prep, the data gradient.
 * Replaces: torchvision Bottleneck conv+FrozenBN+ReLU (src/models/backbone.py:45-55,90-92), ConvLn /
 * ConvA / upconv convolutions (src/models/points/points_sample.py:15-22,
 * src/models/multiscale_transformerr.py:110-116, src/models/dense_upsample.py:82-90,126-146),
 * every nn.Linear on the path (src/models/transformer.py:133-136,
 * src/models/multiscale_transformerr.py:62-64,249-251,425-429,445-449).                          */
int gwd_conv_forward(const gwd_conv_desc *d, void *stream);

/* Weight gradient dw[Cout][KH][KW][Cin] (fp32, ACCUMULATED into dw with atomics; caller zeroes it):
 * d->x = layer input, d->y = gradient w.r.t. the layer output (already multiplied by act'), gather
 * as in the forward.  d->scale (may be NULL): per-Cout multiplier of the result, dw[n] += scale[n] * (...) - the
 * layer computed with w * scale (folded FrozenBatchNorm, src/models/backbone.py:45-55), so this IS the gradient of
 * the unscaled parameter.  Replaces aten::convolution_backward (weight) / addmm weight grads.      */
int gwd_conv_wgrad(const gwd_conv_desc *d, float *dw, void *stream);
/* n independent gwd_conv_wgrad calls handed over together (descs[i] -> dws[i], each accumulated as gwd_conv_wgrad does;
 * two jobs may name the same dw).  Results are those of n single calls; the library is free to run jobs of one
 * kernel shape as ONE launch - the weight gradients of the ~230 Linear / 1x1 layers of a train step are 10-60 us
 * launches of 16-400 workgroups that cannot overlap inside one stream.  Nothing in descs / dws must outlive the call. */
int gwd_conv_wgrad_batch(const gwd_conv_desc *descs, float *const *dws, int32_t n, void *stream);
/* 1 if the kernel gwd_conv_wgrad (batched != 0: gwd_conv_wgrad_batch) selects for this descriptor accumulates d->dbias, else 0: the
 * LDS-DMA family only (bf16, zero page, channel counts in whole 16-byte vectors), without d->scale (a bias under a folded FrozenBN
 * does not exist on this path, and the per-row multiplier must not reach the bias sum).  The tile-conv layers (3x3 / stride 1 over
 * 32- / 64-channel maps of >= 131072 pixels) are declined as a family, whichever kernel takes the member today.  Pure host logic on the descriptor's shape
 * fields, dtype and pointer alignment: launches nothing, touches no device; d->dbias itself is not looked at.                  */
int gwd_conv_wgrad_takes_bias(const gwd_conv_desc *d, int32_t batched);

/* w (fp32 [N][taps][C]), optionally multiplied by row_scale[N] (a frozen BatchNorm folded into the
 * convolution) -> w_fwd (dtype, same layout; may be NULL) and w_dgrad (dtype, [C][taps][N]; may be
 * NULL).                                                                                          */
int gwd_weight_prep(const float *w, const float *row_scale, void *w_fwd, void *w_dgrad, int32_t N,
                    int32_t taps, int32_t C, int32_t dtype, void *stream);

/* gx = gy * act'(.) ; `ref` is the activation OUTPUT for RELU/ELU/SIGMOID (divided by act_scale
 * internally) and the PRE-activation for GELU.  Optional per-channel multiplier `scale` ([C]).   */
int gwd_act_backward(const void *gy, const void *ref, void *gx, const float *scale, int64_t rows,
                     int32_t C, int32_t act, float act_scale, int32_t dtype, void *stream);

/* out[c] += sum_rows g[row][c]  (bias / shift gradients; fp32 atomics, caller zeroes).           */
int gwd_colsum(const void *g, float *out, int64_t rows, int32_t C, int32_t dtype, void *stream);
/* Up to GWD_COLSUM_BATCH gwd_colsum calls (same dtype) as ONE launch: out[c] += column sums of g for every job.  The
 * records are read on the host and travel in the kernel arguments (nothing is uploaded, nothing must outlive the call).
 * block0 / blocks are filled in by the library.  Returns -4 if a job's C is not a multiple of 16 bytes or wider than
 * 256 vectors (run that one through gwd_colsum).                                                               */
#define GWD_COLSUM_BATCH 16
typedef struct {
    const void *g;        /* [rows][C] (dtype)                       */
    float *out;           /* [C] fp32, accumulated                   */
    int64_t rows;
    int32_t C;
    int32_t block0, blocks;   /* library-internal                    */
} gwd_colsum_job;
int gwd_colsum_batch(const gwd_colsum_job *jobs, int32_t n_jobs, int32_t dtype, void *stream);
/* gwd_act_backward and gwd_colsum of its result in one pass (activation backward of a biased layer: dBias is the column
 * sum of gx).  dbias is ACCUMULATED into.  Returns -4 when C is not a multiple of 16 bytes / wider than 256 vectors:
 * the caller then uses the two separate entry points.                                                            */
/* mult (may be NULL): [rows][C] element-wise multiplier of gy applied first (the dropout multiplier of gwd_conv_desc.mult: the
 * layer computed act(v) * mult, so gx = act'(ref) * (gy * mult)).                                                   */
int gwd_act_backward_colsum(const void *gy, const void *ref, void *gx, float *dbias, int64_t rows, int32_t C, int32_t act,
                            float act_scale, const void *mult, int32_t dtype, void *stream);


/* LayerNorm over the last dim (C <= 512), eps 1e-5, optional fused exact GELU on the output.
 * Replaces nn.LayerNorm (+ nn.GELU) call sites: src/models/points/points_sample.py:19-25,
 * src/models/multiscale_transformerr.py:612-632,659-665,755-777, src/models/transformer.py:138-162,
 * src/models/dense_upsample.py:125,138,166,177.                                                  */
/* residual (may be NULL): [rows][C], added AFTER the normalisation / GELU: y = gelu?(LN(x)) + residual - the skip
 * connection of BasicBlock (src/models/points/points_sample.py:41-42); its gradient is gy itself.              */
/* ld: row pitch in elements of x, residual, y (forward) / gy, x, gx (backward); 0 = C.  With ld > C the channels C..ld-1 are
 * zero padding: never read, WRITTEN as zeros in y / gx (statistics, gamma, beta and their gradients cover the C real channels);
 * needs ld to be a multiple of 16 bytes, else -4 (C itself may be anything).                                      */
int gwd_layernorm_forward(const void *x, const float *gamma, const float *beta, const void *residual, void *y, float *mean,
                          float *rstd, int64_t rows, int32_t C, int32_t ld, int32_t gelu, int32_t dtype, void *stream);
/* gskip (may be NULL): [rows][ld], a second gradient of x added to gx (x also feeds a skip connection); returns -4 when the shape
 * has no vector kernel (the caller then adds it).                                                                   */
/* gelu, backward: bit 0 = GELU behind the norm (as forward); bit 1 (GWD_LN_ELU_INPUT) = x is the output of an ELU (alpha 1) whose
 * own backward pass is left to this call: gx = (gx + gskip) * elu'(x) (upconv1 -> norm of src/models/dense_upsample.py:163-166);
 * -4 when the shape has no vector kernel.                                                                             */
#define GWD_LN_ELU_INPUT 2
int gwd_layernorm_backward(const void *gy, const void *x, const float *gamma, const float *beta,
                           const float *mean, const float *rstd, void *gx, float *dgamma, float *dbeta,
                           int64_t rows, int32_t C, int32_t ld, int32_t gelu, const void *gskip, int32_t dtype, void *stream);

/* Softmax over the last dim (row length L <= 1024), forward and backward.
 * Replaces F.softmax in src/models/multi_head_attention.py:366, multiscale_transformerr.py:307,
 * 322-324,550-552,570,576, points_sample.py:277.                                                 */
int gwd_softmax_forward(const void *x, void *y, int64_t rows, int32_t L, int32_t dtype, void *stream);
int gwd_softmax_backward(const void *gy, const void *y, void *gx, int64_t rows, int32_t L, int32_t dtype,
                         void *stream);
/* Attention softmax with the score scaling and the key-padding mask folded in (src/models/multi_head_attention.py:
 * 329-352: q * scaling, masked_fill(-inf), softmax): y = softmax_row(scale * x + mask), key_mask uint8
 * [rows / rows_per_mask][L] (nonzero = key excluded) or NULL.  Backward: gx = scale * y * (gy - <y, gy>).
 * A row whose keys are all excluded (or all -inf) is NaN in every element, as it is in the reference.          */
int gwd_softmax_masked_forward(const void *x, const uint8_t *key_mask, void *y, int64_t rows, int32_t L, int64_t rows_per_mask,
                               float scale, int32_t dtype, void *stream);
int gwd_softmax_scaled_backward(const void *gy, const void *y, void *gx, int64_t rows, int32_t L, float scale, int32_t dtype,
                                void *stream);


/* SiLog masked reduction (src/models/glassrgbd.py:366-374 with the per-scale nearest-resized GT and
 * validity mask of src/engine_glassrgbd.py:65,76-78 gathered on the fly).
 * pred [B][h][w] (dtype), gt [B][H][W] fp32 at full resolution.  sums[3] (double; caller zeroes)
 * receive sum d, sum d^2, count.  log_depth_error selects d = log p - log g, else (p+log p)-(g+log g). */
int gwd_silog_sums(const void *pred, const float *gt, double *sums, int32_t B, int32_t h, int32_t w,
                   int32_t H, int32_t W, int32_t log_depth_error, int32_t dtype, void *stream);
/* loss (one fp32) = scale * sqrt(sums[1]/n - lambda (sums[0]/n)^2), n = sums[2]: the scalar tail of SiLog as one launch.  */
int gwd_silog_finalize(const double *sums, float lambda, float scale, float *loss, void *stream);
/* gpred = gloss * d loss / d pred, loss = 10*sqrt(E[d^2] - lambda*E[d]^2); reads the sums.        */
int gwd_silog_backward(const void *pred, const float *gt, const double *sums, const float *gloss,
                       float loss_weight, float lambda, void *gpred, int32_t B, int32_t h, int32_t w,
                       int32_t H, int32_t W, int32_t log_depth_error, int32_t dtype, void *stream);

/* Mean 2-class cross entropy over pixels (SegLoss, src/models/glassrgbd.py:376-383):
 * logits [P][2] (dtype), target [P] int64.  sum[1] double (caller zeroes).                        */
int gwd_seg_ce_sum(const void *logits, const int64_t *target, double *sum, int64_t P, int32_t dtype,
                   void *stream);
int gwd_seg_ce_backward(const void *logits, const int64_t *target, const float *gloss, float scale,
                        void *glogits, int64_t P, int32_t dtype, void *stream);

/* Anchor-weighted depth of PointBasedPred (src/models/points/points_sample.py:277-279): pred[b][p] = sum_r att[b][p][r] *
 * anchor[b][r]  (att [B][P][R] dtype = the softmax over the R point channels, anchor [B][R] fp32, pred [B][P] fp32), R <= 256.
 * backward: datt[b][p][r] = gpred[b][p] * anchor[b][r] (dtype, may be NULL), danchor [B][R] fp32 ACCUMULATED (caller zeroes). */
int gwd_anchor_depth_forward(const void *att, const float *anchor, float *pred, int32_t B, int64_t P, int32_t R,
                             int32_t dtype, void *stream);
int gwd_anchor_depth_backward(const void *att, const float *anchor, const float *gpred, void *datt, float *danchor,
                              int32_t B, int64_t P, int32_t R, int32_t dtype, void *stream);

/* A (window, token, head, channel) operand: element = p[w*ws + t*ts + h*hs + d], channel stride 1.      */
typedef struct {
    void *p;
    int64_t ws, ts, hs;
} gwd_strided;

/* Fused 7x7 window attention, 49 tokens per window, head_dim in {4, 8, 16, 32}:
 *   O = softmax(scale * Q K^T + bias[head] (+ -100 where region[token_i] != region[token_j])) V
 * bias is the dense [heads][49][49] fp32 relative-position bias when rel_index is NULL; with rel_index (int32 [49*49], the
 * reference's relative_position_index buffer) bias is the PARAMETER ITSELF, the [n_rel][heads] table (n_rel = 169), and
 * bias(h, i, j) = table[rel_index[i*49+j]][h] is gathered in the kernel - no dense copy, and the backward accumulates
 * straight into a table-shaped gradient (multiscale_transformerr.py:313-316).  region (optional, int32
 * [windows_per_image][49]) encodes the SW-MSA shift mask.  Replaces the attention core of
 * WindowAttention / WindowClassAttention (src/models/multiscale_transformerr.py:311-328, 538-556, mask
 * :937-955).  The backward recomputes P, writes dQ/dK/dV and ACCUMULATES dbias (fp32 atomics; caller zeroes). */
int gwd_winattn_forward(const gwd_strided *q, const gwd_strided *k, const gwd_strided *v, const gwd_strided *o,
                        const float *bias, const int32_t *rel_index, int32_t n_rel, const int32_t *region, int64_t n_windows,
                        int32_t windows_per_image, int32_t heads, int32_t head_dim, float scale, int32_t dtype, void *stream);
int gwd_winattn_backward(const gwd_strided *q, const gwd_strided *k, const gwd_strided *v, const gwd_strided *go,
                         const gwd_strided *gq, const gwd_strided *gk, const gwd_strided *gv, const float *bias,
                         float *dbias, const int32_t *rel_index, int32_t n_rel, const int32_t *region, int64_t n_windows,
                         int32_t windows_per_image, int32_t heads, int32_t head_dim, float scale, int32_t dbias_head_major,
                         int32_t dtype, void *stream);
/* dbias_head_major (with rel_index only): dbias is a [heads][n_rel] scratch instead of the [n_rel][heads] table gradient - a wave's
 * flush is then one contiguous run of atomics instead of n_rel 4-byte adds in n_rel different 64-byte segments (41-59 us of every
 * backward launch); the caller adds the transposed scratch to the table's gradient.                                             */

/* Line-point-guided query rewrite of the 1/32-stage WindowAttention (src/models/multiscale_transformerr.py:295-310), the two
 * batched einsums of the reference as kernels that write the layout their consumer reads:
 *   ref_scores:  ra[b][t][r][h] = scale * sum_d q[b,t,h,d] * ref_k[b,r,h,d]   (t = window*49 + token; q is the (B*nwin, 49, H, hd)
 *                operand inside the packed qkv projection; ref_k (B, R, H*hd); ra (B, nwin*49, R, H) = the pixel-major map the
 *                3x3 "diffusion" conv runs over).  backward: g -> dq (same operand addressing, every element written) and
 *                d_ref_k fp32 (B, R, H*hd), overwritten.
 *   ref_mix:     att = softmax over r of ra[b,t,:,h];  q_new[b][t][h*hd+d] = sum_r att[b,t,r,h] * ref_v[b,r,h,d]; att (B,T,R,H)
 *                is saved for the backward pass (NULL: not written).  backward: att, g -> d_ra (B,T,R,H), d_ref_v fp32.
 * R <= 128, H <= 64, hd <= 64.  No atomics: sums over the tokens are gathered per output element (bit-reproducible).     */
int gwd_ref_scores_forward(const gwd_strided *q, const void *ref_k, void *ra, int32_t B, int32_t nwin, int32_t R, int32_t H,
                           int32_t hd, float scale, int32_t dtype, void *stream);
int gwd_ref_scores_backward(const gwd_strided *q, const void *ref_k, const void *g, const gwd_strided *dq, float *d_ref_k, int32_t B,
                            int32_t nwin, int32_t R, int32_t H, int32_t hd, float scale, int32_t dtype, void *stream);
int gwd_ref_mix_forward(const void *ra, const void *ref_v, void *q_new, void *att, int32_t B, int32_t T, int32_t R, int32_t H,
                        int32_t hd, int32_t dtype, void *stream);
int gwd_ref_mix_backward(const void *att, const void *ref_v, const void *g, void *d_ra, float *d_ref_v, int32_t B, int32_t T,
                         int32_t R, int32_t H, int32_t hd, int32_t dtype, void *stream);

/* Class-token attention of WindowClassAttention (src/models/multiscale_transformerr.py:560-578), per
 * (window, head): A = softmax_c(scale * sum_n q[n][r] k[n][c]), o[n][r] = sum_c A[r][c] v[n][c]; 49 tokens n,
 * r < 4, c < e with e in {12, 16, 24}.  q/o/gq are (W,49,heads,4) operands, k/v/gk/gv (W,49,heads,e).     */
int gwd_tokattn_forward(const gwd_strided *q, const gwd_strided *k, const gwd_strided *v, const gwd_strided *o,
                        int64_t n_windows, int32_t heads, int32_t e, float scale, int32_t dtype, void *stream);
int gwd_tokattn_backward(const gwd_strided *q, const gwd_strided *k, const gwd_strided *v, const gwd_strided *go,
                         const gwd_strided *gq, const gwd_strided *gk, const gwd_strided *gv, int64_t n_windows,
                         int32_t heads, int32_t e, float scale, int32_t dtype, void *stream);

/* A 3x3 convolution over a 2x nearest-upsampled map (src/models/dense_upsample.py:150-181, F.interpolate + Conv2d) seen from its
 * low-resolution input is a 4x4 / stride 2 / pad 1 convolution: the data gradient and the weight gradient run in that form on
 * gwd_conv_forward / gwd_conv_wgrad_batch, 16 taps per low-res pixel instead of 36.  These two are its tap bookkeeping:
 * collapse: w (Cout,3,3,Cin) fp32 -> wk (Cin,4,4,Cout) in `dtype`, wk[ci][t][s][co] = sum_{kh in G(t), kw in G(s)} w[co][kh][kw][ci],
 *           G(0) = {2}, G(1) = {1,2}, G(2) = {0,1}, G(3) = {0};
 * fold:     D (Cin,4,4,Cout) fp32 (the weight gradient of the 4x4 form) -> dw (Cout,3,3,Cin) fp32 += sum_{t in T(kh), s in T(kw)} D[ci][t][s][co],
 *           T(0) = {2,3}, T(1) = {1,2}, T(2) = {0,1}.                                                                              */
int gwd_upsample_taps_collapse(const float *w, void *wk, int32_t Cout, int32_t Cin, int32_t dtype, void *stream);
int gwd_upsample_taps_fold(const float *D, float *dw, int32_t Cout, int32_t Cin, void *stream);

/* Both class tokens of a WindowClassAttention block in ONE launch (multiscale_transformerr.py:561-578: the depth token and the
 * segmentation token query the same global_k / global_v).  The softmax is per query channel, so the pair is one problem with 8
 * query channels: k / v are staged once and the backward's gk / gv are the SUM over both tokens (what autograd adds up after two
 * gwd_tokattn_backward calls).  bf16 only (-2 otherwise: issue the two single calls), e in {12, 16, 24} (-4).                  */
int gwd_tokattn_pair_forward(const gwd_strided *q, const gwd_strided *q2, const gwd_strided *k, const gwd_strided *v,
                             const gwd_strided *o, const gwd_strided *o2, int64_t n_windows, int32_t heads, int32_t e,
                             float scale, int32_t dtype, void *stream);
int gwd_tokattn_pair_backward(const gwd_strided *q, const gwd_strided *q2, const gwd_strided *k, const gwd_strided *v,
                              const gwd_strided *go, const gwd_strided *go2, const gwd_strided *gq, const gwd_strided *gq2,
                              const gwd_strided *gk, const gwd_strided *gv, int64_t n_windows, int32_t heads, int32_t e,
                              float scale, int32_t dtype, void *stream);

/* CertainSample entirely on the device (src/models/points/points_sample.py:291-364): pred_small [B][hs][ws],
 * pred_large [B][H][W] fp32 sigmoid maps, edges[n_intervals+1] fp32 interval bounds -> coords [B][S][2] fp32
 * ((x/W)*2-1, (y/H)*2-1).  Integer-valued selection; bit-exact against the CPU reference on identical operands. */
int gwd_certain_sample(const float *pred_small, const float *pred_large, float *coords, int32_t B, int32_t hs,
                       int32_t ws, int32_t H, int32_t W, const float *edges, int32_t n_intervals,
                       int32_t sample_num, void *stream);

/* Linear sum assignment of the line matcher on the device (replaces scipy.optimize.linear_sum_assignment at
 * src/models/matcher.py:74 and its 6 host syncs per step).  cost [layers][B][Q][sum_targets] fp32 is the block
 * cost matrix of matcher.py:52-70; image b owns columns col_offsets[b] .. col_offsets[b+1]-1 (int32 [B+1]).
 * query_of_target [layers][sum_targets] int32 receives the query matched to every target (Q <= 1024, targets of one
 * image <= 1024, else -4).  An image with MORE targets than queries has every query matched, as scipy does on the
 * Q x T matrix; its surplus targets receive the dummy query index Q.
 * The offsets are DEVICE data: sum_targets may be a fixed capacity larger than col_offsets[B]; the padding columns
 * col_offsets[B] .. sum_targets-1 are never read and receive the dummy query index Q, so one captured launch serves
 * batches with any per-image target counts (max_targets is the host's bound on them, <= 1024).
 * A non-finite cost is read as a large finite one; the kernel's running time is bounded by Q and the counts alone. */
int gwd_lsap(const float *cost, const int32_t *col_offsets, int32_t *query_of_target, int32_t layers, int32_t B,
             int32_t Q, int32_t sum_targets, int32_t max_targets, void *stream);

/* grid_sample (align_corners=False, zero padding) of a pixel-major map (B,H,W,C) at S points per image: coords fp32
 * (B,S,2) = normalised (x, y); mode 0 bilinear, 1 nearest; out fp32 (B,S,C) (src/models/points_sample.py:262-268,
 * multiscale_transformerr.py:688-691).  backward adds the scatter of gout into gmap (map dtype, pre-zeroed by the
 * caller); no gradient w.r.t. coords.                                                                          */
int gwd_point_sample_forward(const void *map, const float *coords, float *out, int32_t B, int32_t H, int32_t W, int32_t C,
                             int32_t S, int32_t mode, int32_t dtype, void *stream);
int gwd_point_sample_backward(const float *gout, const float *coords, void *gmap, int32_t B, int32_t H, int32_t W, int32_t C,
                              int32_t S, int32_t mode, int32_t dtype, void *stream);
/* The same gradient, every element of gmap WRITTEN (no pre-zeroing): a gather over the S <= 256 points per pixel.  Returns -4 when
 * S > 256 (use the pair above).                                                     */
int gwd_point_sample_backward_gather(const float *gout, const float *coords, void *gmap, int32_t B, int32_t H, int32_t W, int32_t C,
                                     int32_t S, int32_t mode, int32_t dtype, void *stream);

/* Nearest sampling of the map as torch.roll(F.pad(map, to (Hf, Wf)), (-shift, -shift), (1, 2)) presents it - the shifted-window frame
 * the 1/32 stage samples its reference points in (multiscale_transformerr.py:662-691) - without building that tensor: coords address
 * the (Hf, Wf) frame, frame pixel (y, x) is map pixel ((y + shift) mod Hf, (x + shift) mod Wf), zero in the padding.  The backward
 * writes every element of gmap (gather form); -4 when S > 256 (pad + roll, then the plain entry points).                          */
int gwd_point_sample_framed_forward(const void *map, const float *coords, float *out, int32_t B, int32_t H, int32_t W, int32_t C,
                                    int32_t S, int32_t Hf, int32_t Wf, int32_t shift, int32_t dtype, void *stream);
int gwd_point_sample_framed_backward(const float *gout, const float *coords, void *gmap, int32_t B, int32_t H, int32_t W, int32_t C,
                                     int32_t S, int32_t Hf, int32_t Wf, int32_t shift, int32_t dtype, void *stream);

/* gwd_weight_prep for many weights in one launch (bf16 outputs).  `jobs` is a DEVICE array; job i owns the blocks
 * [block0_i, block0_{i+1}) of the launch, one 32(n) x 32(c) tile of one tap each: blocks_i = taps*ceil(N/32)*ceil(C/32),
 * block0_0 = 0, total_blocks = sum of blocks_i.
 * w_fwd / w_dgrad may be NULL per job.                                                                          */
typedef struct gwd_prep_job {
    const float *w;          /* fp32 master weight (N, taps, C)                         */
    const float *row_scale;  /* optional per-output-row scale (folded FrozenBN), or NULL */
    void *w_fwd;             /* bf16 (N, taps, C) or NULL                                */
    void *w_dgrad;           /* bf16 (C, taps, N) or NULL                                */
    int32_t N, taps, C;
    int32_t block0;
    int32_t Np, Cg, Cgp;     /* Np > 0: ZERO-PADDED copies - w_fwd is (Np, taps, G*Cgp), w_dgrad (G*Cgp, taps, Np), where the C */
    int32_t reserved;        /* input channels are G = C / Cg groups of Cg, each padded to Cgp; the caller zeroes the copies     */
                             /* once, the launch writes the N x taps x C real entries only.  Np = 0: dense copies as above.      */
} gwd_prep_job;
/* block_job (may be NULL): DEVICE array, job index of every block of the launch (total_blocks int32) - without it each block finds
 * its job by a binary search over the device table (~9 dependent loads in front of one 32 x 32 tile).                       */
int gwd_weight_prep_batch(const gwd_prep_job *jobs, int32_t n_jobs, int32_t total_blocks, const int32_t *block_job, void *stream);

/* The set criterion of the line branch around the device LSAP (gwd_lsap), on PADDED targets (cap columns: column t belongs to image
 * bidx[t], valid[t] = 0 marks padding; the LSAP gives padding columns the dummy query Q).  All tensors fp32 unless noted; K = classes
 * incl. "no object" (<= 8), D = line coordinates (<= 8), else -4.
 *   gwd_match_cost: cost (L,B,Q,cap) = w_line * L1(lines (L,B,Q,D), tgt_lines (cap,D)) - w_class * softmax(logits (L,B,Q,K))[tgt_labels
 *     (cap, int64)]  (HungarianMatcher_Line.forward, src/models/matcher.py:52-70).
 *   gwd_set_losses_forward: per layer l: target_class (L,B,Q) int32 (the matched target's label at query qot[l][t], K-1 elsewhere),
 *     ce[l] = sum(nll * w) / sum(w) with w = class_weight[target class], wsum[l] = sum(w), l1[l] = sum over valid t of
 *     |lines[l, bidx[t], qot] - tgt_lines[t]|_1 / max(num_items[0] / world, 1)   (src/models/glassrgbd.py:160-170,231-244); a valid t
 *     with qot = Q (a surplus target of an image with more targets than queries) has no label and no L1 term, forward and backward.
 *   gwd_set_losses_backward: dlogits (fully written) and dlines (ADDED to: caller zeroes) from g_ce[L] / g_l1[L] (either may be NULL).
 *   gwd_set_losses_focal_forward / _backward: the same operands plus gamma (>= 0, else -1), for --label_loss_func focal_loss
 *     (SetCriterion.label_focal_loss, src/models/glassrgbd.py:177-194).  With c the target class of a query, p = softmax(logits),
 *     p_t = p[c], nll = -log p_t, w = class_weight[c] and u = 1 - p_t taken as the SUM OF THE OTHER classes' probabilities (no
 *     cancellation when p_t rounds to 1):  ce[l] = sum(w * nll * u^gamma) / (B*Q) - a plain mean over the queries, NOT the weighted
 *     mean of the pair above (wsum is still written, and ignored by the backward);  d ce[l] / d logits[k] = g_ce[l] * w / (B*Q) *
 *     (p_k - [k = c]) * (u^gamma + gamma * u^(gamma-1) * p_t * nll), with u^0 = 1 also at u = 0 and the second term absent for
 *     gamma = 0.  target_class, l1 and dlines are those of the pair above.                                                         */
int gwd_match_cost(const float *logits, const float *lines, const float *tgt_lines, const int64_t *tgt_labels, float *cost, int32_t L,
                   int32_t B, int32_t Q, int32_t cap, int32_t K, int32_t D, float w_line, float w_class, void *stream);
int gwd_set_losses_forward(const float *logits, const float *lines, const float *tgt_lines, const int64_t *tgt_labels, const int32_t *bidx,
                           const int32_t *valid, const int32_t *qot, const float *class_weight, const float *num_items, float world,
                           int32_t *target_class, float *ce, float *l1, float *wsum, int32_t L, int32_t B, int32_t Q, int32_t cap,
                           int32_t K, int32_t D, void *stream);
int gwd_set_losses_backward(const float *logits, const float *lines, const float *tgt_lines, const int32_t *bidx, const int32_t *valid,
                            const int32_t *qot, const float *class_weight, const float *num_items, float world,
                            const int32_t *target_class, const float *wsum, const float *g_ce, const float *g_l1, float *dlogits,
                            float *dlines, int32_t L, int32_t B, int32_t Q, int32_t cap, int32_t K, int32_t D, void *stream);
int gwd_set_losses_focal_forward(const float *logits, const float *lines, const float *tgt_lines, const int64_t *tgt_labels,
                                 const int32_t *bidx, const int32_t *valid, const int32_t *qot, const float *class_weight,
                                 const float *num_items, float world, float gamma, int32_t *target_class, float *ce, float *l1, float *wsum,
                                 int32_t L, int32_t B, int32_t Q, int32_t cap, int32_t K, int32_t D, void *stream);
int gwd_set_losses_focal_backward(const float *logits, const float *lines, const float *tgt_lines, const int32_t *bidx, const int32_t *valid,
                                  const int32_t *qot, const float *class_weight, const float *num_items, float world, float gamma,
                                  const int32_t *target_class, const float *wsum, const float *g_ce, const float *g_l1, float *dlogits,
                                  float *dlines, int32_t L, int32_t B, int32_t Q, int32_t cap, int32_t K, int32_t D, void *stream);

/* Padding mask of one feature level + sine position embeddings from it (src/models/backbone.py:81-88: F.interpolate(nearest) of the
 * batch mask; src/models/position_encoding.py:28-48: PositionEmbeddingSine).  Two stages, either may be skipped:
 *   mask_full != NULL: mask_level (B,h,w) u8 = nearest-resized mask_full (B,H,W) u8 (non-zero = padding), counts (B,h,w,2) int16 =
 *                      cumulative counts of un-masked pixels along y and along x;
 *   out != NULL:       out (B,h,w,2F) fp32 = [sin|cos interleaved of y / dim_t[c]] | [the same of x], from `counts`; normalize: counts
 *                      scaled to 2 pi by the last row / column (eps 1e-6); dim_t (F) fp32 = temperature^(2 (c/2) / F) from the caller.
 * One level's counts serve any number of embeddings (the reference builds several widths from one mask).                          */
int gwd_pos_sine(const uint8_t *mask_full, uint8_t *mask_level, int16_t *counts, const float *dim_t, float *out, int32_t B, int32_t H,
                 int32_t W, int32_t h, int32_t w, int32_t F, int32_t normalize, void *stream);

/* The ResNet stem in one forward-only kernel: conv 7x7 / stride 2 / pad 3 (3 -> 64 channels) + folded FrozenBatchNorm + ReLU +
 * max-pool 3x3 / stride 2 / pad 1 - conv1 / bn1 / relu / maxpool of torchvision's resnet50 as src/models/backbone.py:65-92 runs
 * them (frozen there: backbone.py:62-64).  x bf16 [B][H][W][3] -> y bf16 [B][Hp][Wp][64], Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (W alike).
 * `packed` = the weights as gwd_stem_pack leaves them (w fp32 [64][7][7][3], times scale[64] when given: the BN scale), i.e.
 * GWD_STEM_PACKED_ELEMS bf16 values in the kernel's operand order; shift fp32 [64] (BN shift) or NULL.  dtype: GWD_BF16 only (-2). */
#define GWD_STEM_PACKED_ELEMS (14 * 2 * 64 * 8)
int gwd_stem_pack(const float *w, const float *scale, void *packed, void *stream);
int gwd_stem_forward(const void *x, const void *packed, const float *shift, void *y, int32_t B, int32_t H, int32_t W, int32_t dtype,
                     void *stream);

/* The other half of the zero-padded copies: a layer that ran on padded channel counts (its activations keep the padded width, so every
 * conv / Linear on them takes the LDS-DMA route; the 30 / 60 / 300-channel pyramid of src/models/points/points_sample.py:45-125
 * is the user) gets its weight gradient in the padded shape; this folds it back: dst (N, taps, G*Cg) += src (.., taps, G*Cgp)
 * rows 0..N-1, group g channels 0..Cg-1.  Up to GWD_UNPAD_BATCH jobs per call = ONE launch; jobs are read on the host (by value
 * in the kernel arguments); block0 is filled in by the library.                                                              */
#define GWD_UNPAD_BATCH 24
typedef struct gwd_unpad_job {
    const float *src;        /* fp32 (>= N, taps, G*Cgp)                                */
    float *dst;              /* fp32 (N, taps, G*Cg), accumulated                       */
    int32_t N, taps, G, Cg, Cgp;
    int32_t block0;
} gwd_unpad_job;
int gwd_unpad_add_batch(const gwd_unpad_job *jobs, int32_t n_jobs, void *stream);

/* y = a + gelu((u - mean_bc(u)) * rsqrt(var_bc(u) + eps)), statistics over the L positions of image b for channel c;
 * a, u, y are (B, L, C), channel innermost (src/models/multiscale_transformerr.py:299-302: conv -> instance
 * normalisation -> GELU -> residual of the reference-point attention logits).  part: fp32 scratch [B][S][C][2]
 * (S slices per image, caller-chosen, fully overwritten); stat: fp32 [B][C][2] = (mean, rstd) saved for backward.
 * backward: du from gy (the gradient w.r.t. a is gy itself).  C * sizeof(dtype) / 16 must be a power of two.     */
int gwd_inorm_gelu_forward(const void *a, const void *u, void *y, float *part, float *stat, int64_t B, int64_t L, int32_t C,
                           int32_t S, float eps, int32_t dtype, void *stream);
int gwd_inorm_gelu_backward(const void *gy, const void *u, const float *stat, float *part, void *du, int64_t B, int64_t L,
                            int32_t C, int32_t S, int32_t dtype, void *stream);

/* Window partition (gather != 0) / reverse (gather == 0) of a (B,H,W,C) token map into (B*nWin,49,C) 7x7 windows
 * with zero padding to multiples of 7 and cyclic shift `shift` (src/models/multiscale_transformerr.py:667-676,
 * 705-707 / 730-747).  Rows of whole 16-byte vectors (C * sizeof(dtype) % 16 == 0) move 16 bytes per thread, any other C one
 * element per thread.  residual (reverse only, may be NULL): a (B,H,W,C)
 * map added to the result - the block's residual stream, `x = shortcut + x` of :749.                           */
int gwd_window_map(const void *src, void *dst, const void *residual, int32_t B, int32_t H, int32_t W, int32_t C, int32_t shift,
                   int32_t gather, int32_t dtype, void *stream);
/* The same for n <= GWD_WINMAP_JOBS maps of one geometry (B, H, W, shift) and channel counts C[i] in ONE launch: the three maps a
 * Swin block with class tokens hands over together (features, depth tokens, seg tokens: multiscale_transformerr.py:700-747).
 * src / dst / residual: HOST arrays of n device pointers (residual, or single entries of it, may be NULL).  16-byte rows only:
 * -4, before anything is launched, when some C[i] * sizeof(dtype) is not a multiple of 16 (the caller issues gwd_window_map
 * per map).                                                                                                        */
#define GWD_WINMAP_JOBS 4
int gwd_window_map_multi(const void *const *src, void *const *dst, const void *const *residual, const int32_t *C, int32_t n,
                         int32_t B, int32_t H, int32_t W, int32_t shift, int32_t gather, int32_t dtype, void *stream);

/* Pixel-major resampling ([B][H][W][C]).  mode 0 = bilinear align_corners=True (PSP branches of
 * src/models/points/points_sample.py:114-121, CertainSample :293), mode 1 = legacy nearest
 * floor(dst*in/out) (src/models/multiscale_transformerr.py:1193,1230,1240,1267).  The backward kernels are
 * gathers over each source pixel's footprint (no atomics, bitwise reproducible).                    */
enum { GWD_RESAMPLE_BILINEAR_AC = 0, GWD_RESAMPLE_NEAREST = 1 };
/* ldy: pixel pitch of y in elements (0 = C).  ldy > C writes the result into a channel slice of a wider map (the PSP concat of
 * points_sample.py:114-122 without a concat pass); vector-sized C and ldy only, else -4.  y itself must start on a vector of the
 * kernel that runs (16 bytes; 8 for bf16 with C % 8 == 4), else -4: a slice that begins inside one cannot be written in place. */
int gwd_resample_forward(const void *x, void *y, int32_t B, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo,
                         int32_t C, int32_t mode, int32_t ldy, int32_t dtype, void *stream);
/* gate (may be NULL) [B][Hs][Ws][C] + gate_act (GWD_ACT_RELU / GWD_ACT_ELU): gx is multiplied by act'(.) of the activation whose
 * OUTPUT is `gate` (the source map of an up-sampling convolution, see gwd_conv_desc.gate); nearest mode with C a multiple of 4, else -4. */
int gwd_resample_backward(const void *gy, void *gx, int32_t B, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo,
                          int32_t C, int32_t mode, const void *gate, int32_t gate_act, int32_t dtype, void *stream);
/* gwd_resample_backward as two separable passes (x, then y) through a caller-provided fp32 scratch tmp[B][Ho][Ws][C]:
 * the same sums in the same order, but 2r+2 taps per thread instead of (2r+2)^2 (13x faster at the 16x pyramid
 * branches).  Returns -4 when C is not a multiple of 16 bytes (use gwd_resample_backward).                       */
/* ldg: pixel pitch of gy in elements (0 = C): the gradient of a channel slice read in place; gy not aligned to the vector
 * width (16 bytes; 8 for bf16 with C % 8 == 4) returns -4 as well.                                                 */
int gwd_resample_backward_sep(const void *gy, float *tmp, void *gx, int32_t B, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo,
                              int32_t C, int32_t mode, int32_t ldg, int32_t dtype, void *stream);

/* k x k / stride k average pooling (nn.AvgPool2d(k, stride=k), points_sample.py:61-75), floor mode.  */
/* dst (B,H,W,C) = [residual +] src (B,Ho,Wo,C) placed on the pixels (stride*i, stride*j), zero elsewhere: with a plain GEMM over
 * the output pixels this is the data gradient of a 1x1 convolution with stride > 1 (the ResNet downsample convs,
 * src/models/backbone.py:90-92), a quarter of the transposed-gather work.  C a multiple of 16 bytes, else -4.        */
int gwd_stride_place(const void *src, const void *residual, void *dst, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t C,
                     int32_t stride, int32_t dtype, void *stream);

/* The four average pools of the PSP module (F.avg_pool2d with k = 16, 8, 4, 2; src/models/points/points_sample.py:107-113) from
 * ONE pass over x (B,H,W,C): p_k (B,H/k,W/k,C).  Backward in one pass as well: gx = g_pass + sum_k g_k[y/k][x/k] / k^2, where g_pass
 * (may be NULL; pixel pitch ldg, 0 = C) is the gradient that reaches the map directly - on this path the first channel slice of the
 * concat's gradient, read in place.  Any g_k may be NULL.  H, W >= 16; C (and ldg) multiples of 16 bytes and g_pass 16-byte
 * aligned, else -4.                                                                                                    */
int gwd_psp_pool_forward(const void *x, void *p16, void *p8, void *p4, void *p2, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t dtype, void *stream);
int gwd_psp_pool_backward(const void *g_pass, const void *g16, const void *g8, const void *g4, const void *g2, void *gx, int32_t B,
                          int32_t H, int32_t W, int32_t C, int32_t ldg, int32_t dtype, void *stream);
/* Low-resolution tail of the PSP module (the 3x3 ConvLn over [x | up(y_1) | ...], points_sample.py:114-125).  A convolution and
 * the align-corners bilinear resize `up` are both linear, so  conv3x3(up(y))(p) = sum_tap [p + tap inside] up(W_tap . y)(p + tap):
 * the caller forms the nine channel products of a branch on its low-resolution pixels, Z_k (B,h_k,w_k,9,N) = a 1x1 convolution of
 * y_k with the weight slice as (9 N, C), taps in the weight's order, and convolves only [x | the remaining branches] at (H, W).
 *   forward:  z = part + sum_k sum_tap [p + tap inside] bilinear_ac(Z_k[.., tap, :])(p + tap),  y = [GELU](LayerNorm(z) gamma + beta);
 *             part (B,H,W,N) is the high-resolution convolution's output; z (may be NULL: not stored), mean, rstd [B*H*W] are
 *             exactly what gwd_layernorm_backward takes (statistics of z as stored, two passes, eps 1e-5); fp32 accumulation.
 *   backward: G_k (B,h_k,w_k,9,N) = the gradient of Z_k from gz (B,H,W,N): every element is one gather over its pixel's footprint,
 *             summed in a fixed order (no atomics: bit-reproducible).
 *   fold:     dw (N,3,3,(1+nbr) C2) fp32 += d_hi (N,3,3,(1+nbr-nlow) C2), the weight gradient of the high-resolution part (x and the
 *             last nbr - nlow branches), and d_low[k] (9 N, C2), the 1x1 weight gradients of the first nlow branches.
 * 1 <= nb <= GWD_PYR_MAX_BRANCHES, h_k <= H, w_k <= W (h_k == 1: every pixel reads row 0).  -4 (nothing launched): N not a multiple
 * of 32 (backward: 8) or above 320, or a branch so fine that an 8x8 tile and its ring reach more than 5 of its rows or columns.  No allocation, no
 * memset, no host synchronisation: all three may be captured.                                                              */
#define GWD_PYR_MAX_BRANCHES 4
int gwd_pyr_tail_forward(const void *part, const void *const *Z, const int32_t *hk, const int32_t *wk, int32_t nb,
                         const float *gamma, const float *beta, void *z, void *y, float *mean, float *rstd, int32_t B,
                         int32_t H, int32_t W, int32_t N, int32_t gelu, int32_t dtype, void *stream);
int gwd_pyr_tail_backward(const void *gz, void *const *G, const int32_t *hk, const int32_t *wk, int32_t nb, int32_t B, int32_t H,
                          int32_t W, int32_t N, int32_t dtype, void *stream);
int gwd_pyr_tail_fold_wgrad(const float *d_hi, const float *const *d_low, int32_t nlow, float *dw, int32_t N, int32_t C2,
                            int32_t nbr, void *stream);
int gwd_avgpool_forward(const void *x, void *y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                        int32_t dtype, void *stream);
int gwd_avgpool_backward(const void *gy, void *gx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                         int32_t dtype, void *stream);

/* sq[0] += sum g^2 over a flat fp32 buffer (double; caller zeroes).  clip_grad_norm_ numerator.    */
int gwd_sqnorm(const float *g, double *sq, int64_t n, void *stream);
/* Fused clip_grad_norm_(max_norm) + torch.optim.AdamW step on a flat fp32 range
 * (src/engine_glassrgbd.py:157-159, src/main_glassrgbd.py:59-66).  coef = min(1, max_norm/(sqrt(sq)+1e-6))
 * is computed on device from sq[0]; grad_scale pre-multiplies g (1/world_size for DDP mean).
 * Optionally refreshes the bf16 shadow copy of the parameters.                                    */
int gwd_adamw_step(float *p, const float *g, float *m, float *v, void *p_bf16, const double *sq,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float bias_corr1, float bias_corr2, float max_norm, float grad_scale, void *stream);

/* Dense evaluation metrics of a batch of B images with H*W = HW pixels each, accumulated on the device.
 * Replaces the device->host copies and per-image numpy of evaluate(): the prediction clamp and GT validity mask
 * (src/engine_glassrgbd.py:249-253), compute_depth_errors (src/util/metrics.py:198-218), the argmax + ignore-255
 * confusion counts of compute_mean_ioU / get_confusion_matrix (src/util/metrics.py:37-74, engine :236-241) and the
 * running sums `depth_eval_measures[:9] += measures; [9] += 1` (engine :262-263).
 *   pred_depth [B][HW] (depth_dtype), gt_depth [B][HW] fp32 - both NULL: no depth part;
 *   seg_logits: class c of pixel i of image b at seg_logits[b*seg_sb + i*seg_sp + c*seg_sc] (seg_dtype; element strides, so
 *               both the reference's (B,2,H,W) and the pixel-major (B,H,W,2) layout are read in place),
 *   seg_gt [B][HW] int64 (255 = ignore)                     - both NULL: no segmentation part;
 *   workspace: gwd_query_workspace(GWD_WS_EVAL, {B, HW}) bytes, fully overwritten;
 *   measures [B][9] f64 OUT: silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3 of each image (engine :204 order;
 *               all NaN for an image without a valid pixel, as numpy's mean of an empty array);
 *   running [10] f64 IN/OUT: += the nine measures of every image, in image order; [9] += B;
 *   confusion [4] int64 IN/OUT: [gt*2 + pred] += pixel counts.
 * Per-pixel terms are formed in fp32 exactly as numpy forms them (IEEE division, so the three threshold counts are
 * bit-exact); sums are f64 and folded in a fixed order: results are bit-reproducible.  Two launches, no atomics.     */
#define GWD_EVAL_NSUM 10
int gwd_eval_accumulate(const void *pred_depth, const float *gt_depth, const void *seg_logits, int64_t seg_sb,
                        int64_t seg_sp, int64_t seg_sc, const int64_t *seg_gt, void *workspace, double *measures,
                        double *running, int64_t *confusion, int32_t B, int64_t HW, float min_depth,
                        float max_depth, int32_t depth_dtype, int32_t seg_dtype, void *stream);

/* Inference post-processing of the dense outputs, one streaming pass behind the forward (csrc/postproc.hip).
 *   depth [B][H][W] (depth_dtype); seg_logits: class c of pixel i of image b at seg_logits[b*seg_sb + i*seg_sp + c*seg_sc]
 *   (seg_dtype; element strides as for the evaluation entry point above); sizes [B][2] int32 = the un-padded (h, w) of each image
 *   (images are top-left aligned), NULL = all of H x W.
 *   depth_out [B][H][W] fp32, depth_mm [B][H][W] uint16 (may be NULL), label [B][H][W] uint8 - every element written.
 * Inside (h, w): depth_out = the clamp of src/engine_glassrgbd.py:249-252 in that order (< min -> min, > max -> max, +inf -> max,
 * NaN -> min, hence -inf -> min); depth_mm = rint(depth_out * 1000) saturated to [0, 65535] (the data set's PNG convention,
 * src/datasets/glassrgbd_norhint.py:273); label = argmax of the two logits by torch.argmax's rules (tie -> 0, a NaN logit is the
 * maximum, the first one wins).  Outside: depth_out 0, depth_mm 0, label 255 (the ignore value of src/util/metrics.py).
 * 16-byte accesses when W % 8 == 0, the logits are interleaved (seg_sp 2, seg_sc 1) or planar (seg_sp 1, seg_sc % 8 == 0),
 * seg_sb % 8 == 0 and all bases are 16-byte aligned; one pixel per thread otherwise.  All shapes are accepted.  One launch. */
int gwd_dense_postprocess(const void *depth, const void *seg_logits, int64_t seg_sb, int64_t seg_sp, int64_t seg_sc,
                          const int32_t *sizes, float *depth_out, uint16_t *depth_mm, uint8_t *label, int32_t B, int32_t H,
                          int32_t W, float min_depth, float max_depth, int32_t depth_dtype, int32_t seg_dtype, void *stream);

/* gwd_dense_postprocess with a bilinear resize to a per-image output size and an optional mirrored twin (the horizontal-mirror
 * ensemble of depth evaluation), one streaming launch, every output element written, no memset, no atomics.
 *   depth [Bs][H][W], seg_logits (strides as above) with Bs = B + twin source images; sizes [B][2] int32 = the un-padded (h, w) of
 *   each image (NULL = H x W) and frame_sizes [B][2] int32 = its output (fh, fw), both DEVICE data (values outside the allocated
 *   extents are clamped to them); twin = 0: no ensemble; twin > 0: image b's twin is source image b + twin, of the same (h, w);
 *   Fh, Fw: the allocated output extent, fh <= Fh, fw <= Fw.
 *   depth_out [B][Fh][Fw] fp32, depth_mm [B][Fh][Fw] uint16 (may be NULL), label [B][Fh][Fw] uint8.
 * Source sample at (y, x), y < h, x < w: s = san(depth[b][y][x]), san = the clamp above; with a twin
 * s = 0.5f * (san(depth[b][y][x]) + san(depth[b + twin][y][w - 1 - x])) and the logits are the sums of the two, class by class.
 * Resize: F.interpolate(mode = "bilinear", align_corners = False) over the un-padded h x w region (padding is never read), down-
 * scaling by the same rule (no anti-aliasing), with exact integer coordinates: n = max((2 d + 1) h - fh, 0), i0 = n / (2 fh),
 * lambda = float(n % (2 fh)) / float(2 fh), i1 = min(i0 + 1, h - 1), and the same along x; rows are blended first, then columns,
 * each as (1 - lambda) a + lambda b in fp32; a tap of weight zero does not enter (its NaN or inf stays out).
 * Inside (fh, fw): depth_out = the interpolated s kept inside [min, max], depth_mm = rint(depth_out * 1000) saturated, label = argmax of the interpolated
 * logits by the rules above.  Outside: 0 / 0 / 255.  fh == h, fw == w, twin == 0 gives gwd_dense_postprocess bit for bit.
 * 8 pixels per thread (16-byte stores) when Fw % 8 == 0 and the outputs are 16-byte aligned (label: 8), one pixel otherwise;
 * 16-byte source loads when W % 8 == 0, the logits are interleaved or planar as above and the sources are 16-byte aligned.
 * -1 on bad arguments, among them any of H, W, Fh, Fw above 16384.                                                           */
int gwd_dense_postprocess_resized(const void *depth, const void *seg_logits, int64_t seg_sb, int64_t seg_sp, int64_t seg_sc,
                                  const int32_t *sizes, const int32_t *frame_sizes, int32_t twin, float *depth_out,
                                  uint16_t *depth_mm, uint8_t *label, int32_t B, int32_t H, int32_t W, int32_t Fh, int32_t Fw,
                                  float min_depth, float max_depth, int32_t depth_dtype, int32_t seg_dtype, void *stream);

/* PostProcess_Line 'prediction' for two classes (src/models/glassrgbd.py:470-477) plus a ranking, one workgroup per image.
 *   logits [B][Q][2] fp32, lines [B][Q][ld] fp32 with ld 4 or 6, sizes [B][2] int32 (h, w), thresh;
 *   scores [B][Q] fp32 = softmax probability of class 0 (the labels are all 0), lines_px [B][Q][4] fp32 (16-byte aligned) = the
 *   first four coordinates times (w, h, w, h), both in query order; order [B][Q] int32 = query indices by score descending, equal
 *   scores by lower index first (a NaN score ranks above every number, as torch.sort has it); count [B] int32 = scores > thresh.
 * Q <= 1024, else -2.  One launch, no atomics.                                                                              */
int gwd_line_postprocess(const float *logits, const float *lines, const int32_t *sizes, float *scores, float *lines_px,
                         int32_t *order, int32_t *count, int32_t B, int32_t Q, int32_t ld, float thresh, void *stream);

/* Structural-AP scoring of the detected lines, one workgroup per image (csrc/linescore.hip; the scalar geometry is csrc/linescore.h).
 * Replaces, per image, what the reference does on the host between evaluate(save_line=True) and its offline scripts:
 *   score = softmax probability of class 0 (src/engine_glassrgbd.py:287,297); the first two points of every query as (y, x) times
 *   (h, w) in fp32; the duplicate trim at the first i > 0 whose line (all ld values) equals line 0 (evaluation/eval_post_online.py:
 *   127-131); L-CNN's line NMS postprocess(lines, scores, diag * t, tol = 0, do_clip = False) (eval_post_online.py:44-91,142) for
 *   each of the T thresholds, with the lines in QUERY order as the reference passes them (not score order); the kept lines times
 *   (128 / h, 128 / w) (:174-175); the second duplicate trim (evaluation/eval-sAP-glassrgbd.py:55-59); and msTPFP
 *   (evaluation/lcnn/metric.py:194-210) against gt * 128 for each of the S squared-distance thresholds.
 * Precision: pinned to f64 after the fp32 scaling, no contraction - the reference's own precision depends on its NumPy version.
 *   logits [B][Q][2] fp32, lines [B][Q][ld] fp32 (ld 4 or 6, x before y), sizes [B][2] int32 (h, w), gt [B][G][4] fp32 normalised
 *   (x1, y1, x2, y2) of which the first gt_count[b] (int32, clamped to [0, G]) rows count (gt may be NULL when G = 0; an image
 *   without ground truth scores every kept line as a false positive); nms_thresholds [T] and sap_thresholds [S]: HOST arrays,
 *   1 <= T, S <= 4, fractions of the image diagonal and squared distances in the 128 x 128 space.
 * Outputs are an accumulator's buffers of `capacity` image slots; images slot .. slot + B - 1 are written, every element of them:
 *   flag [T][S][capacity][Q] uint8: 0 false positive, 1 true positive, 2 not scored (suppressed or behind a trim);
 *   kept_lines [T][capacity][Q][4] f64: (y1, x1, y2, x2) of the kept (clipped) lines in the 128 x 128 space, zeros elsewhere;
 *   score [capacity][Q] fp32; gt_seen [capacity] int32 = the clamped gt_count.
 * A kept line is a true positive iff its distance is below the threshold and no EARLIER kept line with the same choice of ground
 * truth was (first minimum on ties) - the hit array of msTPFP without its serial walk.
 * -1 on bad arguments (slot + B > capacity among them), -2 when Q > 1024 or G > 1024.  One launch, no atomics, no memset. */
int gwd_line_score(const float *logits, const float *lines, const int32_t *sizes, const float *gt, const int32_t *gt_count,
                   const double *nms_thresholds, int32_t T, const double *sap_thresholds, int32_t S, uint8_t *flag,
                   double *kept_lines, float *score, int32_t *gt_seen, int32_t B, int32_t Q, int32_t ld, int32_t G,
                   int64_t capacity, int64_t slot, void *stream);

/* PlaneLoss (src/models/glassrgbd.py:385-450, --with_plane_norm_loss) of ONE image, on the device: Sobel normals of the
 * predicted depth (src/models/losses/sobel.py:5-27), the masks of up to P <= 64 line triangles restricted to the valid
 * pixels (the reference: matplotlib.path.Path.contains_points on the host; same crossing test here, exact in integers),
 * per-plane biased variances of both normal components; loss = sum over planes with >= min_area pixels / max(1, count).
 *   depth [H][W] (dtype), valid [H][W] uint8, tri [P][6] int64 = (x0,y0,x1,y1,x2,y2) already rounded and clamped (:413-418),
 *   n_planes: DEVICE int32 - only the first *n_planes triangles count (the reference's data-dependent top_num, :400, without
 *   a host round trip); workspace: gwd_query_workspace(GWD_WS_PLANE, {P, H*W}) bytes;
 *   stats [4*P + 1] f64 OUT: per plane n, mean_x, mean_y, active; then the number of active planes (read by the backward);
 *   loss [1] fp32 OUT.  backward: gdepth [H][W] (dtype) = gloss[0] * d loss / d depth (every element written).          */
int gwd_plane_loss_forward(const void *depth, const uint8_t *valid, const int64_t *tri, const int32_t *n_planes, int32_t P,
                           int32_t H, int32_t W, int32_t min_area, void *workspace, double *stats, float *loss,
                           int32_t dtype, void *stream);
int gwd_plane_loss_backward(const void *depth, const uint8_t *valid, const int64_t *tri, const int32_t *n_planes, int32_t P,
                            int32_t H, int32_t W, const double *stats, const float *gloss, void *gdepth, int32_t dtype,
                            void *stream);

/* Multi-head attention core on the matrix cores, flash style (csrc/mfattn.hip): head_dim 32, bf16, ANY L and S; no L x S
 * matrix reaches memory (replaces q*scaling, bmm, masked_fill, softmax, dropout, bmm and the head split / merge copies of
 * src/models/multi_head_attention.py:329-375, and their autograd backward).
 *   q: row (b, l) at q + (b*L + l)*q_ts, head h in channels [32h, 32h+32); q_ts, k_ts, ... are TOKEN strides in elements
 *   (multiples of 8, 16-byte aligned bases), so slices of a packed in-projection are read - and their gradients written -
 *   in place; k, v likewise with S tokens per image.  key_padding_mask [B][S] uint8 (nonzero = excluded) or NULL;
 *   mult [B][H][L][S] bf16 dropout multipliers (0 or 1/(1-p)) or NULL.
 *   forward:  out (b, l) rows with token stride o_ts, heads merged; lse [B][H][L] fp32 = log-sum-exp of the scaled, masked
 *             scores of every query (saved for the backward pass).
 *   backward: go -> gq, gk, gv (same addressing); out / lse from the forward; delta [B][H][L] fp32 is scratch.  Every output
 *             row is written by exactly one wave (no atomics): bit-reproducible.
 * Returns -2 for a dtype other than GWD_BF16 (the fp32 parity mode keeps the unfused path).                               */
int gwd_mha_flash_forward(const void *q, const void *k, const void *v, int64_t q_ts, int64_t k_ts, int64_t v_ts,
                          const uint8_t *key_padding_mask, const void *mult, void *out, int64_t o_ts, float *lse, int32_t B,
                          int32_t H, int32_t L, int32_t S, float scale, int32_t dtype, void *stream);
int gwd_mha_flash_backward(const void *q, const void *k, const void *v, const void *go, const void *out, int64_t q_ts,
                           int64_t k_ts, int64_t v_ts, int64_t go_ts, int64_t o_ts, const uint8_t *key_padding_mask,
                           const void *mult, const float *lse, float *delta, void *gq, void *gk, void *gv, int64_t gq_ts,
                           int64_t gk_ts, int64_t gv_ts, int32_t B, int32_t H, int32_t L, int32_t S, float scale, int32_t dtype,
                           void *stream);

/* Batch assembly from raw decoded images (the tail of the input pipeline): ToTensor + Normalize
 * (src/datasets/transforms_depth.py:618-660; torchvision's to_tensor / normalize: x/255, - mean, / std in fp32), the
 * dataset's depth_mm / 1000 and label > 0 (src/datasets/glassrgbd_norhint.py:277-281) and collate_fn_aux's zero padding
 * + padding mask (src/util/misc.py:273-313), one launch for up to GWD_COLLATE_BATCH images.
 *   jobs[i]: device pointers to image i as decoded - rgb uint8 [h][w][3], depth_mm int32 [h][w], labels uint8 [h][w] (a
 *            pointer may be NULL when the matching output is NULL); read on the host, passed in the kernel arguments;
 *   images [n][H][W][3] (dtype, pixel-major), mask [n][H][W] uint8 (1 = padding), depth [n][H][W] fp32 metres,
 *   seg [n][H][W] int64 {0,1}; every element is written (padding = 0); any output may be NULL.                      */
/* The geometric transforms of the input pipeline on decoded images (src/datasets/transforms_depth.py:59-372: hflip / vflip, crop,
 * resize), bit-exact with the Pillow calls the reference makes through torchvision; tables are built by the caller on the host
 * (gw_depth_amd/data.py shows how; oracle/pil_resize_ref.py is the numpy restatement the tests pin against Pillow).
 * gwd_resample_u8_pass: ONE separable pass of Image.resize(BILINEAR) over uint8 pixels with C interleaved channels:
 *   axis 1 (horizontal): dst [other][n_out][C],  dst[j][o][c] = clip8((2^21 + sum_t src[row(j)][col(first_o + t)][c] * kk[o][t]) >> 22)
 *   axis 0 (vertical):   dst [n_out][other][C],  dst[o][j][c] = ... src[row(first_o + t)][col(j)][c] ...
 *   bounds (n_out,2) int32 = (first source index, tap count), kk (n_out,ksize) int32 fixed-point coefficients (22 fractional bits);
 *   index maps along the resampled axis i -> base0 + step0 * i and along the other axis j -> base1 + step1 * j (step = +-1): a flip
 *   and / or a crop window of the source folded into the read; src_row_stride in elements.
 * gwd_gather2d: dst[y][x] = src[ytab[y]][xtab[x]] for elements of 1-4 bytes (NEAREST resize / flip / crop of depth and label maps;
 *   flips and crops of RGB), src_row_stride in BYTES.                                                                             */
int gwd_resample_u8_pass(const uint8_t *src, uint8_t *dst, const int32_t *bounds, const int32_t *kk, int32_t ksize, int32_t axis,
                         int32_t n_out, int32_t other, int32_t C, int64_t src_row_stride, int32_t base0, int32_t step0, int32_t base1,
                         int32_t step1, void *stream);
int gwd_gather2d(const void *src, void *dst, const int32_t *ytab, const int32_t *xtab, int32_t oh, int32_t ow,
                 int64_t src_row_stride_bytes, int32_t elem_bytes, void *stream);

/* The same passes for a whole BATCH of frames, one launch each whatever the number of frames.  The job records are read on the
 * host and travel in the kernel arguments; block0 / blocks are filled in by the library.  Every job's tables live at int32
 * offsets inside ONE device buffer `tables` of table_len int32 values, which the caller uploads once per batch; an offset or
 * extent beyond table_len returns -3.  Nothing else is uploaded, nothing is allocated, nothing synchronises.
 * gwd_resample_u8_pass_batch: job i has exactly the meaning of gwd_resample_u8_pass(src, dst, tables + bounds_off,
 *   tables + kk_off, ksize, axis, n_out, other, C, src_row_stride, base0, step0, base1, step1); axis and C (1..4, else -4) are
 *   common to the launch, everything else differs per job.  n <= GWD_AUGMENT_BATCH.
 * gwd_gather2d_batch: job i = gwd_gather2d(src, dst, tables + ytab_off, tables + xtab_off, oh, ow, src_row_stride_bytes,
 *   elem_bytes) with the element width (1..4, else -4) per job; for 2- and 4-byte elements src, dst and the row stride are
 *   multiples of the width.  n <= GWD_GATHER_BATCH (RGB, depth and labels of GWD_AUGMENT_BATCH frames).              */
#define GWD_AUGMENT_BATCH 16
#define GWD_GATHER_BATCH 48
typedef struct {
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_row_stride;
    int32_t bounds_off, kk_off, ksize, n_out, other, base0, step0, base1, step1;
    int32_t block0, blocks;   /* library-internal */
} gwd_resample_job;
typedef struct {
    const void *src;
    void *dst;
    int64_t src_row_stride_bytes;
    int32_t ytab_off, xtab_off, oh, ow, elem_bytes;
    int32_t block0, blocks;   /* library-internal */
} gwd_gather_job;
int gwd_resample_u8_pass_batch(const gwd_resample_job *jobs, int32_t n, int32_t axis, int32_t C, const int32_t *tables,
                               int64_t table_len, void *stream);
int gwd_gather2d_batch(const gwd_gather_job *jobs, int32_t n, const int32_t *tables, int64_t table_len, void *stream);

/* One adjustment of the reference's ColorJitter (src/datasets/transforms_depth.py:551-600) on a uint8 RGB image of npix pixels,
 * bit-exact with torchvision's PIL path: mode 0 brightness, 1 contrast, 2 saturation (Pillow ImageEnhance: Image.blend with a black /
 * mean-luma / luma degenerate image, factor >= 0), 3 hue (RGB -> HSV, H + shift with uint8 wrap-around, HSV -> RGB; here `factor` is
 * the SHIFT 0..255 = uint8(hue_factor * 255) as the caller's host arithmetic casts it: int(hue_factor * 255) & 255).  scratch: 8 bytes of device memory (the contrast mean's luma sum; may be NULL for the other modes).  Data-pipeline
 * entry point: not meant for HIP-graph capture (mode 1 clears its scratch with a memset node).                                     */
int gwd_color_adjust(const uint8_t *rgb, uint8_t *out, uint64_t *scratch, int64_t npix, int32_t mode, float factor, void *stream);
/* One adjustment on each of up to GWD_AUGMENT_BATCH frames in ONE launch, IN PLACE, with the arithmetic of gwd_color_adjust
 * (mode and factor per job as there; mode -1 leaves the frame untouched).  The records travel in the kernel arguments.
 * Contrast (mode 1) reads the frame's 64-bit luma sum from sums[job index].  phase GWD_COLOR_SUMS is the companion launch that
 * ADDS the luma sum of every mode-1 job's image, as it stands, to sums[job index] (integer atomics: order-independent, so the
 * mean stays bit-exact) and touches no pixel; the caller zeroes `sums` beforehand and runs it before phase GWD_COLOR_ADJUST
 * whenever a job is a contrast.  sums may be NULL when no job is.  A phase with nothing to do launches nothing.  Data-pipeline
 * entry point like gwd_color_adjust: not meant for HIP-graph capture.                                                    */
#define GWD_COLOR_ADJUST 0
#define GWD_COLOR_SUMS 1
typedef struct {
    uint8_t *rgb;             /* [npix][3], adjusted in place            */
    int64_t npix;
    int32_t mode;             /* 0..3 as gwd_color_adjust, -1 = skip     */
    float factor;
    int32_t block0, blocks;   /* library-internal                        */
} gwd_color_job;
int gwd_color_adjust_batch(const gwd_color_job *jobs, int32_t n, uint64_t *sums, int32_t phase, void *stream);

/* Strided batched GEMM  C[b0][b1] (M x N) = alpha * A[b0][b1] (M x K) * B[b0][b1] (N x K)^T  (csrc/bmm.hip).
 * Every operand has inner stride 1; a_ld / b_ld / c_ld are the element strides of the outer matrix dimension, *_sb0 / *_sb1 those of
 * the two batch dimensions (0 broadcasts an operand over a batch dimension).  a_kmajor / b_kmajor: the operand is stored [k][row]
 * (k is the outer dimension) instead of [row][k] - with these the gradients of a product need no transposed copies.
 * c_is_f32_accumulate: C is fp32 whatever `dtype` says and the result is ADDED to it (fp32 atomics; the caller zeroes it); required
 * for splits > 1, which cuts the reduction over K into `splits` workgroups per tile (long reductions onto a small result).
 * Replaces torch.bmm of the point heads (src/models/points/points_sample.py:271-279) and, in the fp32 parity mode, the two attention
 * products of src/models/multi_head_attention.py:347-371 (exact fp32: v_mfma_f32_32x32x2_f32).                                   */
typedef struct {
    const void *a, *b;
    void *c;
    int64_t a_sb0, a_sb1, a_ld, b_sb0, b_sb1, b_ld, c_sb0, c_sb1, c_ld;
    int32_t M, N, K, nb0, nb1;
    int32_t a_kmajor, b_kmajor, c_is_f32_accumulate, splits;
    float alpha;
    int32_t dtype;        /* GWD_F32 / GWD_BF16 of a, b (and of c unless c_is_f32_accumulate) */
} gwd_bmm_desc;
int gwd_bmm(const gwd_bmm_desc *d, void *stream);

#define GWD_COLLATE_BATCH 16
typedef struct {
    const void *rgb, *depth_mm, *labels;
    int32_t h, w;
} gwd_image_job;
int gwd_collate(const gwd_image_job *jobs, int32_t n, int32_t H, int32_t W, const float *mean, const float *std,
                void *images, uint8_t *mask, float *depth, int64_t *seg, int32_t dtype, void *stream);

/* L-CNN's line NMS over the detector's queries (postprocess, evaluation/eval_post_online.py:44-91 of the reference, at tol = 0 and
 * do_clip = False), one workgroup per image (csrc/linenms.hip; the scalar geometry is csrc/linescore.h, f64, no contraction): the
 * suppressed, clipped and compacted detections of every image, in one launch, without atomics or a memset.
 *   logits [B + twin][Q][2] fp32, lines [B + twin][Q][ld] fp32 (ld 4 or 6, x before y), sizes [B][2] int32 (h, w): the lines are
 *   scaled to this size in fp32 and the threshold is t * sqrt(h^2 + w^2) of it; t (a fraction of the diagonal, >= 0) is a HOST value.
 * Candidates of image b, from its Q queries: score = softmax probability of class 0 (gwd_line_postprocess's, bit for bit); the list
 *   is cut at the first i > 0 whose ld values all equal query 0's (eval_post_online.py:127-131); with min_score a number only
 *   score > min_score enters (a NaN score never does), min_score NaN = no floor.
 *   order NULL: query order, as the reference passes them.  order [B + twin][Q] int32: place k of image b holds the query taken
 *   k-th (gwd_line_postprocess's `order` gives score descending, ties by lower index); entries outside [0, Q) are skipped.
 *   twin = B: image b + twin is the prediction for the mirrored image b; its surviving queries are candidates of image b too, mirrored
 *   back by hflip_lines' rule (end points swapped, x -> w - x in fp32 on the pixel values).  With order NULL they follow the
 *   image's own; with an order the two lists are merged by score (a NaN above every number), the image's own first on ties, equal
 *   scores of one list by place.  twin = 0: none.
 * Outputs, C = Q (twin = 0) or 2 Q rows per image, every element written; row r is the r-th kept line in candidate order:
 *   nms_lines [B][C][4] f64 = (x1, y1, x2, y2) in pixels, clipped to the part no earlier kept line covers; nms_scores [B][C] fp32;
 *   nms_ids [B][C] int32 = the query index, + Q for a query of the twin; nms_count [B] int32 = kept lines; rows from nms_count on
 *   hold zeros / 0 / -1.
 * -1 on bad arguments (a NULL other than order, ld not 4 or 6, twin not 0 or B, t negative or NaN), -2 when an image has more than
 * 1024 candidates (Q > 1024, or 2 Q > 1024 with a twin); nothing is launched then.                                            */
int gwd_line_nms(const float *logits, const float *lines, const int32_t *sizes, const int32_t *order, double t, float min_score,
                 double *nms_lines, float *nms_scores, int32_t *nms_ids, int32_t *nms_count, int32_t B, int32_t Q, int32_t ld,
                 int32_t twin, void *stream);

/* Widens up to GWD_WIDEN_BATCH planes of unsigned 16-bit values (depth in millimetres as the PNG decoder produced it, kept in a
 * sample's record: gw_depth_amd/dataset.py) to the int32 planes gwd_gather2d_batch / gwd_collate take, in ONE launch: dst[k] = src[k]
 * zero-extended (65535 stays 65535) for k < n.  `jobs` is a HOST array; the records travel in the kernel arguments (nothing is
 * uploaded, nothing must outlive the call).  src needs 2-byte alignment only, dst 4-byte (-3 otherwise); jobs with n == 0 are
 * skipped; a null pointer, n < 0 or n_jobs outside 1..GWD_WIDEN_BATCH returns -1.  No allocation, no synchronisation, no atomics.  */
#define GWD_WIDEN_BATCH 16
typedef struct {
    const uint16_t *src;
    int32_t *dst;
    int64_t n;
} gwd_widen_job;
int gwd_widen_u16_batch(const gwd_widen_job *jobs, int32_t n_jobs, void *stream);

/* Dense metrics of up to GWD_EVAL_FRAMES_BATCH frames at FRAME size, by region, in ONE launch (csrc/evalframes.hip): what
 * InferenceSession.predict_frames returns, scored against the ground truth as the data set stores it.  The arithmetic is
 * gwd_eval_accumulate's (src/engine_glassrgbd.py:249-253, src/util/metrics.py:198-218 and :37-56), pixel for pixel.
 *   depth [n_jobs][Fh][Fw] fp32, label [n_jobs][Fh][Fw] uint8: frame i sits top-left in plane i; whatever lies outside its
 *   (fh, fw) is never read as a pixel.  `jobs` is a HOST array, the records travel in the kernel arguments: gt_depth_mm = the
 *   frame's fh x fw millimetres, densely packed, gt_bytes (2: unsigned 16-bit, the plane of a sample's record; 4: int32) wide;
 *   gt_label = its fh x fw raw label bytes.  bin_edges: HOST array of n_bins + 1 ascending fp32 values, n_bins 0..8.
 * Per pixel: g = float(mm) / 1000 (IEEE), glass = raw label > 0 (src/datasets/glassrgbd_norhint.py:273,275); the prediction is
 * clamped (< min -> min, > max -> max, NaN -> min, in that order); the pixel is valid when min < g < max and then adds the ten
 * terms of GWD_EVAL_NSUM to region 0 (all), to region 1 (glass) or 2 (non-glass), and to region 3 + k when
 * bin_edges[k] <= g < bin_edges[k + 1] (at most one).  R = 3 + n_bins.  The confusion counts take every pixel of the frame whose
 * predicted label is 0 or 1: [glass * 2 + label].
 * Outputs, image record i of the call at index image_offset + i, every element of the n_jobs records written:
 *   sums [..][R][10] f64 the raw sums; measures [..][R][9] f64 in the order of gwd_eval_accumulate, NaN where the region of the
 *   image has no valid pixel; conf [..][4] int64.
 *   running [R][10] f64 IN/OUT: += the nine measures of every image whose region is not empty, in image order, and [9] += 1 for
 *   each of them (the reference's running sum would turn NaN on an empty image; here the count says how many entered);
 *   confusion [4] int64 IN/OUT.
 *   workspace: GWD_EVAL_FRAMES_WS_BYTES, 16-byte aligned; its first 128 bytes (the tickets) must be ZERO before the first call on
 *   it and are zero again after every call; calls that share a workspace must be ordered on one stream.
 * No allocation, no memset, no host synchronisation, no floating-point atomics (one integer ticket per workgroup).  A frame is
 * partitioned by fh * fw alone and folded in a fixed order: bit-reproducible, and a frame's record does not depend on its slot,
 * on the other frames, on Fh x Fw or on alignment.  16-byte / 8-byte accesses when Fw % 8 == 0, fw % 8 == 0, depth and
 * gt_depth_mm are 16-byte and label and gt_label 8-byte aligned; element-wise otherwise.  All shapes are accepted.
 * -1 on bad arguments (a null pointer, n_jobs outside 1..16, a frame larger than Fh x Fw or empty, n_bins outside 0..8, edges
 * that descend or are NaN, min_depth >= max_depth, a negative offset), -2 when gt_bytes is not 2 or 4, -3 when a gt_depth_mm is
 * not aligned to its element; nothing is launched then.                                                                        */
#define GWD_EVAL_FRAMES_BATCH 16
#define GWD_EVAL_FRAMES_MAX_BINS 8
#define GWD_EVAL_FRAMES_WS_BYTES (128 + 16 * 256 * 32 + 16 * 5 * 256 * 160)
typedef struct {
    const void *gt_depth_mm;
    const uint8_t *gt_label;
    int32_t fh, fw;
} gwd_frame_eval_job;
int gwd_eval_frames(const gwd_frame_eval_job *jobs, int32_t n_jobs, const float *depth, const uint8_t *label, int32_t Fh,
                    int32_t Fw, int32_t gt_bytes, float min_depth, float max_depth, const float *bin_edges, int32_t n_bins,
                    void *workspace, int64_t image_offset, double *sums, double *measures, int64_t *conf, double *running,
                    int64_t *confusion, void *stream);

/* Guarded optimizer step and per-tensor statistics of a flat fp32 buffer (csrc/health.hip).
 *
 * gwd_segment_stats: segment s of `x` is x[seg_begin[s] : seg_end[s]) (DEVICE int64 tables of S entries; begins are multiples of 8
 * elements, ends are arbitrary, an empty segment is legal; what lies between two segments is never read).  out[s]:
 *   sumsq     f64  sum of the squares of the FINITE elements, each square taken in fp64 (exact for an fp32 operand, never inf),
 *   absmax    f32  largest finite magnitude (0 for none),
 *   nonfinite i32  number of NaN and +-Inf elements.
 * `chunks` is a DEVICE table of n_chunks records the caller builds ONCE: every segment cut, in segment order, into pieces of at
 * most GWD_HEALTH_CHUNK elements (every piece but a segment's last a multiple of 8 long), so that no piece straddles two
 * segments; an empty segment has no piece.  One workgroup reduces one piece in a fixed order into partial[chunk]
 * (gwd_query_workspace(GWD_WS_HEALTH, {n_chunks}) bytes, fully overwritten); a second launch folds the pieces of every segment in
 * ascending chunk order.  No atomics, no memset: out is bit-identical from call to call.  16-byte loads; a piece's last
 * len % 4 elements are read one by one.  -1 on a null pointer, S < 1 or n_chunks < 0; -3 when x is not 16-byte aligned.
 *
 * gwd_health_decide (one wave): folds the S records in segment order and fills the 64-byte control block:
 *   sq = the fold of sumsq; nonfinite_total; apply = (nonfinite_total == 0); then applied += apply, skipped += !apply,
 *   streak = apply ? 0 : streak + 1; when apply, bc1 / bc2 = fp32(1 - beta^t), t = applied (after the increment), computed in
 *   fp64 and rounded once; clip_coef = min(max_norm / (fp32(sqrt(sq)) * grad_scale + 1e-6), 1) as gwd_adamw_step forms it (1
 *   when max_norm <= 0).  `loss` (DEVICE fp32, may be NULL: recorded as 0 / not finite = 0) is recorded and never decides.
 *   ring[(step - 1) % ring_len] = the step's record, step = applied + skipped (after the increments).  When the step is NOT
 *   applied, bad[s] = out[s].nonfinite for every segment (bad keeps the culprits of the last skipped step).
 *   -1 on a null pointer (loss excepted), S < 1 or ring_len < 1.
 *
 * gwd_adamw_step_guarded: gwd_adamw_step with sq, bias_corr1 and bias_corr2 read from `ctl`; stores nothing when
 * ctl->apply == 0.                                                                                                              */
#define GWD_HEALTH_CHUNK 16384
typedef struct {
    double sumsq;
    float absmax;
    int32_t nonfinite;
} gwd_segment_record;
typedef struct {
    int64_t begin;      /* first element of the piece in x */
    int32_t len;        /* 1 .. GWD_HEALTH_CHUNK */
    int32_t segment;
} gwd_health_chunk;
typedef struct {
    double sq;
    int64_t applied, skipped, streak;
    int32_t nonfinite_total, apply, loss_finite, reserved;
    float bc1, bc2, clip_coef, loss;
} gwd_health_ctl;       /* 64 bytes; all zero before the first step (applied may be seeded from a checkpoint) */
typedef struct {
    int64_t step;       /* 1-based; 0 = slot never written */
    double grad_norm;   /* sqrt(sq) * grad_scale, over the finite elements */
    float clip_coef, loss;
    int32_t apply, nonfinite_total;
} gwd_health_record;    /* 32 bytes */
int gwd_segment_stats(const float *x, const int64_t *seg_begin, const int64_t *seg_end, int32_t S, const gwd_health_chunk *chunks,
                      int32_t n_chunks, void *partial, gwd_segment_record *out, void *stream);
int gwd_health_decide(const gwd_segment_record *stats, int32_t S, const float *loss, gwd_health_ctl *ctl, gwd_health_record *ring,
                      int32_t ring_len, int32_t *bad, double beta1, double beta2, float max_norm, float grad_scale, void *stream);
int gwd_adamw_step_guarded(float *p, const float *g, float *m, float *v, void *p_bf16, const gwd_health_ctl *ctl, int64_t n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                           void *stream);

/* Weight EMA fused into the AdamW pass (csrc/ema.hip).
 *
 * gwd_adamw_step_ema: the AdamW step of gwd_adamw_step (ctl == NULL: sq, which may be NULL, bias_corr1 and bias_corr2 as there) or of
 *   gwd_adamw_step_guarded (ctl != NULL: sq, bc1 and bc2 from the control block, the three arguments ignored; nothing is stored, ema
 *   included, when ctl->apply == 0) - p, m, v and the bf16 shadow come out bit-identical to those entry points - and, in the same
 *   pass, the fp32 average of the NEW parameters:
 *       ema' = fmaf(omd, p' - ema, ema),  omd = (float)(1 - d),  d = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay
 *   with d formed in fp64 on the device and t the 1-based update number: t = ema_t (ctl == NULL) or ctl->applied - ema_t (ema_t =
 *   the applied-step count at which averaging began).  A parameter that does not move keeps its average bit for bit.
 *   Any 4-byte aligned fp32 range works; p, g, m, v and ema share their offset from a 16-byte boundary and p_bf16 sits at the same
 *   ELEMENT offset from an 8-byte boundary (slices of flat buffers at equal offsets): -3 otherwise.  One grid-stride pass covers
 *   GWD_EMA_PASS elements.  -1 on a null p, g, m, v or ema, n < 0 or ema_decay outside (0, 1); 0 at n == 0.
 *
 * gwd_ema_swap: exchanges p[i] and ema[i] in place; p_bf16 (may be NULL) becomes bf16(new p[i]) in the same pass.  Two calls restore
 *   every bit of all three buffers.  Same alignment rule and return codes.                                                       */
#define GWD_EMA_PASS 2097152
int gwd_adamw_step_ema(float *p, const float *g, float *m, float *v, void *p_bf16, float *ema, const double *sq,
                       const gwd_health_ctl *ctl, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                       float bias_corr1, float bias_corr2, float max_norm, float grad_scale, double ema_decay, int32_t ema_warmup,
                       int64_t ema_t, void *stream);
int gwd_ema_swap(float *p, float *ema, void *p_bf16, int64_t n, void *stream);

/* Glass regions on the device (csrc/regions.hip): from the frame-size results of
 * InferenceSession.predict_frames to objects.  labels [B][Fh][Fw] uint8 (1 = glass), depth_mm [B][Fh][Fw] uint16, sizes [B][2]
 * int32 (fh, fw) on the DEVICE; frame b sits top-left in plane b and a pixel outside (fh, fw) never takes part, whatever byte it
 * holds.  B <= 16, Fh, Fw <= 16384.  No host synchronisation, no memset, no floating-point atomics; no loop of any kernel waits
 * for another thread.  workspace: gwd_query_workspace(GWD_WS_REGIONS, {B, Fh, Fw, max_candidates}) bytes, 16-byte aligned, needs no
 * initialisation; calls that share it must be ordered on one stream, and gwd_region_planes takes the workspace (and B) of the
 * gwd_glass_regions call whose outputs it reads.
 *
 * gwd_glass_regions: connected components of the glass pixels of every frame, `connectivity` 4 or 8 (union-find over an int32
 *   parent plane; the representative - `anchor` - of a component is its smallest raster index y * fw + x in FRAME coordinates).
 *   Components with area >= min_area are candidates; the max_regions (<= GWD_REGION_MAX) largest are kept, ranked by (area
 *   descending, anchor ascending).  An image with more than max_candidates candidates is refused: region_count = -1, map and
 *   records 0.  A pixel counts as having depth when lo_mm <= depth_mm <= hi_mm (1 <= lo_mm <= hi_mm <= 65535).
 *     region_map   [B][Fh][Fw] uint8   0 = in no kept region (all of the plane outside the frame included), r + 1 = rank r
 *     region_count [B] int32           kept regions, or -1
 *     region_total [B] int32           components found, before min_area
 *     records      [B][max_regions][GWD_REGION_RECORD] int64, rows from region_count on 0:
 *                  area, x0, y0, x1, y1 (inclusive box), anchor, sum_x, sum_y, n_depth, sum_mm, min_mm, max_mm (the last three
 *                  over the n_depth pixels with depth; 0 when there are none).  Exact.
 * gwd_region_planes: per kept region the least-squares plane w = alpha x + beta y + gamma in inverse depth, w = 1000 / depth_mm
 *   formed in fp64 (1 / m), x, y frame pixels, over its n_depth pixels.  For a pinhole camera (fx, fy, cx, cy) the 3-D plane
 *   n . P = d maps to alpha = nx / (fx d), beta = ny / (fy d), gamma = (nz - nx cx / fx - ny cy / fy) / d, so no intrinsics are
 *   needed to fit.  planes [B][max_regions][6] fp64: alpha, beta, gamma, rms of the residual w - fit (1 / m), n_used, status;
 *   status 1 (coefficients and rms NaN): fewer than 3 pixels, or collinear pixels - decided exactly from the integer moments.
 *   Rows from region_count on are 0.  Bit-identical from call to call.
 * gwd_depth_planar: depth_planar fp32 / depth_planar_mm uint16 [B][Fh][Fw] = `depth` (fp32, may be NULL: depth_mm / 1000) and
 *   depth_mm, with every pixel of a kept region of status 0 where alpha x + beta y + gamma > 0 rewritten to
 *   clamp(1 / (alpha x + beta y + gamma), min_depth, max_depth), evaluated in fp64 and rounded once to fp32; its millimetres by
 *   gwd_dense_postprocess's conversion.  Outside the frame 0 / 0.
 * -1 on a null pointer or a size / count / range outside its limits, -2 when connectivity is not 4 or 8, -3 when a pointer is
 * not aligned to its element (the workspace: 16 bytes); nothing is launched then.                                            */
#define GWD_REGION_MAX 32
#define GWD_REGION_RECORD 12
#define GWD_REGION_CANDIDATES 8192
int gwd_glass_regions(const uint8_t *labels, const uint16_t *depth_mm, const int32_t *sizes, int32_t B, int32_t Fh, int32_t Fw,
                      int32_t max_regions, int32_t min_area, int32_t connectivity, int32_t max_candidates, int32_t lo_mm,
                      int32_t hi_mm, void *workspace, uint8_t *region_map, int32_t *region_count, int32_t *region_total,
                      int64_t *records, void *stream);
int gwd_region_planes(const uint8_t *region_map, const uint16_t *depth_mm, const int32_t *sizes, const int32_t *region_count,
                      const int64_t *records, int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions, int32_t lo_mm,
                      int32_t hi_mm, void *workspace, double *planes, void *stream);
int gwd_depth_planar(const uint8_t *region_map, const uint16_t *depth_mm, const float *depth, const int32_t *sizes,
                     const int32_t *region_count, const double *planes, int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions,
                     float min_depth, float max_depth, float *depth_planar, uint16_t *depth_planar_mm, void *stream);

/* Line profiles (csrc/lineprofile.hip, the scalar geometry is csrc/lineprobe.h): every detected line walked
 * through the dense results of the same frames, in ONE launch, one wave per line.  lines [B][C][4] fp32 (GWD_LINES_F32) or fp64
 * (GWD_LINES_F64) (x1, y1, x2, y2) frame pixels; count [B] int32: rows r < count[b] are processed (clamped to 0 .. C); order [B][C]
 * int32 or NULL: row r reads lines[b][order[b][r]] (an index outside 0 .. C-1 makes the row degenerate).  labels / depth_mm / sizes
 * as for gwd_glass_regions; region_map [B][Fh][Fw] uint8 of gwd_glass_regions or NULL; intrinsics [B][4] fp64 (fx, fy, cx, cy) and
 * line_points, both or neither.  B <= 16, Fh, Fw <= 16384, C <= GWD_PROFILE_MAX_LINES.  All arithmetic is fp64, every operation
 * rounded on its own.  With dx = x2 - x1, dy = y2 - y1, L2 = dx dx + dy dy:
 *   samples   n = the smallest integer >= 1 with n n >= L2, at most max_samples - 1 (2 <= max_samples <= GWD_PROFILE_MAX_SAMPLES);
 *             S = n + 1 samples at t = k / n.  L2 not a positive finite number: a degenerate line.
 *   probes    per sample `on` = (x1 + t dx, y1 + t dy), a = on + offset (-dy / L, dx / L), b = on - the same; a probe reads the
 *             pixel (floor x, floor y) and is in the frame iff 0 <= x < fw, 0 <= y < fh of its image.
 *   counts    [B][C][GWD_PROFILE_COUNTS] int32: S; n_in, n_glass (label 1), n_depth (lo_mm <= mm <= hi_mm) of on, a, b; region_a,
 *             region_b = the rank of region_map holding most in-frame samples of that side (ties: the lower rank), -1 for none.
 *   fits      [B][C][3][5] fp64 per probe: w0, w1 (the least-squares fit of w = 1000 / mm, affine in t, at t = 0 and 1; centred,
 *             two passes), rms of the residual (third pass), n_used, status: 0 fitted, 1 fewer than 2 samples with depth (NaN),
 *             2 degenerate line (NaN, every count 0), 3 a row from count[b] on (zeros, regions -1, kind 0).
 *   kind      [B][C] int32.  A side has glass when 1000 n_glass >= hi n_in, has none when 1000 n_glass <= lo n_in (n_in > 0,
 *             0 <= lo < hi <= 1000): 1 glass on side a only, 2 on side b only, 3 on both, 4 on neither, 0 anything else.
 *   line_points [B][C][2][3] fp64: the ends ((x - cx) / fx, (y - cy) / fy, 1) z with z = 1 / w, w = w0, w1 of the `on` fit; NaN
 *             where that fit has status != 0 (rows from count[b] on included) or w <= 0.
 * No global atomics, no memset, no floating-point atomics; bit-identical from call to call; a line's record depends on neither
 * its row nor its neighbours nor Fh x Fw.  -1 on a null pointer or a size / range outside its limits (offset in (0, 16384]),
 * -2 on another lines_dtype, C > GWD_PROFILE_MAX_LINES or max_samples outside 2 .. GWD_PROFILE_MAX_SAMPLES, -3 when a pointer is
 * not aligned to its element; nothing is launched then.                                                                       */
#define GWD_LINES_F32 0
#define GWD_LINES_F64 1
#define GWD_PROFILE_MAX_LINES 2048
#define GWD_PROFILE_MAX_SAMPLES 2048
#define GWD_PROFILE_COUNTS 12
int gwd_line_profiles(const void *lines, int32_t lines_dtype, const int32_t *count, const int32_t *order, const uint8_t *labels,
                      const uint16_t *depth_mm, const int32_t *sizes, const uint8_t *region_map, const double *intrinsics,
                      int32_t B, int32_t C, int32_t Fh, int32_t Fw, double offset, int32_t max_samples, int32_t lo_mm,
                      int32_t hi_mm, int32_t hi, int32_t lo, int32_t *counts, double *fits, int32_t *kind, double *line_points,
                      void *stream);

/* Sensor depth fusion (csrc/fusion.hip, the fit is csrc/planefit.h): the depth plane of an RGB-D camera,
 * completed behind glass.  It stands where the reference builds its ground truth - depth_interpolation/depth_interpolation.py:
 * region_depth_completion fits every labelled pane from the depth measured on its frame, fuse_region_depth writes the pane's depth
 * over the sensor's - and where a user of predict_frames would today copy three planes to the host and run scipy.ndimage filters and
 * numpy.linalg.lstsq per frame.  sensor_mm [B][Fh][Fw] uint16 millimetres, 0 = no reading, registered to the frame; labels, depth
 * (fp32), depth_mm, sizes of predict_frames; region_map, region_count, records of gwd_glass_regions for the same frames.  A value
 * is VALID when lo_mm <= mm <= hi_mm.  B <= 16, Fh, Fw <= 16384.  A pixel outside its frame never takes part, neither as a sample
 * nor as a neighbour, whatever byte it holds.  No host synchronisation, no memset, no floating-point atomics, no loop that waits
 * for another thread; bit-identical from call to call.  workspace: gwd_query_workspace(GWD_WS_FUSION, {B, Fh, Fw}) bytes, 16-byte
 * aligned, needs no initialisation; the three calls are ordered on one stream and gwd_fusion_planes takes the workspace of the
 * gwd_fusion_ring call whose ring it reads.
 *
 * gwd_fusion_ring: fusion_ring [B][Fh][Fw] uint8, 0 = none, r + 1 = rank r: a pixel inside its frame with labels != 1, a valid
 *   sensor reading, no pixel with labels == 1 within Chebyshev distance gap and a pixel of a kept region within Chebyshev distance
 *   ring (1 <= ring <= GWD_FUSION_MAX_RING, 0 <= gap < ring) gets the smallest rank among those regions.  Two separable passes: a
 *   row pass into the workspace, a column pass over that.
 *   fusion_scale [B][4] fp64: s, n, sum sensor_mm * depth_mm, sum depth_mm^2 over the n pixels inside the frame that are not glass,
 *   have no glass within gap and both values valid (exact integers below 2^64, added with integer atomics);
 *   s = (double)sum_sp / (double)sum_pp, or 1.0 when align == 0, n < min_align or sum_pp == 0.
 * gwd_fusion_planes: per kept region the plane w = alpha x + beta y + gamma in inverse depth w = 1000 / sensor_mm over its ring
 *   pixels, by gwd_region_planes' method with coordinates relative to (max(x0 - ring, 0), max(y0 - ring, 0)).  With trim > 0, a
 *   first fit of status 0 and rms1 > 0, a second fit over the samples with e * e <= (trim * rms1)^2, e = w - ((alpha1 x + beta1 y)
 *   + gamma1) in fp64 without contraction against the STORED first coefficients; its rms over those samples; otherwise the first
 *   fit stands.  fusion_planes [B][max_regions][GWD_FUSION_PLANE] fp64: alpha1, beta1, gamma1, rms1, n1, alpha, beta, gamma, rms,
 *   n_used, status, 0.  status 0 usable; 1 fewer than 3 or collinear samples in either fit (its coefficients and rms NaN); 2 fitted
 *   but n_used < min_ring or rms > max_rms (pass infinity for no limit).  Rows from region_count on are 0.
 * gwd_fusion_depth: depth_fused fp32, depth_fused_mm uint16, fused_source uint8 [B][Fh][Fw]; per pixel inside its frame the
 *   first that applies: GWD_FUSED_SENSOR - labels != 1 and a valid reading: the millimetres copied, fp32 = mm / 1000 as
 *   gwd_depth_planar forms it; GWD_FUSED_PLANE - region_map names a kept region of status 0 with den = (alpha x + beta y) + gamma
 *   > 0: clamp(1 / den, min_depth, max_depth) in fp64, rounded once to fp32, millimetres by gwd_dense_postprocess's conversion;
 *   GWD_FUSED_NETWORK - everything else: clamp((double)depth * s, min_depth, max_depth), rounded and converted alike.  Outside
 *   the frame 0 / 0 / 0.  Rows of Fw % 4 == 0 in 16-byte aligned planes move four pixels per thread.
 * -1 on a null pointer or a size / count / range outside its limits, -2 on ring, gap, trim or max_rms outside theirs, -3 when a
 * pointer is not aligned to its element (the workspace: 16 bytes); nothing is launched then.                                  */
#define GWD_FUSION_MAX_RING 32
#define GWD_FUSION_PLANE 12
#define GWD_FUSED_SENSOR 1
#define GWD_FUSED_PLANE 2
#define GWD_FUSED_NETWORK 3
int gwd_fusion_ring(const uint8_t *labels, const uint16_t *sensor_mm, const uint16_t *depth_mm, const int32_t *sizes,
                    const uint8_t *region_map, const int32_t *region_count, int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions,
                    int32_t ring, int32_t gap, int32_t lo_mm, int32_t hi_mm, int32_t align, int32_t min_align, void *workspace,
                    uint8_t *fusion_ring, double *fusion_scale, void *stream);
int gwd_fusion_planes(const uint8_t *fusion_ring, const uint16_t *sensor_mm, const int32_t *sizes, const int32_t *region_count,
                      const int64_t *records, int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions, int32_t ring, int32_t lo_mm,
                      int32_t hi_mm, double trim, int32_t min_ring, double max_rms, void *workspace, double *fusion_planes,
                      void *stream);
int gwd_fusion_depth(const uint8_t *labels, const uint16_t *sensor_mm, const float *depth, const int32_t *sizes,
                     const uint8_t *region_map, const int32_t *region_count, const double *fusion_planes, const double *fusion_scale,
                     int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions, int32_t lo_mm, int32_t hi_mm, float min_depth,
                     float max_depth, float *depth_fused, uint16_t *depth_fused_mm, uint8_t *fused_source, void *stream);

/* Rendering of predict_frames' results (csrc/render.hip, the scalar geometry is csrc/rendergeom.h): uint8 RGB
 * panels at frame size, ONE launch for all P panels of all B frames, integer arithmetic throughout; tests/render_ref.py states the
 * same in numpy and the kernel equals it bit for bit.  canvas [B][P][Fh][Fw][3] uint8, 16-byte aligned; EVERY byte of it is written
 * (a pixel outside its frame is 0 0 0): no memset.  sizes [B][2] int32 (fh, fw) on the device; frame b is fh x fw clamped to
 * 0 .. min(Fh, ext_h[b]) x 0 .. min(Fw, ext_w[b]) - ext: what every operand handed over for frame b covers, so nothing is read
 * outside an operand whatever sizes holds.  B <= 16, P <= GWD_RENDER_MAX_PANELS, Fh, Fw <= 16384.
 * Operands travel per frame: a slot holds B pointers and B row pitches (frames: bytes per row, 3 bytes per pixel; planes: elements
 * per row), so a plane may be one [B][Fh][Fw] tensor or B separate views.  planes: uint16 millimetres; label_planes and region_map:
 * uint8.  tables [n_tables][256][3] uint8 on the device: every colour table of the call (depth tables, palettes, region colours
 * indexed by rank, the score table, the 5 colours of profile_kind).
 * A panel's pixel, layer over layer:
 *   base     GWD_RENDER_BLACK; GWD_RENDER_FRAME: the frame's RGB; GWD_RENDER_DEPTH: planes[plane] through tables[table] at
 *            clamp((2 * 255 * (mm - lo_mm) + span) / (2 * span), 0, 255), span = hi_mm - lo_mm >= 1, mm == 0: void_rgb;
 *            GWD_RENDER_LABELS: label_planes[plane] through tables[table].
 *   tint     tint >= 0: where label_planes[tint] == 1, c = (c * (256 - tint_alpha) + tint_rgb * tint_alpha + 128) >> 8.
 *   outline  outlines != 0 (needs region_map): a pixel with rank r = region_map > 0 one of whose 4 neighbours lies outside the
 *            frame or holds another value takes tables[region_table][r - 1].
 *   lines    rows r < count[b] (clamped to 0 .. C) of lines [B][C][4] fp32 / fp64 (GWD_LINES_*), through order [B][C] when given
 *            (src = order[b][r], outside 0 .. C-1: not drawn); not drawn either with a non-finite coordinate or one above 32767 in
 *            magnitude, or, with scores [B][C] (fp32 / fp64, indexed by src), a score that is NaN or below min_score.  Ends are
 *            quantised to 1/16 pixel, X = floor(16 x + 0.5); pixel (ix, iy) is the point (16 ix + 8, 16 iy + 8); it is covered when it
 *            lies within width8 (= round(8 * width in pixels), 1 .. GWD_RENDER_MAX_WIDTH8) of the segment, ties inside, in exact int64
 *            arithmetic (rendergeom.h: rg_covered).  Where several rows cover a pixel the LOWEST row index wins.  GWD_RENDER_LINES_SCORE:
 *            tables[line_table] at clamp(floor((score - score_lo) * score_k), 0, 255) in fp64; GWD_RENDER_LINES_KIND:
 *            tables[line_table][kinds[b][r]] (kinds [B][C] int32 indexed by the ROW, values outside 0 .. 4 count as 0);
 *            GWD_RENDER_LINES_FIXED: line_rgb.
 *   ends     ends != 0: discs of end_radius pixels (0 .. GWD_RENDER_MAX_END_RADIUS, 0 = none) about both ends of every drawn row,
 *            the same integer test, above all lines, end_rgb.
 * width8 and end_radius hold for the whole call: coverage is decided once per pixel, the panels only choose colours.
 * One workgroup per 64 x 16 pixel tile of one frame; it bins the rows that can touch its tile into an LDS list in row order
 * (a conservative integer test), draws and continues when the list is full, and stores every panel's tile through LDS in 16-byte
 * pieces with a scalar head and tail per row.  No atomics, no workspace, no scratch; repeated calls are bit-identical; a frame's
 * panels depend on neither its slot nor its neighbours.
 * -1 on a null pointer or a size / count / range outside its limits, -2 on an enum, an index or a dtype outside its range or a
 * layer whose operand is missing, -3 when a pointer is not aligned to its element (the canvas: 16 bytes); nothing is launched then. */
#define GWD_RENDER_MAX_PANELS 8
#define GWD_RENDER_MAX_PLANES 4
#define GWD_RENDER_MAX_TABLES 16
#define GWD_RENDER_MAX_WIDTH8 128
#define GWD_RENDER_MAX_END_RADIUS 64
#define GWD_RENDER_BLACK 0
#define GWD_RENDER_FRAME 1
#define GWD_RENDER_DEPTH 2
#define GWD_RENDER_LABELS 3
#define GWD_RENDER_LINES_NONE 0
#define GWD_RENDER_LINES_SCORE 1
#define GWD_RENDER_LINES_KIND 2
#define GWD_RENDER_LINES_FIXED 3
typedef struct gwd_render_slot {
    const void *ptr[16];
    int32_t pitch[16];
} gwd_render_slot;
typedef struct gwd_render_panel {
    int32_t base, plane, table, lo_mm, hi_mm;
    int32_t tint, tint_alpha;
    int32_t outlines, region_table;
    int32_t lines, line_table, ends;
    uint8_t void_rgb[4], tint_rgb[4], line_rgb[4], end_rgb[4];       /* r, g, b, unused */
} gwd_render_panel;
typedef struct gwd_render_desc {
    uint8_t *canvas;
    const int32_t *sizes;
    const uint8_t *tables;
    const void *lines;                                    /* NULL: no lines (C = 0) */
    const int32_t *count, *order;
    const void *scores;
    const int32_t *kinds;
    double min_score, score_lo, score_k;
    int32_t B, P, Fh, Fw, C, n_planes, n_label_planes, n_tables, lines_dtype, scores_dtype, width8, end_radius, has_frames,
        has_region_map;
    int32_t ext_h[16], ext_w[16];
    gwd_render_slot frames, region_map, planes[GWD_RENDER_MAX_PLANES], label_planes[GWD_RENDER_MAX_PLANES];
    gwd_render_panel panels[GWD_RENDER_MAX_PANELS];
} gwd_render_desc;
int gwd_render_frames(const gwd_render_desc *desc, void *stream);

/* Point clouds of predict_frames' results (csrc/cloud.hip): every frame's dense depth unprojected through its
 * pinhole intrinsics, the valid points packed frame after frame in raster order; tests/cloud_ref.py states the same in numpy.
 * depth [B][Fh][Fw] fp32 metres, labels [B][Fh][Fw] uint8, sizes [B][2] int32 (fh, fw) on the DEVICE, intrinsics [B][4] fp64
 * (fx, fy, cx, cy) at frame size.  Optional (NULL: absent): region_map uint8 / region_count [B] int32 / planes [B][max_regions][6]
 * fp64 of gwd_glass_regions / gwd_region_planes (all three or none), source [B][Fh][Fw] uint8 (fused_source), poses [B][3][4] fp64
 * camera-to-world rows [R | t], frames (has_frames != 0): B uint8 RGB images, a pointer and a row pitch in bytes each, 3 bytes per
 * pixel.  ext_h / ext_w [B]: what the HOST knows frame b cannot exceed (1 .. Fh, 1 .. Fw; at most what its image covers): sizes is
 * clamped to it, so nothing is read outside an operand whatever sizes holds.  B <= 16, Fh, Fw <= 16384.
 *   candidates  pixel (x, y) of frame b with x < fw, y < fh, x % stride == 0, y % stride == 0 (1 <= stride <= GWD_CLOUD_MAX_STRIDE).
 *   a point     z = depth finite with min_depth <= z <= max_depth (compared in fp64); label != 255; keep admits the label
 *               (GWD_CLOUD_KEEP_GLASS: label == 1, GWD_CLOUD_KEEP_NON_GLASS: label != 1); with edge > 0 every lattice neighbour
 *               (+- stride in x or y, inside the frame) with such a depth zn has |zn - z| <= edge * min(zn, z) in fp64.
 *   position    X = ((x - cx) z) / fx, Y = ((y - cy) z) / fy, Z = z; with poses Pw_i = ((r_i0 X + r_i1 Y) + r_i2 Z) + t_i; fp64, one
 *               rounding per operation, one rounding to fp32.
 *   normal      (normals != 0; otherwise zeros) a pixel whose region_map value is r + 1 with r < region_count[b], planes[b][r]
 *               of status 0 and m = (alpha fx, beta fy, (gamma + alpha cx) + beta cy) of finite length > 0: -m / |m|.  Any other
 *               pixel: dx x dy of the unprojected camera positions of its 1-pixel neighbours - per axis the central difference where
 *               both neighbours lie in the frame with a depth as above, else the one-sided one that exists - normalised, negated
 *               when n . P > 0; an axis without a neighbour or a cross product of length 0: zeros.  Rotated by R with poses.
 *   record      32 bytes: fp32 x y z nx ny nz; uint8 red green blue (0 without frames), label, region (region_map or 0), source
 *               (or 0), frame (b), flags: 1 a point, 2 has a normal, 4 the normal is a pane's, 8 has colour.
 * cloud [capacity][32] uint8, 16-byte aligned: the points of frame 0 in raster order, then frame 1's, ...; cloud_offsets [B + 1]
 * int32: the exclusive prefix of the frames' counts, [B] the total; every row from the total on is written as 32 zero bytes.
 * capacity must cover the sum over b of ceil(ext_h / stride) * ceil(ext_w / stride) and be at most 2^31 - 1: -1 otherwise, the
 * kernels never truncate.  workspace: gwd_query_workspace(GWD_WS_CLOUD, {B, Fh, Fw, stride}) bytes, 16-byte aligned, needs no
 * initialisation.  Three launches: one workgroup per GWD_CLOUD_TILE candidates of one frame counts its points; one workgroup turns
 * the counts into exclusive offsets; the first grid again ranks its points by ballot and stores them, two 16-byte stores each, and
 * zeroes the tail.  No workgroup waits for another, no atomics, no memset, no host synchronisation; bit-identical from call to call;
 * a frame's rows depend on neither its slot nor its neighbours nor Fh x Fw.
 * -1 on a null pointer or a size / capacity / range outside its limits, -2 on a keep outside its enum, an incomplete region
 * triple, max_regions outside 1 .. GWD_REGION_MAX or edge NaN, -3 when a pointer is not aligned to its element (workspace and
 * cloud: 16 bytes); nothing is launched then.                                                                                 */
#define GWD_CLOUD_TILE 1024
#define GWD_CLOUD_RECORD 32
#define GWD_CLOUD_MAX_STRIDE 16
#define GWD_CLOUD_KEEP_ALL 0
#define GWD_CLOUD_KEEP_GLASS 1
#define GWD_CLOUD_KEEP_NON_GLASS 2
typedef struct gwd_cloud_desc {
    const float *depth;
    const uint8_t *labels;
    const int32_t *sizes;
    const double *intrinsics;
    const uint8_t *region_map;
    const int32_t *region_count;
    const double *planes;
    const uint8_t *source;
    const double *poses;
    void *workspace;
    uint8_t *cloud;
    int32_t *cloud_offsets;
    double min_depth, max_depth, edge;                    /* edge <= 0: no edge rule */
    int64_t capacity;
    int32_t B, Fh, Fw, max_regions, stride, normals, keep, has_frames;
    int32_t ext_h[16], ext_w[16];
    gwd_render_slot frames;
} gwd_cloud_desc;
int gwd_point_cloud(const gwd_cloud_desc *desc, void *stream);

/* Scene map (csrc/scene.hip): the clouds of gwd_point_cloud, in world coordinates (poses), merged call after
 * call into one persistent voxel grid on the device - one merged record per occupied voxel, in the order the voxels were first seen;
 * tests/scene_ref.py states the same in numpy.  The map is the caller's memory, described by gwd_scene_desc; the library keeps nothing.
 *   keys, marks [slots] uint64, ranks [slots] int32: an open-addressing table; slots a power of two, max_voxels < slots <=
 *               2 * GWD_SCENE_MAX_VOXELS.  voxels [max_voxels][GWD_SCENE_VOXEL_BYTES] bytes, 16-byte aligned: the integer accumulators
 *               of the voxel of each rank.  state [8] int64: serial (calls integrated), count (voxels), points (rows taken in),
 *               dropped (rows refused), status (0 ok, 1 overflow), three spare.  voxel: the edge in metres, finite and > 0; origin
 *               [3] finite; 1 <= max_voxels <= GWD_SCENE_MAX_VOXELS.  All of it is undefined until gwd_scene_reset has run.
 * gwd_scene_reset      one launch: an empty map, state all zero.
 * gwd_scene_integrate  cloud [rows][32] uint8 (16-byte aligned) records of gwd_point_cloud, cloud_offsets [n_offsets] int32 on the
 *                      DEVICE, n_offsets >= 2: only its last entry, the total, is read (clamped to 0 .. rows); 1 <= rows <= 2^31 - 1.
 *                      Row r < total is DROPPED (counted in `dropped`) when flag 1 is not set, x, y or z is not finite, or a voxel
 *                      index is outside -2^20 .. 2^20 - 1.  Per axis in fp64, one rounding per operation: t = (p - origin) / voxel,
 *                      i = floor(t), q = (int)floor((t - i) * 65536).  The voxel (ix, iy, iz) accumulates n += 1, sum_q += q; with
 *                      flag 2 and every |normal component| <= 2: n_normal += 1, sum_n += (int64)rint(normal * 32767); with flag 8:
 *                      n_colour += 1, sum_rgb += rgb; with label == 1: n_glass += 1; first_seen / last_seen: the serials of the
 *                      first and the last call that reached it.  Voxels are ranked by birth = (serial of the call that created
 *                      them, their smallest row of that call): A then B gives the voxels and the order of A || B in one call.  A
 *                      call that would bring count above max_voxels sets status 1 and changes nothing else; from then on the
 *                      contents are undefined until gwd_scene_reset, and calls return at once on the device.  serial advances by one
 *                      per call whatever happened (at most 2^31 - 1 calls and 2^31 - 1 observations per voxel are supported).
 *                      Five launches (claim, count, scan, rank, add); 64-bit compare-and-swap, 64-bit min and integer adds only,
 *                      so the result does not depend on scheduling; no thread waits for another, a probe visits at most `slots`
 *                      slots; nothing is read back: serial, count and status live in `state`.
 * gwd_scene_extract    cloud [max_voxels][32] uint8 and voxel_stats [max_voxels][4] int32 (n, n_glass, first_seen, last_seen), both
 *                      16-byte aligned: one row per KEPT voxel in rank order - n >= min_obs (>= 1) and keep admits its label (1 when
 *                      2 n_glass >= n, else 0; GWD_CLOUD_KEEP_*) - every row behind them zero; cloud_offsets [2] int32 = {0, kept}.
 *                      position ((i + (sum_q / n + 0.5) / 65536) * voxel) + origin per axis in fp64, in that order, one rounding
 *                      to fp32; normal sum_n / |sum_n| in fp64 (flag 2) when n_normal > 0 and the sum is not zero, else zeros; rgb
 *                      (2 sum + n_colour) / (2 n_colour) in integers (flag 8), 0 without colour; region, source, frame 0; flags
 *                      1 | GWD_SCENE_FLAG_MERGED | those.  With status != 0: all zero, cloud_offsets {0, 0}; never a truncated map.
 *                      Three launches; the map is not changed.
 * workspace: gwd_query_workspace(GWD_WS_SCENE, {rows, max_voxels}) bytes, 16-byte aligned, needs no initialisation.
 * -1 on a null pointer or a size / range outside its limits, -2 on a keep outside its enum or a voxel / origin that is NaN, infinite
 * or (voxel) not positive, -3 when a pointer is not aligned to its element (voxels, cloud, voxel_stats, workspace: 16 bytes);
 * nothing is launched then.                                                                                                   */
#define GWD_SCENE_TILE 1024
#define GWD_SCENE_VOXEL_BYTES 128
#define GWD_SCENE_MAX_VOXELS 134217728
#define GWD_SCENE_FLAG_MERGED 16
typedef struct gwd_scene_desc {
    uint64_t *keys;
    uint64_t *marks;
    int32_t *ranks;
    void *voxels;
    int64_t *state;
    double voxel;
    double origin[3];
    int64_t max_voxels, slots;
} gwd_scene_desc;
int gwd_scene_reset(const gwd_scene_desc *map, void *stream);
int gwd_scene_integrate(const gwd_scene_desc *map, const uint8_t *cloud, const int32_t *cloud_offsets, int64_t rows, int32_t n_offsets,
                        void *workspace, void *stream);
int gwd_scene_extract(const gwd_scene_desc *map, int32_t min_obs, int32_t keep, void *workspace, uint8_t *cloud, int32_t *cloud_offsets,
                      int32_t *voxel_stats, void *stream);

/* Scene view (csrc/view.hip): a cloud of 32-byte records - gwd_point_cloud's or gwd_scene_extract's - projected
 * into V <= 16 posed pinhole cameras and z-buffered; tests/view_ref.py states the same in numpy.  cloud [rows][32] uint8 (16-byte
 * aligned), cloud_offsets [n_offsets] int32 on the DEVICE, n_offsets >= 2: only its last entry, the total, is read (clamped to
 * 0 .. rows); 1 <= rows <= 2^31 - 1.  sizes [V][2] int32 (fh, fw) on the DEVICE, intrinsics [V][4] fp64 (fx, fy, cx, cy), poses
 * [V][3][4] fp64 camera-to-world rows [R | t] as gwd_point_cloud takes them (the view applies the transpose) or NULL: the cloud is in
 * the camera's frame.  ext_h / ext_w [V]: what the HOST knows view v cannot exceed (1 .. Fh, 1 .. Fw): sizes is clamped to it, so
 * nothing is written outside a plane whatever sizes holds.  Fh, Fw <= 16384.
 *   a row r < total is drawn into view v unless flag 1 is clear, a coordinate is not finite or keep (GWD_CLOUD_KEEP_*: label == 1 /
 *   label != 1) does not admit its label.  fp64, one rounding per operation: d = p - t, X = (r00 d0 + r10 d1) + r20 d2, Y and Z
 *   likewise with the second and third column; min_depth <= Z <= max_depth; u = (fx X) / Z + cx, v = (fy Y) / Z + cy;
 *   hx = max(0.5, min(max_splat / 2, ((0.5 footprint) fx) / Z)), hy with fy; the pixels ceil(u - hx) <= x <= ceil(u + hx) - 1 and
 *   the same in y, clamped in fp64 to the frame (pixel centres are integers; footprint 0: the one nearest pixel, ties to the larger
 *   coordinate); a NaN draws nothing.  A pixel keeps the smallest key float32(Z) bits << 32 | r drawn on it: the nearest point after
 *   one rounding to fp32, ties to the lowest row.
 * view_depth [V][Fh][Fw] fp32 (that float32, or 0), view_index [V][Fh][Fw] int32 (the row, or -1), both 16-byte aligned; view_labels
 * [V][Fh][Fw] uint8 (the row's label, or 255), view_rgb [V][Fh][Fw][3] uint8 (the row's colour with flag 8, else 0), both 4-byte
 * aligned: every byte is written, the pixels outside (fh, fw) hold the empty values.  workspace: gwd_query_workspace(GWD_WS_VIEW,
 * {V, Fh, Fw}) bytes - the z-buffer, 8 per pixel - 16-byte aligned, needs no initialisation.  Three launches (clear, splat, resolve):
 * one 64-bit unsigned min per covered pixel, skipped after a plain load when the stored key is smaller already; rectangles above 16
 * pixels are walked by the whole wave.  No memset, no host synchronisation, no thread waits for another; the minimum is unique, so
 * results are bit-identical from call to call.
 * -1 on a null pointer or a size / range outside its limits, -2 on a keep outside its enum, max_splat outside 1 ..
 * GWD_VIEW_MAX_SPLAT, a footprint that is NaN, negative or infinite, or depth bounds that are NaN or not 0 < min_depth <= max_depth <
 * infinity, -3 when a pointer is not aligned as above; nothing is launched then.                                               */
#define GWD_VIEW_TILE 1024
#define GWD_VIEW_MAX_SPLAT 64
typedef struct gwd_view_desc {
    const uint8_t *cloud;
    const int32_t *cloud_offsets;
    const int32_t *sizes;
    const double *intrinsics;
    const double *poses;
    void *workspace;
    float *view_depth;
    int32_t *view_index;
    uint8_t *view_labels;
    uint8_t *view_rgb;
    double min_depth, max_depth, footprint;
    int64_t rows;
    int32_t n_offsets, V, Fh, Fw, max_splat, keep;
    int32_t ext_h[16], ext_w[16];
} gwd_view_desc;
int gwd_cloud_view(const gwd_view_desc *desc, void *stream);

#ifdef __cplusplus
}
#endif
#endif

// Low-resolution tail of the PSP pyramid (PyramidLayer.lastconv[0], points_sample.py:114-125).
//
// The 3x3 convolution over [x | up(y_1) | ... | up(y_n)] is linear, and so is the align-corners bilinear resize `up`: the channel
// mixing of an up-sampled branch commutes with the resize,
//     conv3x3(up(y))(p) = sum_tap [p + tap inside the map] * up(W_tap . y)(p + tap),
// so the nine channel products W_tap . y of a branch run as ONE 1x1 convolution on its few low-resolution pixels (y -> Z, 9 N
// channels) and only a bilinear gather of Z is left at full resolution.  This file holds that gather fused with the layer's
// LayerNorm [+ GELU] (forward), its transpose (backward: gz -> the gradient G of every Z, a gather over each low-resolution pixel's
// footprint - no atomics, bit-reproducible) and the fold of the partial weight gradients into the parameter's own layout.
//
// Coordinates follow resample.hip: src = dst * (h - 1) / (H - 1) in fp32, i0 = (int)src, i1 = i0 + (i0 < h - 1), l = src - i0.
#include "common.h"

namespace {

constexpr int PT_TH = 8, PT_TW = 8;         // forward: output pixels of a workgroup (256 threads = 64 pixels x 4 channel lanes)
constexpr int PT_CH = 32;                   // channels of one pass over the tile (4 lanes x 8)
constexpr int PT_MAXCHUNK = 10;             // N <= 320
constexpr int PT_MAXR = 5, PT_MAXC = 5;     // low-resolution rows / columns of one branch under a tile and its 3x3 ring, held in LDS
constexpr int PT_MAXPOS = PT_MAXR * PT_MAXC;
constexpr int PT_TAB = 128;                  // backward: footprint rows / columns whose weights are tabulated in LDS
constexpr int PT_SPLIT = 4;                 // backward: footprint rows of one low-resolution pixel are dealt to 4 thread groups

struct PyrBranches {
    void *p[GWD_PYR_MAX_BRANCHES];          // forward: the products Z_k; backward: their gradients G_k
    int h[GWD_PYR_MAX_BRANCHES], w[GWD_PYR_MAX_BRANCHES];
    int start[GWD_PYR_MAX_BRANCHES + 1];    // backward: first workgroup of branch k
    int n;
};

__device__ __forceinline__ float pt_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// weight with which output coordinate o reads source coordinate s (of `in`), as resample.hip's tap_weight
__device__ __forceinline__ float pt_weight(int o, int s, int in, float scale) {
    const float f = scale * o;
    const int i0 = (int)f, i1 = i0 + (i0 < in - 1);
    const float l = f - i0;
    return (i0 == s ? 1.f - l : 0.f) + (i1 == s ? l : 0.f);
}

template <typename T> struct Vec8;          // 8 channels in the storage type
template <> struct alignas(16) Vec8<__bf16> { __bf16 e[8]; };
template <> struct alignas(16) Vec8<float> { float e[8]; };

template <typename T> struct Raw8;         // the same 8 channels as plain registers (a prefetched value on its way to LDS)
template <> struct Raw8<__bf16> { uint4 a; };
template <> struct Raw8<float> { uint4 a, b; };

template <typename T>
__device__ __forceinline__ void fma8(float (&acc)[8], float wgt, const Vec8<T> &v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, to_f32(v.e[e]), acc[e]);
}

// z = part + sum_k sum_tap [p + tap inside] bilinear(Z_k[.., tap, :])(p + tap);  y = [GELU](LayerNorm(z)), mean, rstd.
// Thread (pixel, lane q): channels 32 j + 8 q .. + 7 of every chunk j, all in registers until the LayerNorm.
// Per chunk and branch the gather is separable: the tile's window of Z goes to LDS; a horizontal stage forms, for each of its few
// low-resolution rows and each row tap ty, the column-interpolated sum over the three column taps at every pixel column of the tile
// (6 multiply-adds an element); the vertical stage interpolates those between two rows for each ty (6 more) - not the direct 36.
// Workgroups are numbered so that runs of two tile rows stay on one XCD: neighbouring tiles read the same window of Z.
template <typename T>
__global__ __launch_bounds__(256) void pyr_tail_fwd_kernel(const T *__restrict__ part, const PyrBranches br, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, T *__restrict__ z, T *__restrict__ y,
                                                           float *__restrict__ mean, float *__restrict__ rstd, int H, int W, int N, int gelu) {
    __shared__ Vec8<T> smz[PT_MAXPOS * 36];
    __shared__ Vec8<float> smh[PT_MAXR * 3 * PT_TW * 4];
    const int t = threadIdx.x, q = t & 3, pix = t >> 2;
    const int ntx = (W + PT_TW - 1) / PT_TW, nty = (H + PT_TH - 1) / PT_TH;
    const long vb = xcd_grouped_block(blockIdx.x, gridDim.x, 2 * ntx);
    const int px0 = (int)(vb % ntx) * PT_TW, py0 = (int)((vb / ntx) % nty) * PT_TH, b = (int)(vb / ((long)ntx * nty));
    const int pxl = pix & (PT_TW - 1);
    const int px = px0 + pxl, py = py0 + pix / PT_TW;
    const bool inside = px < W && py < H;
    const int nch = N / PT_CH;
    float acc[PT_MAXCHUNK][8];
#pragma unroll
    for (int j = 0; j < PT_MAXCHUNK; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    // source rows / columns the tile's 3x3 taps reach
    const int ya = max(py0 - 1, 0), yb = min(py0 + PT_TH, H - 1), xa = max(px0 - 1, 0), xb = min(px0 + PT_TW, W - 1);
    for (int k = 0; k < br.n; ++k) {
        const int h = br.h[k], w = br.w[k];
        const float sh = pt_scale(h, H), sw = pt_scale(w, W);
        const int rlo = (int)(sh * ya), rhi = min((int)(sh * yb) + 1, h - 1);
        const int clo = (int)(sw * xa), chi = min((int)(sw * xb) + 1, w - 1);
        const int nc = min(chi - clo + 1, PT_MAXC), nr = min(rhi - rlo + 1, PT_MAXR);
        const T *Zk = (const T *)br.p[k] + (size_t)b * h * w * 9 * N;
        // the thread's share of the window (the same places for every chunk); chunk j + 1 is fetched while chunk j is summed
        static_assert(PT_MAXPOS * 36 <= 4 * 256, "four window places a thread");
        const int nitem = nr * nc * 36;
        auto place = [&](int u) {
            const int i = min(t + u * 256, nitem - 1);                 // past the window: a valid place again, loaded and not stored
            const int pos = i / 36, rem = i - pos * 36;                // rem = tap * 4 + lane
            return (((rlo + pos / nc) * w + clo + pos % nc) * 9 + (rem >> 2)) * N + (rem & 3) * 8;
        };
        const int zoff0 = place(0), zoff1 = place(1), zoff2 = place(2), zoff3 = place(3);
        typedef Raw8<T> R8;
        R8 pre0 = *(const R8 *)(Zk + zoff0), pre1 = *(const R8 *)(Zk + zoff1), pre2 = *(const R8 *)(Zk + zoff2), pre3 = *(const R8 *)(Zk + zoff3);
        R8 *smr = (R8 *)smz;
#pragma unroll
        for (int j = 0; j < PT_MAXCHUNK; ++j) {
            if (j < nch) {
                if (t < nitem) smr[t] = pre0;
                if (t + 256 < nitem) smr[t + 256] = pre1;
                if (t + 512 < nitem) smr[t + 512] = pre2;
                if (t + 768 < nitem) smr[t + 768] = pre3;
                __syncthreads();
                if (j + 1 < nch) {
                    const T *Zn = Zk + (j + 1) * PT_CH;
                    pre0 = *(const R8 *)(Zn + zoff0);
                    pre1 = *(const R8 *)(Zn + zoff1);
                    pre2 = *(const R8 *)(Zn + zoff2);
                    pre3 = *(const R8 *)(Zn + zoff3);
                }
                // horizontal: item (low row rr, row tap ty, pixel column, lane)
                for (int i = t; i < nr * 3 * PT_TW * 4; i += 256) {
                    const int lane = i & 3, xl = (i >> 2) & (PT_TW - 1), rt = i / (PT_TW * 4);      // rt = rr * 3 + ty
                    const int rr = rt / 3, ty = rt - rr * 3;
                    Vec8<float> hv;
#pragma unroll
                    for (int e = 0; e < 8; ++e) hv.e[e] = 0.f;
#pragma unroll
                    for (int tx = 0; tx < 3; ++tx) {
                        const int xx = px0 + xl + tx - 1;
                        if (xx < 0 || xx >= W) continue;
                        const float fx = sw * xx;
                        const int c0 = (int)fx, c1 = c0 + (c0 < w - 1);
                        const float lx = fx - c0, hx = 1.f - lx;
                        const int tq = (ty * 3 + tx) * 4 + lane;
                        fma8<T>(hv.e, hx, smz[(rr * nc + min(c0 - clo, PT_MAXC - 1)) * 36 + tq]);
                        fma8<T>(hv.e, lx, smz[(rr * nc + min(c1 - clo, PT_MAXC - 1)) * 36 + tq]);
                    }
                    smh[i] = hv;
                }
                __syncthreads();
                // vertical: between the two low rows of every row tap
                if (inside) {
#pragma unroll
                    for (int ty = 0; ty < 3; ++ty) {
                        const int yy = py + ty - 1;
                        if (yy < 0 || yy >= H) continue;
                        const float fy = sh * yy;
                        const int r0 = (int)fy, r1 = r0 + (r0 < h - 1);
                        const float ly = fy - r0, hy = 1.f - ly;
                        fma8<float>(acc[j], hy, smh[((min(r0 - rlo, PT_MAXR - 1) * 3 + ty) * PT_TW + pxl) * 4 + q]);
                        fma8<float>(acc[j], ly, smh[((min(r1 - rlo, PT_MAXR - 1) * 3 + ty) * PT_TW + pxl) * 4 + q]);
                    }
                }
            }
        }
    }
    // ---- + part, z in the storage type (what gwd_layernorm_backward will read), two-pass LayerNorm over the pixel's N channels
    const size_t row = ((size_t)b * H + (inside ? py : 0)) * W + (inside ? px : 0);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PT_MAXCHUNK; ++j) {
        if (j < nch && inside) {
            const size_t off = row * N + j * PT_CH + q * 8;
            const Vec8<T> pv = *(const Vec8<T> *)(part + off);
            Vec8<T> zv;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                zv.e[e] = from_f32<T>(acc[j][e] + to_f32(pv.e[e]));
                acc[j][e] = to_f32(zv.e[e]);
                s += acc[j][e];
            }
            if (z) *(Vec8<T> *)(z + off) = zv;
        }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    const float mu = s / (float)N;
    float v2 = 0.f;
#pragma unroll
    for (int j = 0; j < PT_MAXCHUNK; ++j) {
        if (j < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = acc[j][e] - mu;
                v2 += d * d;
            }
        }
    }
    v2 += __shfl_xor(v2, 1, 64);
    v2 += __shfl_xor(v2, 2, 64);
    const float rs = rsqrtf(v2 / (float)N + 1e-5f);
    if (!inside) return;
    if (q == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
#pragma unroll
    for (int j = 0; j < PT_MAXCHUNK; ++j) {
        if (j < nch) {
            const int ch = j * PT_CH + q * 8;
            Vec8<T> ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float o = (acc[j][e] - mu) * rs * gamma[ch + e] + beta[ch + e];
                if (gelu) o = gelu_t<T>(o);
                ov.e[e] = from_f32<T>(o);
            }
            *(Vec8<T> *)(y + row * N + ch) = ov;
        }
    }
}

// G_k(q, tap, :) = sum_p wy(py + ty, r) wx(px + tx, c) gz(p, :), q = (r, c).  One workgroup per low-resolution pixel: N / 8 channel
// lanes x PT_SPLIT groups that take every PT_SPLIT-th row of the footprint; a row is first summed along x into three column-tap
// sums, then spread onto the three row taps; the groups' partial sums meet in LDS and are added in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void pyr_tail_bwd_kernel(const T *__restrict__ gz, const PyrBranches br, int H, int W, int N) {
    __shared__ float sm[(PT_SPLIT - 1) * 9 * (PT_MAXCHUNK * 4) * 8];
    __shared__ float tabx[PT_TAB * 3], taby[PT_TAB * 3];       // the weights of the footprint's columns / rows for the three taps
    const int lanes = N / 8, lane = threadIdx.x % lanes, grp = threadIdx.x / lanes;
    int k = 0;
    while (k + 1 < br.n && (int)blockIdx.x >= br.start[k + 1]) ++k;
    const int h = br.h[k], w = br.w[k];
    // runs of two low-resolution rows stay on one XCD: neighbouring pixels' footprints overlap by half and meet in its L2
    const int local = (int)xcd_grouped_block(blockIdx.x - br.start[k], br.start[k + 1] - br.start[k], 2 * w);
    const int c = local % w, r = (local / w) % h, b = local / (w * h);
    const float sh = pt_scale(h, H), sw = pt_scale(w, W);
    // gz rows / columns that reach (r, c) through some tap: the resize's footprint (conservative, as resample.hip) and one ring
    int ylo = 0, yhi = H - 1, xlo = 0, xhi = W - 1;
    if (sh > 0.f) {
        ylo = max(0, (int)floorf((r - 1) / sh) - 2);
        yhi = min(H - 1, (int)ceilf((r + 1) / sh) + 2);
    }
    if (sw > 0.f) {
        xlo = max(0, (int)floorf((c - 1) / sw) - 2);
        xhi = min(W - 1, (int)ceilf((c + 1) / sw) + 2);
    }
    // trim the conservative column range to the columns that carry weight: the inner loop then runs without a branch
    auto wx_of = [&](int xx, int tx) {
        const int sx = xx + tx - 1;
        return (sx >= 0 && sx < W) ? pt_weight(sx, c, w, sw) : 0.f;
    };
    while (xlo < xhi && wx_of(xlo, 0) == 0.f && wx_of(xlo, 1) == 0.f && wx_of(xlo, 2) == 0.f) ++xlo;
    while (xhi > xlo && wx_of(xhi, 0) == 0.f && wx_of(xhi, 1) == 0.f && wx_of(xhi, 2) == 0.f) --xhi;
    auto wy_of = [&](int yy, int ty) {
        const int sy = yy + ty - 1;
        return (sy >= 0 && sy < H) ? pt_weight(sy, r, h, sh) : 0.f;
    };
    // every thread of the workgroup needs the same weights: formed once (a footprint wider than the table keeps the arithmetic)
    const bool tab = xhi - xlo < PT_TAB && yhi - ylo < PT_TAB;
    if (tab) {
        for (int i = threadIdx.x; i < (xhi - xlo + 1) * 3; i += blockDim.x) tabx[i] = wx_of(xlo + i / 3, i % 3);
        for (int i = threadIdx.x; i < (yhi - ylo + 1) * 3; i += blockDim.x) taby[i] = wy_of(ylo + i / 3, i % 3);
        __syncthreads();
    }
    float acc[9][8];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
    const T *gb = gz + (size_t)b * H * W * N + lane * 8;
    for (int yy = ylo + grp; yy <= yhi; yy += PT_SPLIT) {
        float wy[3];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) wy[ty] = tab ? taby[(yy - ylo) * 3 + ty] : wy_of(yy, ty);
        if (wy[0] == 0.f && wy[1] == 0.f && wy[2] == 0.f) continue;
        float rowsum[3][8];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) rowsum[i][e] = 0.f;
#pragma unroll 4
        for (int xx = xlo; xx <= xhi; ++xx) {
            float wx[3];
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) wx[tx] = tab ? tabx[(xx - xlo) * 3 + tx] : wx_of(xx, tx);
            const Vec8<T> v = *(const Vec8<T> *)(gb + ((size_t)yy * W + xx) * N);
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) fma8<T>(rowsum[tx], wx[tx], v);
        }
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[ty * 3 + tx][e] = fmaf(wy[ty], rowsum[tx][e], acc[ty * 3 + tx][e]);
    }
    if (grp > 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[(((grp - 1) * 9 + i) * lanes + lane) * 8 + e] = acc[i][e];
    }
    __syncthreads();
    if (grp == 0) {
        T *G = (T *)br.p[k] + ((size_t)(b * h + r) * w + c) * 9 * N + lane * 8;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            Vec8<T> ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = acc[i][e];
#pragma unroll
                for (int g = 0; g < PT_SPLIT - 1; ++g) v += sm[((g * 9 + i) * lanes + lane) * 8 + e];
                ov.e[e] = from_f32<T>(v);
            }
            *(Vec8<T> *)(G + (size_t)i * N) = ov;
        }
    }
}

// dw (N, 9, (1 + nbr) C2) += the high-resolution convolution's gradient d_hi (N, 9, (1 + nbr - nlow) C2: the map itself and the
// branches that stayed at high resolution) and the low branches' product gradients d_low[k] (9 N, C2), rows tap * N + n.
struct PyrFold {
    const float *lo[GWD_PYR_MAX_BRANCHES];
};
__global__ __launch_bounds__(256) void pyr_tail_fold_kernel(const float *__restrict__ d_hi, const PyrFold lo, float *__restrict__ dw, int N,
                                                            int C2, int nbr, int nlow, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Cw = (1 + nbr) * C2, Chi = (1 + nbr - nlow) * C2;
    const int ch = (int)(i % Cw);
    const int64_t nt = i / Cw;                 // n * 9 + tap
    const int tap = (int)(nt % 9), n = (int)(nt / 9);
    const int g = ch / C2, ci = ch - g * C2;
    float v;
    if (g == 0) v = d_hi[nt * Chi + ci];
    else if (g <= nlow) v = lo.lo[g - 1][((size_t)tap * N + n) * C2 + ci];
    else v = d_hi[nt * Chi + (g - nlow) * C2 + ci];
    dw[i] += v;
}

int check_branches(const int32_t *hk, const int32_t *wk, int nb, int H, int W) {
    for (int k = 0; k < nb; ++k) {
        if (hk[k] <= 0 || wk[k] <= 0 || hk[k] > H || wk[k] > W) return -1;
    }
    return 0;
}

}  // namespace

extern "C" int gwd_pyr_tail_forward(const void *part, const void *const *Z, const int32_t *hk, const int32_t *wk, int32_t nb,
                                    const float *gamma, const float *beta, void *z, void *y, float *mean, float *rstd, int32_t B,
                                    int32_t H, int32_t W, int32_t N, int32_t gelu, int32_t dtype, void *stream) {
    if (!part || !Z || !hk || !wk || !gamma || !beta || !y || !mean || !rstd || B <= 0 || H <= 0 || W <= 0 || N <= 0) return -1;
    if (nb < 1 || nb > GWD_PYR_MAX_BRANCHES || check_branches(hk, wk, nb, H, W)) return -1;
    if (dtype != GWD_BF16 && dtype != GWD_F32) return -2;
    if (N % PT_CH || N > PT_CH * PT_MAXCHUNK) return -4;
    PyrBranches br = {};
    br.n = nb;
    for (int k = 0; k < nb; ++k) {
        if (!Z[k]) return -1;
        // low-resolution rows / columns under one tile and its ring: floor(scale * span) + 3 at the most
        const double sh = H > 1 ? (double)(hk[k] - 1) / (H - 1) : 0.0, sw = W > 1 ? (double)(wk[k] - 1) / (W - 1) : 0.0;
        int nr = (int)(sh * (PT_TH + 1) * (1.0 + 1e-6)) + 3, nc = (int)(sw * (PT_TW + 1) * (1.0 + 1e-6)) + 3;
        nr = nr < hk[k] ? nr : hk[k];
        nc = nc < wk[k] ? nc : wk[k];
        if (nr > PT_MAXR || nc > PT_MAXC) return -4;
        br.p[k] = const_cast<void *>(Z[k]);
        br.h[k] = hk[k];
        br.w[k] = wk[k];
    }
    const int64_t nblk = (int64_t)B * ((W + PT_TW - 1) / PT_TW) * ((H + PT_TH - 1) / PT_TH);
    if (nblk >= (1LL << 31)) return -7;
    const int grid = (int)nblk;
    if (dtype == GWD_BF16)
        pyr_tail_fwd_kernel<__bf16><<<grid, 256, 0, (hipStream_t)stream>>>((const __bf16 *)part, br, gamma, beta, (__bf16 *)z, (__bf16 *)y, mean,
                                                                           rstd, H, W, N, gelu);
    else
        pyr_tail_fwd_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float *)part, br, gamma, beta, (float *)z, (float *)y, mean, rstd,
                                                                          H, W, N, gelu);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_pyr_tail_backward(const void *gz, void *const *G, const int32_t *hk, const int32_t *wk, int32_t nb, int32_t B, int32_t H,
                                     int32_t W, int32_t N, int32_t dtype, void *stream) {
    if (!gz || !G || !hk || !wk || B <= 0 || H <= 0 || W <= 0 || N <= 0) return -1;
    if (nb < 1 || nb > GWD_PYR_MAX_BRANCHES || check_branches(hk, wk, nb, H, W)) return -1;
    if (dtype != GWD_BF16 && dtype != GWD_F32) return -2;
    if (N % 8 || N > PT_CH * PT_MAXCHUNK) return -4;
    PyrBranches br = {};
    br.n = nb;
    int64_t blocks = 0;
    for (int k = 0; k < nb; ++k) {
        if (!G[k]) return -1;
        br.p[k] = G[k];
        br.h[k] = hk[k];
        br.w[k] = wk[k];
        br.start[k] = (int)blocks;
        blocks += (int64_t)B * hk[k] * wk[k];
        if (blocks >= (1LL << 31)) return -7;
    }
    br.start[nb] = (int)blocks;
    const int threads = N / 8 * PT_SPLIT;
    if (dtype == GWD_BF16) pyr_tail_bwd_kernel<__bf16><<<(int)blocks, threads, 0, (hipStream_t)stream>>>((const __bf16 *)gz, br, H, W, N);
    else pyr_tail_bwd_kernel<float><<<(int)blocks, threads, 0, (hipStream_t)stream>>>((const float *)gz, br, H, W, N);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_pyr_tail_fold_wgrad(const float *d_hi, const float *const *d_low, int32_t nlow, float *dw, int32_t N, int32_t C2,
                                       int32_t nbr, void *stream) {
    if (!d_hi || !d_low || !dw || N <= 0 || C2 <= 0 || nbr < 1 || nbr > GWD_PYR_MAX_BRANCHES || nlow < 1 || nlow > nbr) return -1;
    PyrFold lo = {};
    for (int k = 0; k < nlow; ++k) {
        if (!d_low[k]) return -1;
        lo.lo[k] = d_low[k];
    }
    const int64_t total = (int64_t)N * 9 * (1 + nbr) * C2;
    if ((total + 255) / 256 >= (1LL << 31)) return -7;
    pyr_tail_fold_kernel<<<(int)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_hi, lo, dw, N, C2, nbr, nlow, total);
    GWD_CHECK_LAUNCH();
    return 0;
}

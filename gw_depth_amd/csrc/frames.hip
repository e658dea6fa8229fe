// Decoded frames resident in HBM (gw_depth_amd/dataset.py): a sample's record holds its planes as the decoder produced them - uint8
// RGB, 16-bit depth in millimetres, uint8 labels.  The augmentation and gwd_collate read RGB and labels as views of the record; depth
// they take as int32, so the depth planes of a batch (up to GWD_WIDEN_BATCH) are widened here in ONE launch.
//
// Memory-bound: 2 bytes read, 4 written per element.  A plane starts anywhere on a 2-byte boundary (4-byte for the destination): the
// elements in front of the source's first 16-byte boundary (at most 7) and behind its last one go one by one, the body as one 16-byte
// load and two 16-byte stores per lane (the stores are dword-aligned, which a global dwordx4 store accepts).  The job records travel by
// value in the kernel arguments; workgroup -> job through the block0 prefix, as in gwd_colsum_batch.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef int32_t i32x4_dw __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kThreads = 256;
constexpr int kMaxBlocksPerJob = 1024;

struct WidenBatch {
    gwd_widen_job j[GWD_WIDEN_BATCH];
    int32_t block0[GWD_WIDEN_BATCH], blocks[GWD_WIDEN_BATCH];
    int32_t n;
};

__global__ __launch_bounds__(kThreads) void widen_u16_batch_kernel(const WidenBatch b) {
    int ji = 0;
#pragma unroll 1
    for (int k = 1; k < b.n; ++k)
        if ((int)blockIdx.x >= b.block0[k]) ji = k;
    const gwd_widen_job job = b.j[ji];
    const int blk = blockIdx.x - b.block0[ji], nblk = b.blocks[ji];
    const uint16_t *__restrict__ src = job.src;
    int32_t *__restrict__ dst = job.dst;
    const int64_t n = job.n;
    // head: the elements in front of the first 16-byte boundary of src (an even byte count: src is 2-byte aligned)
    int64_t head = (int64_t)((16 - ((uintptr_t)src & 15)) & 15) >> 1;
    if (head > n) head = n;
    const int64_t nvec = (n - head) >> 3;
    const int64_t tail0 = head + (nvec << 3);
    if (blk == 0) {                                       // at most 7 + 7 single elements per job
        const int t = threadIdx.x;
        if (t < head) dst[t] = (int32_t)src[t];
        if (t >= 64 && tail0 + (t - 64) < n) dst[tail0 + (t - 64)] = (int32_t)src[tail0 + (t - 64)];
    }
    const u16x8 *__restrict__ vs = (const u16x8 *)(src + head);
    int32_t *__restrict__ vd = dst + head;
    for (int64_t v = (int64_t)blk * kThreads + threadIdx.x; v < nvec; v += (int64_t)nblk * kThreads) {
        const u16x8 x = __builtin_nontemporal_load(vs + v);
        i32x4_dw lo, hi;
        lo.x = x.s0; lo.y = x.s1; lo.z = x.s2; lo.w = x.s3;
        hi.x = x.s4; hi.y = x.s5; hi.z = x.s6; hi.w = x.s7;
        i32x4_dw *o = (i32x4_dw *)(vd + (v << 3));
        o[0] = lo;
        o[1] = hi;
    }
}

}  // namespace

extern "C" int gwd_widen_u16_batch(const gwd_widen_job *jobs, int32_t n_jobs, void *stream) {
    if (!jobs || n_jobs < 1 || n_jobs > GWD_WIDEN_BATCH) return -1;
    WidenBatch b;
    int total = 0, m = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const gwd_widen_job &j = jobs[i];
        if (!j.src || !j.dst || j.n < 0) return -1;
        if (((uintptr_t)j.src & 1) || ((uintptr_t)j.dst & 3)) return -3;
        if (j.n == 0) continue;
        int64_t nb = ((j.n >> 3) + kThreads - 1) / kThreads;
        nb = nb > kMaxBlocksPerJob ? kMaxBlocksPerJob : (nb < 1 ? 1 : nb);
        b.j[m] = j;
        b.block0[m] = total;
        b.blocks[m] = (int)nb;
        total += (int)nb;
        ++m;
    }
    if (m == 0) return 0;
    b.n = m;
    widen_u16_batch_kernel<<<total, kThreads, 0, (hipStream_t)stream>>>(b);
    GWD_CHECK_LAUNCH();
    return 0;
}

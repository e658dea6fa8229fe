// Tile compaction, the pieces cloud.hip and scene.hip share (DESIGN.md sections 28, 29): candidates are cut into tiles of ROUNDS x WAVES x 64,
// workgroup g takes tile g and thread t of it the candidates j * 64 * WAVES + t, j = 0 .. ROUNDS - 1.  A count launch leaves every tile's
// number of kept candidates (tile_sum), ONE workgroup turns the counts into exclusive offsets (scan_tiles), an emit launch evaluates
// the predicate again and ranks the kept candidates inside their tile (TileRank): a row is the tile's offset + the rank.  Offsets are
// a function of the counts alone: no workgroup waits for another and no atomic decides an order.
#pragma once
#include "common.h"

constexpr int kScanThreads = 1024;

// n, uniform in each of the WAVES waves, summed over the workgroup -> *out, stored by thread 0; part: WAVES ints of LDS.  One barrier.
template <int WAVES> __device__ __forceinline__ void tile_sum(int n, int *part, int32_t *out) {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += part[w];
        *out = t;
    }
}

// one workgroup of kScanThreads: `counts` [tiles] -> exclusive offsets in place, [tiles] the total; thread t owns `chunk` consecutive
// tiles; sums: kScanThreads ints of LDS, free again on return
__device__ __forceinline__ void scan_tiles(int32_t *counts, int tiles, int *sums) {
    const int t = threadIdx.x;
    const int chunk = (tiles + kScanThreads - 1) / kScanThreads;
    const int lo = min(t * chunk, tiles), hi = min(lo + chunk, tiles);
    int mine = 0;
    for (int k = lo; k < hi; ++k) mine += counts[k];
    sums[t] = mine;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {          // inclusive, Hillis-Steele
        const int v = t >= o ? sums[t - o] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int run = sums[t] - mine;
    for (int k = lo; k < hi; ++k) {
        const int c = counts[k];
        counts[k] = run;
        run += c;
    }
    if (t == kScanThreads - 1) counts[tiles] = sums[t];
    __syncthreads();
}

// The rank of a lane's kept candidates inside the tile.  Every lane of the workgroup calls vote(j, ...) for every round, then the
// workgroup passes ONE __syncthreads(), then a lane that keeps anything calls finish(); part: ROUNDS * WAVES ints of LDS.
template <int ROUNDS, int WAVES> struct TileRank {
    int below[ROUNDS];
    unsigned mine = 0u;

    // round j with this lane's predicate: the kept lanes below it in its wave, the wave's count to LDS
    __device__ __forceinline__ void vote(int j, bool ok, int *part) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const unsigned long long m = __ballot(ok);
        below[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (ok) mine |= 1u << j;
        if (lane == 0) part[j * WAVES + wave] = __popcll(m);
    }
    // behind the barrier: + the kept candidates of the rounds and waves ahead of this one; rank(j) is valid from here on
    __device__ __forceinline__ void finish(const int *part) {
        const int wave = threadIdx.x >> 6;
        int before = 0;
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                if (w == wave) below[j] += before;
                before += part[j * WAVES + w];
            }
        }
    }
    __device__ __forceinline__ bool any() const { return mine != 0u; }
    __device__ __forceinline__ bool keeps(int j) const { return (mine >> j & 1u) != 0u; }
    __device__ __forceinline__ int rank(int j) const { return below[j]; }
};

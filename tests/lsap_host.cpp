// Host build of gw_depth_amd/csrc/lsap.hip for tests/test_lsap_host.py: the kernel's own source, one std::thread per lane of the
// workgroup, with barriers and wave shuffles emulated - so that matrices no GPU test may feed it (NaN, +-inf) run through the very loops
// whose bounds the kernel states.  Built by the test with g++ into a shared object and called through ctypes.
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace {
struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    int n = 0, waiting = 0;
    unsigned long phase = 0;
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        const unsigned long p = phase;
        if (++waiting == n) {
            waiting = 0;
            ++phase;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return phase != p; });
        }
    }
};
Barrier g_barrier;
unsigned long long g_slot[1024];
long g_barriers_seen[1024];
struct Idx { int x; };
thread_local Idx threadIdx, blockIdx;

inline void __syncthreads() {
    ++g_barriers_seen[threadIdx.x];
    g_barrier.wait();
}
template <typename T> inline T __shfl_xor(T v, int o, int) {
    static_assert(sizeof(T) <= 8, "");
    unsigned long long bits = 0;
    std::memcpy(&bits, &v, sizeof(T));
    g_slot[threadIdx.x] = bits;
    g_barrier.wait();
    bits = g_slot[threadIdx.x ^ o];                     // o < 64: the partner is a lane of the same wave
    g_barrier.wait();
    T r;
    std::memcpy(&r, &bits, sizeof(T));
    return r;
}
using std::isfinite;
using std::min;
}  // namespace

#define GWD_LSAP_HOST 1
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(n)
#include "lsap.hip"

// one launch of lsap_kernel<NW> (waves = 1 or 4) over layers * B workgroups, one after another; returns the largest number of
// __syncthreads() any thread passed in one workgroup (a measure of the trips taken)
extern "C" long lsap_host(const float *cost, const int32_t *col_off, int32_t *out, int layers, int B, int Q, int sumT, int waves) {
    const int nt = 64 * waves;
    long worst = 0;
    for (int blk = 0; blk < layers * B; ++blk) {
        g_barrier.n = nt;
        std::fill(g_barriers_seen, g_barriers_seen + nt, 0L);
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t)
            th.emplace_back([=] {
                threadIdx.x = t;
                blockIdx.x = blk;
                if (waves == 1)
                    lsap_kernel<1>(cost, col_off, out, B, Q, sumT);
                else
                    lsap_kernel<4>(cost, col_off, out, B, Q, sumT);
            });
        for (auto &x : th) x.join();
        worst = std::max(worst, *std::max_element(g_barriers_seen, g_barriers_seen + nt));
    }
    return worst;
}

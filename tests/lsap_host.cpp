// Host build of gw_depth_amd/csrc/lsap.hip for tests/test_lsap_host.py and tests/test_criterion_witnesses.py: the kernel's own
// source, one fiber per lane of the workgroup, with barriers and wave shuffles emulated - so that matrices no GPU test may feed it
// (NaN, +-inf) run through the very loops whose bounds the kernel states, and so that its result can be compared with the sequential
// reference of tests/lsap_ref.py at every case.  Built by tests/lsap_build.py with g++ into a shared object and called through ctypes.
//
// The lanes are cooperative fibers on one OS thread (a barrier of 256 OS threads costs a scheduler round trip, and a 257 x 257 solve
// passes ten thousand of them): a lane runs until its next barrier and hands over to the next lane; when the last lane has arrived the
// first one goes on.  That is a barrier as long as every live lane meets the same sequence of barriers, which the kernel guarantees
// (its early exits are uniform over the workgroup).  A fiber is entered once through makecontext / swapcontext and switched with
// _setjmp / _longjmp afterwards (no signal-mask system call per switch); build without _FORTIFY_SOURCE, whose longjmp check refuses a
// jump to another stack.
//
// What this build witnesses is the kernel's ARITHMETIC and its TRIP COUNTS, not its synchronisation: the lanes always run in the
// order 0 .. N - 1 between two barriers, so a barrier that is missing in the source cannot show here the way it sometimes could with
// preemptive threads.  Races are a matter for the device tests, which run every case twice and compare the bits.
#include <algorithm>
#include <cmath>
#include <csetjmp>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <ucontext.h>
#include <vector>

namespace {
constexpr int MAX_LANES = 1024;
constexpr size_t STACK_BYTES = 256 * 1024;
struct Fiber {
    ucontext_t ctx;
    jmp_buf jb;
    bool started = false, done = false;
    std::vector<char> stack;
};
Fiber g_fiber[MAX_LANES];
jmp_buf g_main_jb;
ucontext_t g_main_ctx;
int g_lanes = 0, g_current = 0;
void (*g_body)() = nullptr;
unsigned long long g_slot[2][MAX_LANES];
int g_parity[MAX_LANES];
long g_barriers_seen[MAX_LANES];
struct Idx { int x; };
Idx threadIdx, blockIdx;                                  // of the running fiber; set on every switch
int g_block = 0;

void fiber_main();

// continue with lane `to` (or with the launcher when to < 0); returns when somebody switches back to the caller
void switch_to(int from, int to) {
    jmp_buf &mine = from < 0 ? g_main_jb : g_fiber[from].jb;
    if (_setjmp(mine)) return;
    if (to < 0) _longjmp(g_main_jb, 1);
    g_current = to;
    threadIdx.x = to;
    blockIdx.x = g_block;
    Fiber &f = g_fiber[to];
    if (f.started) _longjmp(f.jb, 1);
    f.started = true;
    getcontext(&f.ctx);
    f.stack.resize(STACK_BYTES);
    f.ctx.uc_stack.ss_sp = f.stack.data();
    f.ctx.uc_stack.ss_size = f.stack.size();
    f.ctx.uc_link = nullptr;
    makecontext(&f.ctx, fiber_main, 0);
    setcontext(&f.ctx);
}

int next_live(int from) {
    for (int k = 1; k <= g_lanes; ++k) {
        const int t = (from + k) % g_lanes;
        if (!g_fiber[t].done) return t;
    }
    return -1;
}

void yield() {
    const int me = g_current, to = next_live(me);
    if (to != me) switch_to(me, to);
    g_current = me;
    threadIdx.x = me;
}

void fiber_main() {
    const int me = g_current;
    g_body();
    g_fiber[me].done = true;
    switch_to(me, next_live(me));                        // never returns: a finished lane is not switched to again
}

// one workgroup of `lanes` lanes, each running body()
void run_block(int lanes, int block, void (*body)()) {
    g_lanes = lanes;
    g_block = block;
    g_body = body;
    for (int t = 0; t < lanes; ++t) {
        g_fiber[t].started = g_fiber[t].done = false;
        g_parity[t] = 0;
    }
    switch_to(-1, 0);
}

inline void __syncthreads() {
    ++g_barriers_seen[threadIdx.x];
    yield();
}
// one yield per shuffle: the slots alternate, and a lane that writes slot[p] again (two shuffles on) has passed the yield of the
// shuffle in between, by which every lane has read what it wanted from slot[p]
template <typename T> inline T __shfl_xor(T v, int o, int) {
    static_assert(sizeof(T) <= 8, "");
    unsigned long long bits = 0;
    std::memcpy(&bits, &v, sizeof(T));
    const int p = g_parity[threadIdx.x] ^= 1;
    g_slot[p][threadIdx.x] = bits;
    yield();
    bits = g_slot[p][threadIdx.x ^ o];                  // o < 64: the partner is a lane of the same wave
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

namespace {
struct Args {
    const float *cost;
    const int32_t *col_off;
    int32_t *out;
    int B, Q, sumT, waves;
} g_args;

void lane_body() {
    const Args a = g_args;
    if (a.waves == 1)
        lsap_kernel<1>(a.cost, a.col_off, a.out, a.B, a.Q, a.sumT);
    else
        lsap_kernel<4>(a.cost, a.col_off, a.out, a.B, a.Q, a.sumT);
}
}  // namespace

// one launch of lsap_kernel<NW> (waves = 1 or 4) over layers * B workgroups, one after another; returns the largest number of
// __syncthreads() any thread passed in one workgroup (a measure of the trips taken)
extern "C" long lsap_host(const float *cost, const int32_t *col_off, int32_t *out, int layers, int B, int Q, int sumT, int waves) {
    const int nt = 64 * waves;
    long worst = 0;
    g_args = Args{cost, col_off, out, B, Q, sumT, waves};
    for (int blk = 0; blk < layers * B; ++blk) {
        std::fill(g_barriers_seen, g_barriers_seen + nt, 0L);
        run_block(nt, blk, lane_body);
        worst = std::max(worst, *std::max_element(g_barriers_seen, g_barriers_seen + nt));
    }
    return worst;
}

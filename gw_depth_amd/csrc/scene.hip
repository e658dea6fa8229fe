// Scene map on the device: the posed point clouds of gwd_point_cloud merged, call after call, into one persistent voxel grid - one
// record per occupied voxel, in the order the voxels were first seen.  The semantics are tests/scene_ref.py's.
//
// The map is five caller-owned arrays (gwd_scene_desc): an open-addressing table of `slots` entries - key, mark, rank - the voxels'
// accumulators indexed by RANK (128 bytes each, integers only) and a state block of eight int64 (serial, count, points, dropped,
// status).  The library keeps nothing; every launch reads serial / count / status from the state block, so a captured replay of a call
// stays valid.
//
// gwd_scene_reset       one launch: keys and marks all ones (empty), ranks -1, accumulators and state zero.
// gwd_scene_integrate   five launches over tiles of GWD_SCENE_TILE rows of the cloud; the launch boundaries are the only ordering.
//   claim               a row's voxel key from its position (fp64, one rounding per operation); linear probing from the key's hash,
//                       a 64-bit compare-and-swap claims the first empty slot, a slot that already holds the key is joined at once;
//                       a 64-bit min (by the first lane of each run of one slot in a wave) leaves (~serial << 32 | row) of the
//                       voxel's FIRST row of this call in `mark`; the row's slot
//                       goes to the workspace (-2: dropped, -1: the probe met `slots` other keys, status is raised).
//   count               per tile: the rows that are the first row of a voxel WITHOUT a rank - its birth row - and the dropped rows.
//   scan                ONE workgroup: tile counts -> exclusive offsets; count / points / dropped / serial advance, the overflow is
//                       guarded (status 1, nothing else changes); the call's serial, its base rank and `ok` go to the workspace.
//   rank                the first grid again: a birth row's rank = base + the births before it (ballot + population count), written
//                       to its slot; the voxel's key and first_seen to its accumulators.
//   add                 the rows of one voxel that lie next to each other in a wave (a raster-ordered cloud is made of such runs) are
//                       summed by shuffles, the run's first lane adds the sums to the accumulators of the voxel's rank with integer
//                       atomic adds; the voxel's first row of the call writes last_seen.
// gwd_scene_extract     three launches over tiles of ranks, cloud.hip's shape: count the kept voxels, scan, emit the record (two
//                       16-byte stores) and the statistics (one) and zero both tails.
// Only integer atomics take part - compare-and-swap, min, add - so the accumulators do not depend on the order of arrival, and a
// voxel's rank is a function of (serial, row) alone, not of the slot its key landed in: results are bit-identical from run to run.  No
// thread waits for another: a probe visits at most `slots` slots, accumulators start as zeros so a joined slot needs no
// initialisation, and there is no "being initialised" state.
#include "compact.h"

// tests/scene_ref.py rounds after every operation; hipcc would contract a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRounds = GWD_SCENE_TILE / kThreads;
constexpr int kResetBlocks = 2048;
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kBias = 1 << 20;                            // a voxel index is -2^20 .. 2^20 - 1
constexpr int kDropped = -2, kNoSlot = -1;
static_assert(GWD_SCENE_TILE % kThreads == 0, "a tile is whole rounds of the workgroup");

// the accumulators of one voxel: one 128-byte line
struct Voxel {
    unsigned long long key;
    unsigned long long n_glass;                           // n | n_glass << 32
    unsigned long long normal_colour;                     // n_normal | n_colour << 32
    long long sum_q[3], sum_n[3];
    unsigned long long sum_rgb[3];
    int32_t first_seen, last_seen;
    unsigned long long pad[3];
};
static_assert(sizeof(Voxel) == GWD_SCENE_VOXEL_BYTES, "gwd_scene_desc.voxels");

enum { kSerial = 0, kCount = 1, kPoints = 2, kDroppedRows = 3, kStatus = 4 };      // the state block

struct SceneArgs {
    unsigned long long *keys, *marks;
    int32_t *ranks;
    Voxel *voxels;
    long long *state;
    const uint4 *cloud_in;
    const int32_t *total_in;                              // &cloud_offsets[n_offsets - 1]
    int32_t *slot_of, *births, *drops;                    // workspace: [rows], [tiles + 1], [tiles]
    long long *call;                                      // workspace: serial, base rank, ok
    uint4 *cloud_out;
    int32_t *offsets_out;
    int4 *stats_out;
    double voxel, origin[3];
    int64_t max_voxels, slots, rows;
    int32_t tiles, shift, min_obs, keep;
};

__device__ __forceinline__ int64_t total_rows(const SceneArgs &a) { return min((int64_t)max(*a.total_in, 0), a.rows); }

// the voxel of a point: index and sub-voxel offset in 1/65536 per axis; false: the row is dropped
__device__ __forceinline__ bool quantise(const SceneArgs &a, const uint4 &r0, const uint4 &r1, unsigned long long &key, int (&q)[3]) {
    if (!(r1.w >> 24 & 1u)) return false;
    const float p[3] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)};
    key = 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(fabsf(p[k]) <= 3.40282346638528859812e38f)) return false;      // NaN, Inf
        const double t = ((double)p[k] - a.origin[k]) / a.voxel;
        const double i = floor(t);
        if (!(i >= (double)-kBias && i < (double)kBias)) return false;
        q[k] = (int)floor((t - i) * 65536.0);
        key |= (unsigned long long)((long long)i + kBias) << (21 * k);
    }
    return true;
}

__device__ __forceinline__ unsigned long long mark_of(long long serial, int64_t row) {
    return (unsigned long long)(0xffffffffu - (unsigned)serial) << 32 | (unsigned long long)row;      // a later call's rows are smaller
}

__global__ __launch_bounds__(kThreads) void scene_reset_kernel(const SceneArgs a) {
    const int64_t step = (int64_t)gridDim.x * kThreads, at = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t s = at; s < a.slots; s += step) {
        a.keys[s] = kEmpty;
        a.marks[s] = kEmpty;
        a.ranks[s] = -1;
    }
    uint4 *v = (uint4 *)a.voxels;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t k = at; k < a.max_voxels * (GWD_SCENE_VOXEL_BYTES / 16); k += step) v[k] = zero;
    if (at < 8) a.state[at] = 0;
}

// Runs of neighbouring lanes with the same value of `id` (rows of one voxel lie next to each other in a raster-ordered cloud): whether
// this lane begins one, and the last lane of its run.  Lanes with valid = false are runs of their own.  All 64 lanes call it.
__device__ __forceinline__ bool run_head(int id, bool valid, int lane, int &run_end) {
    const int prev = __shfl_up(id, 1, 64);
    const bool prev_valid = __shfl_up((int)valid, 1, 64) != 0;
    const bool head = lane == 0 || !valid || !prev_valid || id != prev;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);      // lane 63: 2 << 63 = 0, the mask is empty
    run_end = above ? __ffsll(above) - 2 : 63;
    return head;
}

__global__ __launch_bounds__(kThreads) void scene_claim_kernel(const SceneArgs a) {
    const int64_t total = total_rows(a);
    const long long serial = a.state[kSerial];
    const bool closed = a.state[kStatus] != 0;            // overflowed before this call: nothing is claimed until reset
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        const int64_t row = (int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x;
        unsigned long long key = 0ull;
        int q[3];
        int32_t slot = kDropped;
        if (row < total && quantise(a, a.cloud_in[2 * row], a.cloud_in[2 * row + 1], key, q)) {
            slot = kNoSlot;
            int64_t s = (int64_t)((key * 0x9e3779b97f4a7c15ull) >> a.shift);
            for (int64_t step = 0; step < a.slots && !closed; ++step, s = (s + 1) & (a.slots - 1)) {
                unsigned long long seen = a.keys[s];
                if (seen == kEmpty) seen = atomicCAS(&a.keys[s], kEmpty, key);
                if (seen == kEmpty || seen == key) {
                    slot = (int32_t)s;
                    break;
                }
                // a table that another row found full: stop walking it (the call ends in status 1 either way)
                if ((step & 63) == 63 && __hip_atomic_load(&a.state[kStatus], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
            }
            if (slot < 0) atomicOr((unsigned long long *)&a.state[kStatus], 1ull);
        }
        // rows grow with the lane: the first lane of a run of one slot holds the run's smallest row, it alone takes part in the min
        int run_end;
        const bool head = run_head(slot, slot >= 0, lane, run_end);
        if (head && slot >= 0) atomicMin(&a.marks[slot], mark_of(serial, row));
        if (row < total) a.slot_of[row] = slot;
    }
}

// whether `row` is the birth row of its voxel: the voxel's first row of this call, and the voxel has no rank yet
__device__ __forceinline__ bool is_birth(const SceneArgs &a, long long serial, int64_t row, int32_t slot) {
    return slot >= 0 && a.marks[slot] == mark_of(serial, row) && a.ranks[slot] < 0;
}

__global__ __launch_bounds__(kThreads) void scene_count_kernel(const SceneArgs a) {
    __shared__ int part[2][kWaves];
    const int64_t total = total_rows(a);
    const long long serial = a.state[kSerial];
    int births = 0, drops = 0;                            // uniform in the wave
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        const int64_t row = (int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x;
        const int32_t slot = row < total ? a.slot_of[row] : kNoSlot;
        births += __popcll(__ballot(row < total && is_birth(a, serial, row, slot)));
        drops += __popcll(__ballot(row < total && slot == kDropped));
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = births;
        part[1][threadIdx.x >> 6] = drops;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += part[threadIdx.x][w];
        (threadIdx.x == 0 ? a.births : a.drops)[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kScanThreads) void scene_scan_kernel(const SceneArgs a) {
    __shared__ int sums[kScanThreads];
    const int t = threadIdx.x;
    scan_tiles(a.births, a.tiles, sums);
    long long drops = 0;
    for (int k = t; k < a.tiles; k += kScanThreads) drops += a.drops[k];
    __syncthreads();                                      // sums is free again
    sums[t] = (int)drops;                                 // at most 2^31 - 1 rows in a call
    __syncthreads();
    for (int o = kScanThreads / 2; o > 0; o >>= 1) {
        if (t < o) sums[t] += sums[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const long long serial = a.state[kSerial], count = a.state[kCount], born = a.births[a.tiles];
        const bool ok = a.state[kStatus] == 0 && count + born <= a.max_voxels;
        a.call[0] = serial;
        a.call[1] = count;
        a.call[2] = ok;
        a.state[kSerial] = serial + 1;
        if (ok) {
            a.state[kCount] = count + born;
            a.state[kPoints] += total_rows(a) - sums[0];
            a.state[kDroppedRows] += sums[0];
        } else {
            a.state[kStatus] = 1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void scene_rank_kernel(const SceneArgs a) {
    __shared__ int part[kRounds * kWaves];
    if (!a.call[2]) return;                               // uniform: overflow, the contents are undefined from here on
    const int64_t total = total_rows(a);
    const long long serial = a.call[0];
    int32_t slot[kRounds];
    TileRank<kRounds, kWaves> births;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        const int64_t row = (int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x;
        slot[j] = row < total ? a.slot_of[row] : kNoSlot;
        births.vote(j, row < total && is_birth(a, serial, row, slot[j]), part);
    }
    __syncthreads();
    if (!births.any()) return;
    const long long base = a.call[1] + a.births[blockIdx.x];
    births.finish(part);
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        const long long rank = base + births.rank(j);
        if (births.keeps(j) && rank < a.max_voxels) {     // the scan has checked count + born <= max_voxels: always true
            a.ranks[slot[j]] = (int32_t)rank;             // only this row reads or writes the rank of its slot in this launch
            a.voxels[rank].key = a.keys[slot[j]];
            a.voxels[rank].first_seen = (int32_t)serial;
        }
    }
}

// sum over the lanes from this one to the end of its run (a suffix scan by doubling): the run's first lane ends with the run's sum
template <typename T> __device__ __forceinline__ T run_sum(T v, int lane, int run_end) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_down(v, d, 64);
        if (lane + d <= run_end) v += o;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void scene_add_kernel(const SceneArgs a) {
    if (!a.call[2]) return;
    const int64_t total = total_rows(a);
    const long long serial = a.call[0];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        const int64_t row = (int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x;
        const int32_t slot = row < total ? a.slot_of[row] : kNoSlot;
        int32_t rank = slot >= 0 ? a.ranks[slot] : -1;
        if (rank >= a.max_voxels) rank = -1;              // never: every claimed slot has its rank by now
        const bool valid = rank >= 0;
        // what this row adds, in 32 bits: a wave's 64 rows cannot overflow them (65535 * 64 < 2^23)
        unsigned counts = 0u, sq[3] = {0u, 0u, 0u}, red_green = 0u, blue = 0u;      // counts: n, n_glass, n_normal, n_colour, 8 bits each
        int sn[3] = {0, 0, 0};
        if (valid) {
            const uint4 r0 = a.cloud_in[2 * row], r1 = a.cloud_in[2 * row + 1];
            unsigned long long key;
            int q[3];
            quantise(a, r0, r1, key, q);
            const unsigned flags = r1.w >> 24, label = r1.z >> 24;
            const float n[3] = {__uint_as_float(r0.w), __uint_as_float(r1.x), __uint_as_float(r1.y)};
            // |component| <= 2 bounds a sum (a unit normal's are <= 1 up to rounding); NaN fails the comparison
            const bool normal = (flags & 2u) && fabsf(n[0]) <= 2.0f && fabsf(n[1]) <= 2.0f && fabsf(n[2]) <= 2.0f;
            const bool colour = (flags & 8u) != 0u;
            counts = 1u | (unsigned)(label == 1u) << 8 | (unsigned)normal << 16 | (unsigned)colour << 24;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sq[k] = (unsigned)q[k];
                if (normal) sn[k] = (int)rint((double)n[k] * 32767.0);
            }
            if (colour) {
                red_green = (r1.z & 255u) | (r1.z >> 8 & 255u) << 16;
                blue = r1.z >> 16 & 255u;
            }
        }
        // the rows of one voxel that lie next to each other in the wave are summed first: their first lane adds for all of them
        int run_end;
        const bool head = run_head(rank, valid, lane, run_end);
        counts = run_sum(counts, lane, run_end);
        red_green = run_sum(red_green, lane, run_end);
        blue = run_sum(blue, lane, run_end);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sq[k] = run_sum(sq[k], lane, run_end);
            sn[k] = run_sum(sn[k], lane, run_end);
        }
        if (!head || !valid) continue;
        Voxel &v = a.voxels[rank];
        const unsigned long long n_normal = counts >> 16 & 255u, n_colour = counts >> 24;
        atomicAdd(&v.n_glass, (unsigned long long)(counts & 255u) | (unsigned long long)(counts >> 8 & 255u) << 32);
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd((unsigned long long *)&v.sum_q[k], (unsigned long long)sq[k]);
        if (n_normal | n_colour) atomicAdd(&v.normal_colour, n_normal | n_colour << 32);
        if (n_normal) {
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd((unsigned long long *)&v.sum_n[k], (unsigned long long)(long long)sn[k]);
        }
        if (n_colour) {
            atomicAdd(&v.sum_rgb[0], (unsigned long long)(red_green & 0xffffu));
            atomicAdd(&v.sum_rgb[1], (unsigned long long)(red_green >> 16));
            atomicAdd(&v.sum_rgb[2], (unsigned long long)blue);
        }
        // the voxel's first row of the call begins a run; an atomic as every other access to this line in this launch (serials only
        // grow: max = store)
        if (a.marks[slot] == mark_of(serial, row)) atomicMax(&v.last_seen, (int32_t)serial);
    }
}

// ---- extract
__device__ __forceinline__ bool kept(const SceneArgs &a, int64_t rank, long long count) {
    if (rank >= count) return false;
    const unsigned long long c = a.voxels[rank].n_glass;
    const long long n = (long long)(c & 0xffffffffull), glass = (long long)(c >> 32);
    if (n < a.min_obs) return false;
    const bool is_glass = 2 * glass >= n;
    return a.keep == GWD_CLOUD_KEEP_ALL || (a.keep == GWD_CLOUD_KEEP_GLASS) == is_glass;
}

__device__ __forceinline__ long long live_count(const SceneArgs &a) {
    return a.state[kStatus] != 0 ? 0 : min(max(a.state[kCount], 0ll), (long long)a.max_voxels);      // overflowed: an empty cloud
}

__global__ __launch_bounds__(kThreads) void scene_keep_kernel(const SceneArgs a) {
    __shared__ int part[kWaves];
    const long long count = live_count(a);
    int n = 0;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) n += __popcll(__ballot(kept(a, (int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x, count)));
    tile_sum<kWaves>(n, part, &a.births[blockIdx.x]);
}

__global__ __launch_bounds__(kScanThreads) void scene_keep_scan_kernel(const SceneArgs a) {
    __shared__ int sums[kScanThreads];
    scan_tiles(a.births, a.tiles, sums);
    if (threadIdx.x < 2) a.offsets_out[threadIdx.x] = threadIdx.x ? a.births[a.tiles] : 0;
}

__device__ __forceinline__ void merged_record(const SceneArgs &a, const Voxel &v, uint4 &r0, uint4 &r1, int4 &st) {
    const long long n = (long long)(v.n_glass & 0xffffffffull), glass = (long long)(v.n_glass >> 32);
    const long long n_normal = (long long)(v.normal_colour & 0xffffffffull), n_colour = (long long)(v.normal_colour >> 32);
    float p[3], nrm[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double i = (double)((long long)(v.key >> (21 * k) & 0x1fffffull) - kBias);
        p[k] = (float)(((i + ((double)v.sum_q[k] / (double)n + 0.5) / 65536.0) * a.voxel) + a.origin[k]);
    }
    unsigned flags = 1u | GWD_SCENE_FLAG_MERGED;
    if (n_normal > 0 && (v.sum_n[0] | v.sum_n[1] | v.sum_n[2]) != 0) {
        const double s[3] = {(double)v.sum_n[0], (double)v.sum_n[1], (double)v.sum_n[2]};
        const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = (float)(s[k] / len);
        flags |= 2u;
    }
    unsigned rgb = 0u;
    if (n_colour > 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb |= (unsigned)((2ull * v.sum_rgb[k] + (unsigned long long)n_colour) / (2ull * (unsigned long long)n_colour)) << (8 * k);
        flags |= 8u;
    }
    const unsigned label = 2 * glass >= n ? 1u : 0u;
    r0 = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), __float_as_uint(nrm[0]));
    r1 = make_uint4(__float_as_uint(nrm[1]), __float_as_uint(nrm[2]), rgb | label << 24, flags << 24);
    st = make_int4((int)n, (int)glass, v.first_seen, v.last_seen);
}

__global__ __launch_bounds__(kThreads) void scene_emit_kernel(const SceneArgs a) {
    __shared__ int part[kRounds * kWaves];
    const long long count = live_count(a);
    TileRank<kRounds, kWaves> voxels;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) voxels.vote(j, kept(a, (int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x, count), part);
    __syncthreads();
    if (voxels.any()) {
        const int64_t base = a.births[blockIdx.x];
        voxels.finish(part);
#pragma unroll
        for (int j = 0; j < kRounds; ++j) {
            const int64_t row = base + voxels.rank(j);
            if (voxels.keeps(j) && row < a.max_voxels) {
                uint4 r0, r1;
                int4 st;
                merged_record(a, a.voxels[(int64_t)blockIdx.x * GWD_SCENE_TILE + j * kThreads + threadIdx.x], r0, r1, st);
                a.cloud_out[2 * row] = r0;
                a.cloud_out[2 * row + 1] = r1;
                a.stats_out[row] = st;
            }
        }
    }
    // the rows behind the last kept voxel: zeros, shared out over the whole grid
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t row = (int64_t)a.births[a.tiles] + (int64_t)blockIdx.x * kThreads + threadIdx.x; row < a.max_voxels;
         row += (int64_t)gridDim.x * kThreads) {
        a.cloud_out[2 * row] = zero;
        a.cloud_out[2 * row + 1] = zero;
        a.stats_out[row] = make_int4(0, 0, 0, 0);
    }
}

int64_t tiles_of(int64_t n) { return (n + GWD_SCENE_TILE - 1) / GWD_SCENE_TILE; }
int64_t pad16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// the map's own checks, shared by the three calls; 0 or the status to return
int check_map(const gwd_scene_desc *m, SceneArgs &a) {
    if (!m || !m->keys || !m->marks || !m->ranks || !m->voxels || !m->state) return -1;
    if (m->max_voxels < 1 || m->max_voxels > GWD_SCENE_MAX_VOXELS || m->slots <= m->max_voxels || m->slots > 2 * GWD_SCENE_MAX_VOXELS ||
        (m->slots & (m->slots - 1)))
        return -1;
    if (!(m->voxel > 0.0) || !(m->voxel < 1e300)) return -2;                     // NaN, zero, negative, Inf
    for (int k = 0; k < 3; ++k)
        if (!(m->origin[k] > -1e300 && m->origin[k] < 1e300)) return -2;
    if (((uintptr_t)m->keys & 7) || ((uintptr_t)m->marks & 7) || ((uintptr_t)m->ranks & 3) || ((uintptr_t)m->voxels & 15) ||
        ((uintptr_t)m->state & 7))
        return -3;
    a.keys = (unsigned long long *)m->keys; a.marks = (unsigned long long *)m->marks; a.ranks = m->ranks;
    a.voxels = (Voxel *)m->voxels; a.state = (long long *)m->state;
    a.voxel = m->voxel;
    for (int k = 0; k < 3; ++k) a.origin[k] = m->origin[k];
    a.max_voxels = m->max_voxels; a.slots = m->slots;
    int bits = 0;
    while ((1ll << bits) < m->slots) ++bits;
    a.shift = 64 - bits;                                  // slots >= 2: 1 <= bits <= 28
    a.cloud_in = nullptr; a.total_in = nullptr; a.slot_of = a.births = a.drops = nullptr; a.call = nullptr;
    a.cloud_out = nullptr; a.offsets_out = nullptr; a.stats_out = nullptr;
    a.rows = 0; a.tiles = 0; a.min_obs = 1; a.keep = GWD_CLOUD_KEEP_ALL;
    return 0;
}

}  // namespace

// bytes of gwd_query_workspace(GWD_WS_SCENE, {rows, max_voxels}) (optim.hip): what integrate needs for `rows` rows or extract for
// max_voxels voxels, whichever is more
int64_t gwd_scene_workspace_bytes(int64_t rows, int64_t max_voxels) {
    if (rows < 1 || rows > 2147483647LL || max_voxels < 1 || max_voxels > GWD_SCENE_MAX_VOXELS) return -1;
    const int64_t t = tiles_of(rows);
    const int64_t integrate = 16 * 2 + pad16(rows * 4) + pad16((t + 1) * 4) + pad16(t * 4);
    const int64_t extract = pad16((tiles_of(max_voxels) + 1) * 4);
    return integrate > extract ? integrate : extract;
}

extern "C" int gwd_scene_reset(const gwd_scene_desc *map, void *stream) {
    SceneArgs a;
    if (const int rc = check_map(map, a)) return rc;
    scene_reset_kernel<<<kResetBlocks, kThreads, 0, (hipStream_t)stream>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_scene_integrate(const gwd_scene_desc *map, const uint8_t *cloud, const int32_t *cloud_offsets, int64_t rows,
                                   int32_t n_offsets, void *workspace, void *stream) {
    SceneArgs a;
    if (const int rc = check_map(map, a)) return rc;
    if (!cloud || !cloud_offsets || !workspace || rows < 1 || rows > 2147483647LL || n_offsets < 2) return -1;
    if (((uintptr_t)cloud & 15) || ((uintptr_t)cloud_offsets & 3) || ((uintptr_t)workspace & 15)) return -3;
    a.cloud_in = (const uint4 *)cloud;
    a.total_in = cloud_offsets + (n_offsets - 1);
    a.rows = rows;
    a.tiles = (int32_t)tiles_of(rows);
    char *ws = (char *)workspace;
    a.call = (long long *)ws;
    a.slot_of = (int32_t *)(ws + 32);
    a.births = (int32_t *)(ws + 32 + pad16(rows * 4));
    a.drops = (int32_t *)(ws + 32 + pad16(rows * 4) + pad16((a.tiles + 1) * 4));
    const hipStream_t s = (hipStream_t)stream;
    scene_claim_kernel<<<(unsigned)a.tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    scene_count_kernel<<<(unsigned)a.tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    scene_scan_kernel<<<1, kScanThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    scene_rank_kernel<<<(unsigned)a.tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    scene_add_kernel<<<(unsigned)a.tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_scene_extract(const gwd_scene_desc *map, int32_t min_obs, int32_t keep, void *workspace, uint8_t *cloud,
                                 int32_t *cloud_offsets, int32_t *voxel_stats, void *stream) {
    SceneArgs a;
    if (const int rc = check_map(map, a)) return rc;
    if (!workspace || !cloud || !cloud_offsets || !voxel_stats || min_obs < 1) return -1;
    if (keep != GWD_CLOUD_KEEP_ALL && keep != GWD_CLOUD_KEEP_GLASS && keep != GWD_CLOUD_KEEP_NON_GLASS) return -2;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)cloud & 15) || ((uintptr_t)cloud_offsets & 3) || ((uintptr_t)voxel_stats & 15)) return -3;
    a.tiles = (int32_t)tiles_of(a.max_voxels);
    a.births = (int32_t *)workspace;
    a.cloud_out = (uint4 *)cloud; a.offsets_out = cloud_offsets; a.stats_out = (int4 *)voxel_stats;
    a.min_obs = min_obs; a.keep = keep;
    const hipStream_t s = (hipStream_t)stream;
    scene_keep_kernel<<<(unsigned)a.tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    scene_keep_scan_kernel<<<1, kScanThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    scene_emit_kernel<<<(unsigned)a.tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

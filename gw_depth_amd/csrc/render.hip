// Rendering of predict_frames' results on the device: uint8 RGB panels at frame size (base: black / the frame / a depth plane through
// a table / a label plane through a palette; glass tint; region outlines; lines; end markers), all P panels of all B frames in ONE
// launch, integer arithmetic throughout.  The semantics are tests/render_ref.py's; the scalar geometry is
// csrc/rendergeom.h, which a CPU test also compiles.
//
// gwd_render_frames     One workgroup of four waves per 64 x 16 pixel tile of one frame (grid: tiles x B); lane l of wave w owns the
//                       pixels (x0 + l, y0 + w + 4 k), k = 0 .. 3, so every plane read of a wave is 64 consecutive elements.
//   binning             the rows of the frame go past the tile 256 at a time, one per thread: quantised, tested against the tile by
//                       rg_tile_may_touch (conservative: it may keep a row that covers nothing here, never drop one that does) and
//                       compacted IN ROW ORDER into an LDS list through ballot and prefix count.  The list holds kList rows; when a
//                       chunk's hits do not fit behind what it holds, the tile draws what it has and starts the list again, so any
//                       C and any number of rows through one tile stay correct.
//   draw                every pixel walks the list once for all panels: the first row that covers it (the lowest index: the list is
//                       in row order and so are the chunks) and whether an end disc does.  Exact int64 tests, no square root.
//   panels              per panel the tile's colours go to an LDS stage whose rows sit at the canvas row's own offset from a
//                       16-byte boundary, and leave it in 16-byte stores; the partial pieces at either end of a tile's row (a row is
//                       3 Fw bytes: every alignment occurs) are byte stores by one lane each.  Every byte of the canvas is written.
// No atomics, no workspace, no floating point beyond the quantisation of the ends and the two fp64 operations of the score index.
#include "common.h"
#include "rendergeom.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kList = 256;                                // rows the LDS list holds = rows per binning chunk: a chunk always fits an empty list
constexpr int kStageRow = 3 * kTileW + 16;                // a tile row of the stage: 192 bytes at an offset of 0 .. 15
constexpr int kMaxB = 16;
static_assert(kStageRow % 16 == 0 && kThreads == kTileH * 16 && kThreads == 4 * kTileW, "tile geometry");

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

struct Rgb {
    int r, g, b;
};

__device__ __forceinline__ Rgb table_at(const uint8_t *__restrict__ tables, int table, int idx) {
    const uint8_t *t = tables + ((int64_t)table * 256 + idx) * 3;
    return Rgb{t[0], t[1], t[2]};
}
__device__ __forceinline__ Rgb rgb_of(const uint8_t c[4]) { return Rgb{c[0], c[1], c[2]}; }

__global__ __launch_bounds__(kThreads) void render_frames_kernel(const gwd_render_desc d) {
    __shared__ int32_t l_ax[kList], l_ay[kList], l_bx[kList], l_by[kList];
    __shared__ uint32_t l_meta[kList];                    // row | score index << 16 | kind << 24
    __shared__ int32_t wave_hits[4];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTileH * kStageRow];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int tiles_x = (d.Fw + kTileW - 1) / kTileW;
    const int x0 = ((int)blockIdx.x % tiles_x) * kTileW, y0 = ((int)blockIdx.x / tiles_x) * kTileH;
    const int fh = frame_side(d.sizes[2 * b], min(d.Fh, d.ext_h[b]));
    const int fw = frame_side(d.sizes[2 * b + 1], min(d.Fw, d.ext_w[b]));
    const int px = x0 + lane;
    const bool tile_live = x0 < fw && y0 < fh;            // uniform

    // ---- lines: the first covering row and the end discs of every pixel, once for all panels
    int best[4] = {-1, -1, -1, -1};
    bool dot[4] = {false, false, false, false};
    bool want_lines = false, want_ends = false;
    for (int p = 0; p < d.P; ++p) {
        want_lines |= d.panels[p].lines != GWD_RENDER_LINES_NONE;
        want_ends |= d.panels[p].ends != 0 && d.end_radius > 0;
    }
    if (d.lines && tile_live && (want_lines || want_ends)) {
        const int n = min(max(d.count[b], 0), d.C);
        const int tx1 = min(x0 + kTileW, fw) - 1, ty1 = min(y0 + kTileH, fh) - 1;
        const int reach = max(want_lines ? d.width8 : 0, want_ends ? 16 * d.end_radius : 0);
        const int64_t h2 = (int64_t)d.width8 * d.width8, r2 = (int64_t)(16 * d.end_radius) * (16 * d.end_radius);
        const int cx = 16 * px + 8;
        int len = 0;                                      // uniform: every thread forms it from the same LDS words

        auto draw = [&](int upto) {
            for (int e = 0; e < upto; ++e) {
                RgRow row;
                row.ax = l_ax[e], row.ay = l_ay[e], row.bx = l_bx[e], row.by = l_by[e];
                if (cx < min(row.ax, row.bx) - reach || cx > max(row.ax, row.bx) + reach) continue;
                const int meta = (int)l_meta[e];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int y = y0 + wave + 4 * k, cy = 16 * y + 8;
                    if (px >= fw || y >= fh) continue;
                    if (want_lines && best[k] < 0 && rg_covered(row, cx, cy, h2)) best[k] = meta;
                    if (want_ends && !dot[k]) dot[k] = rg_disc(row.ax, row.ay, cx, cy, r2) || rg_disc(row.bx, row.by, cx, cy, r2);
                }
            }
        };

        for (int base = 0;; base += kThreads) {           // one more turn than there are chunks: the last one only draws
            const int r = base + tid;
            bool hit = false;
            RgRow row;
            row.ax = row.ay = row.bx = row.by = 0;
            uint32_t meta = 0;
            if (r < n) {
                const int src = d.order ? d.order[(int64_t)b * d.C + r] : r;
                if (src >= 0 && src < d.C) {
                    const int64_t at = ((int64_t)b * d.C + src) * 4;
                    double v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        v[k] = d.lines_dtype == GWD_LINES_F64 ? ((const double *)d.lines)[at + k] : (double)((const float *)d.lines)[at + k];
                    bool ok = rg_quantise(v[0], v[1], v[2], v[3], row);
                    int sidx = 0, kind = 0;
                    if (d.scores) {
                        const int64_t sa = (int64_t)b * d.C + src;
                        const double s = d.scores_dtype == GWD_LINES_F64 ? ((const double *)d.scores)[sa] : (double)((const float *)d.scores)[sa];
                        ok = ok && s >= d.min_score;      // NaN fails
                        sidx = rg_score_index(s, d.score_lo, d.score_k);
                    }
                    if (d.kinds) {
                        kind = d.kinds[(int64_t)b * d.C + r];
                        kind = kind >= 0 && kind <= 4 ? kind : 0;
                    }
                    meta = (uint32_t)r | (uint32_t)sidx << 16 | (uint32_t)kind << 24;
                    hit = ok && rg_tile_may_touch(row, x0, y0, tx1, ty1, reach);
                }
            }
            const unsigned long long votes = __ballot(hit);
            const int before = __popcll(votes & ((1ull << lane) - 1ull));
            if (lane == 0) wave_hits[wave] = __popcll(votes);
            __syncthreads();
            int total = 0, ahead = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int c = wave_hits[w];
                total += c;
                ahead += w < wave ? c : 0;
            }
            const bool done = base >= n;                  // uniform, as is the test below
            if (done || len + total > kList) {            // the rows are through, or the list is full: draw what it holds, start it again
                draw(len);
                len = 0;
                if (done) break;
                __syncthreads();
            }
            if (hit) {
                const int at = len + ahead + before;      // < kList: total <= kThreads == kList
                l_ax[at] = row.ax, l_ay[at] = row.ay, l_bx[at] = row.bx, l_by[at] = row.by, l_meta[at] = meta;
            }
            len += total;
            __syncthreads();
        }
    }

    // ---- region outlines: the rank whose colour the pixel takes, or 0
    int ring[4] = {0, 0, 0, 0};
    bool want_outlines = false;
    for (int p = 0; p < d.P; ++p) want_outlines |= d.panels[p].outlines != 0;
    if (want_outlines && d.has_region_map && tile_live) {
        const uint8_t *__restrict__ M = (const uint8_t *)d.region_map.ptr[b];
        const int64_t pitch = d.region_map.pitch[b];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + wave + 4 * k;
            if (px >= fw || y >= fh) continue;
            const int r = M[y * pitch + px];
            if (r == 0) continue;
            const bool edge = px == 0 || px == fw - 1 || y == 0 || y == fh - 1 || M[y * pitch + px - 1] != r || M[y * pitch + px + 1] != r ||
                              M[(y - 1) * pitch + px] != r || M[(y + 1) * pitch + px] != r;      // || stops before a read outside the frame
            ring[k] = edge ? r : 0;
        }
    }

    // ---- the panels
    const int row_bytes = 3 * min(kTileW, d.Fw - x0);     // of this tile in a canvas row
    for (int p = 0; p < d.P; ++p) {
        const gwd_render_panel &pn = d.panels[p];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ty = wave + 4 * k, y = y0 + ty;
            if (px >= d.Fw || y >= d.Fh) continue;
            Rgb c{0, 0, 0};
            if (px < fw && y < fh) {
                if (pn.base == GWD_RENDER_FRAME) {
                    const uint8_t *f = (const uint8_t *)d.frames.ptr[b] + (int64_t)y * d.frames.pitch[b] + 3 * px;
                    c = Rgb{f[0], f[1], f[2]};
                } else if (pn.base == GWD_RENDER_DEPTH) {
                    const int mm = ((const uint16_t *)d.planes[pn.plane].ptr[b])[(int64_t)y * d.planes[pn.plane].pitch[b] + px];
                    const int span = pn.hi_mm - pn.lo_mm, num = 510 * (mm - pn.lo_mm) + span;      // |num| < 2^26
                    c = mm == 0 ? rgb_of(pn.void_rgb) : table_at(d.tables, pn.table, num < 0 ? 0 : min(num / (2 * span), 255));
                } else if (pn.base == GWD_RENDER_LABELS) {
                    c = table_at(d.tables, pn.table, ((const uint8_t *)d.label_planes[pn.plane].ptr[b])[(int64_t)y * d.label_planes[pn.plane].pitch[b] + px]);
                }
                if (pn.tint >= 0 && ((const uint8_t *)d.label_planes[pn.tint].ptr[b])[(int64_t)y * d.label_planes[pn.tint].pitch[b] + px] == 1) {
                    const int a = pn.tint_alpha;
                    c.r = (c.r * (256 - a) + pn.tint_rgb[0] * a + 128) >> 8;
                    c.g = (c.g * (256 - a) + pn.tint_rgb[1] * a + 128) >> 8;
                    c.b = (c.b * (256 - a) + pn.tint_rgb[2] * a + 128) >> 8;
                }
                if (pn.outlines && ring[k]) c = table_at(d.tables, pn.region_table, ring[k] - 1);
                if (pn.lines != GWD_RENDER_LINES_NONE && best[k] >= 0) {
                    c = pn.lines == GWD_RENDER_LINES_SCORE ? table_at(d.tables, pn.line_table, (best[k] >> 16) & 255)
                        : pn.lines == GWD_RENDER_LINES_KIND ? table_at(d.tables, pn.line_table, (best[k] >> 24) & 255)
                                                            : rgb_of(pn.line_rgb);
                }
                if (pn.ends && dot[k]) c = rgb_of(pn.end_rgb);
            }
            const int64_t g0 = ((((int64_t)b * d.P + p) * d.Fh + y) * d.Fw + x0) * 3;
            uint8_t *s = stage + ty * kStageRow + (int)(g0 & 15) + 3 * lane;
            s[0] = (uint8_t)c.r, s[1] = (uint8_t)c.g, s[2] = (uint8_t)c.b;
        }
        __syncthreads();
        {   // 16 threads per tile row: 13 aligned 16-byte pieces, the head, the tail
            const int ty = tid >> 4, slot = tid & 15, y = y0 + ty;
            if (y < d.Fh) {
                const int64_t g0 = ((((int64_t)b * d.P + p) * d.Fh + y) * d.Fw + x0) * 3, g1 = g0 + row_bytes;
                const int64_t floor0 = g0 & ~(int64_t)15;
                const int64_t first = min((g0 + 15) & ~(int64_t)15, g1), last = max(g1 & ~(int64_t)15, first);      // head [g0, first), body [first, last), tail [last, g1)
                const uint8_t *src = stage + ty * kStageRow;       // the byte of canvas offset g sits at src[g - floor0]
                if (slot < 13) {
                    const int64_t a = floor0 + 16 * slot;
                    if (a >= first && a + 16 <= last) *(u32x4 *)(d.canvas + a) = *(const u32x4 *)(src + 16 * slot);
                } else if (slot == 13) {
                    for (int64_t g = g0; g < first; ++g) d.canvas[g] = src[g - floor0];
                } else if (slot == 14) {
                    for (int64_t g = last; g < g1; ++g) d.canvas[g] = src[g - floor0];
                }
            }
        }
        __syncthreads();
    }
}

bool slot_ok(const gwd_render_slot &s, int B, int align) {
    for (int b = 0; b < B; ++b)
        if (!s.ptr[b] || s.pitch[b] < 1 || ((uintptr_t)s.ptr[b] & (align - 1))) return false;
    return true;
}
bool slot_null(const gwd_render_slot &s, int B) {
    for (int b = 0; b < B; ++b)
        if (!s.ptr[b]) return true;
    return false;
}

}  // namespace

extern "C" int gwd_render_frames(const gwd_render_desc *desc, void *stream) {
    if (!desc) return -1;
    const gwd_render_desc &d = *desc;
    if (!d.canvas || !d.sizes || !d.tables) return -1;
    if (d.B < 1 || d.B > kMaxB || d.P < 1 || d.P > GWD_RENDER_MAX_PANELS || d.Fh < 1 || d.Fw < 1 || d.Fh > 16384 || d.Fw > 16384) return -1;
    if (d.n_planes < 0 || d.n_planes > GWD_RENDER_MAX_PLANES || d.n_label_planes < 0 || d.n_label_planes > GWD_RENDER_MAX_PLANES ||
        d.n_tables < 1 || d.n_tables > GWD_RENDER_MAX_TABLES)
        return -1;
    if (d.lines) {
        if (!d.count || d.C < 1 || d.C > GWD_PROFILE_MAX_LINES) return -1;
        if (d.width8 < 1 || d.width8 > GWD_RENDER_MAX_WIDTH8 || d.end_radius < 0 || d.end_radius > GWD_RENDER_MAX_END_RADIUS) return -1;
        if (d.scores && (d.min_score != d.min_score || !(d.score_k > 0.0) || !(d.score_k < 1.7976931348623157e308) ||
                         !(d.score_lo > -1.7976931348623157e308 && d.score_lo < 1.7976931348623157e308)))
            return -1;
    } else if (d.count || d.order || d.scores || d.kinds) {
        return -1;
    }
    for (int b = 0; b < d.B; ++b)
        if (d.ext_h[b] < 0 || d.ext_w[b] < 0) return -1;
    if (d.has_frames && slot_null(d.frames, d.B)) return -1;
    if (d.has_region_map && slot_null(d.region_map, d.B)) return -1;
    for (int i = 0; i < d.n_planes; ++i)
        if (slot_null(d.planes[i], d.B)) return -1;
    for (int i = 0; i < d.n_label_planes; ++i)
        if (slot_null(d.label_planes[i], d.B)) return -1;

    if (d.lines && ((d.lines_dtype != GWD_LINES_F32 && d.lines_dtype != GWD_LINES_F64) ||
                    (d.scores && d.scores_dtype != GWD_LINES_F32 && d.scores_dtype != GWD_LINES_F64)))
        return -2;
    for (int p = 0; p < d.P; ++p) {
        const gwd_render_panel &pn = d.panels[p];
        const bool table_ok = pn.table >= 0 && pn.table < d.n_tables;
        if (pn.base < GWD_RENDER_BLACK || pn.base > GWD_RENDER_LABELS) return -2;
        if (pn.base == GWD_RENDER_FRAME && !d.has_frames) return -2;
        if (pn.base == GWD_RENDER_DEPTH && (pn.plane < 0 || pn.plane >= d.n_planes || !table_ok || pn.lo_mm < 0 || pn.hi_mm > 65535 || pn.lo_mm >= pn.hi_mm))
            return -2;
        if (pn.base == GWD_RENDER_LABELS && (pn.plane < 0 || pn.plane >= d.n_label_planes || !table_ok)) return -2;
        if (pn.tint >= d.n_label_planes || (pn.tint >= 0 && (pn.tint_alpha < 0 || pn.tint_alpha > 256))) return -2;
        if (pn.outlines && (!d.has_region_map || pn.region_table < 0 || pn.region_table >= d.n_tables)) return -2;
        if (pn.lines < GWD_RENDER_LINES_NONE || pn.lines > GWD_RENDER_LINES_FIXED) return -2;
        if ((pn.lines != GWD_RENDER_LINES_NONE || pn.ends) && !d.lines) return -2;
        if (pn.lines == GWD_RENDER_LINES_SCORE && (!d.scores || pn.line_table < 0 || pn.line_table >= d.n_tables)) return -2;
        if (pn.lines == GWD_RENDER_LINES_KIND && (!d.kinds || pn.line_table < 0 || pn.line_table >= d.n_tables)) return -2;
    }

    if (((uintptr_t)d.canvas & 15) || ((uintptr_t)d.sizes & 3) || ((uintptr_t)d.count & 3) || ((uintptr_t)d.order & 3) || ((uintptr_t)d.kinds & 3) ||
        ((uintptr_t)d.lines & (d.lines_dtype == GWD_LINES_F64 ? 7 : 3)) || ((uintptr_t)d.scores & (d.scores_dtype == GWD_LINES_F64 ? 7 : 3)))
        return -3;
    if (d.has_frames && !slot_ok(d.frames, d.B, 1)) return -3;
    if (d.has_region_map && !slot_ok(d.region_map, d.B, 1)) return -3;
    for (int i = 0; i < d.n_planes; ++i)
        if (!slot_ok(d.planes[i], d.B, 2)) return -3;
    for (int i = 0; i < d.n_label_planes; ++i)
        if (!slot_ok(d.label_planes[i], d.B, 1)) return -3;

    const int tiles = ((d.Fw + kTileW - 1) / kTileW) * ((d.Fh + kTileH - 1) / kTileH);
    render_frames_kernel<<<dim3(tiles, d.B), kThreads, 0, (hipStream_t)stream>>>(d);
    GWD_CHECK_LAUNCH();
    return 0;
}

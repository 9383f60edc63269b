// qoi_stats_core.h — the tile arithmetic of qoimi_pixel_stats: which pixels of a region a lane takes, what it keeps of them, how a lane's
// share joins the 64-bit totals, and what the flags make of the totals.
//
// The definition (normative; qoi_amd/pixelstats.py states it in Python).  A region cw x ch at (x, y) of an image staged as rows of w pixels of 4
// bytes has cw * ch pixels, numbered row-major.  A TILE is kStatsTilePx consecutive pixels of one region; lane l of the kStatsThreads lanes of a
// tile takes the kStatsLanePx consecutive pixels from tile * kStatsTilePx + l * kStatsLanePx on, as far as the region has them.  The two flip
// bits of a region change nothing but `first`: the walk ignores them.
//
// What a lane may keep in 32 bits.  A lane sees kStatsLanePx = 4 pixels of a tile and is flushed when its workgroup leaves the region, so it
// holds at most 4 pixels of every tile of ONE region, however the host cuts the tiles over workgroups (run_staged caps the grid at 8
// workgroups per compute unit; a single workgroup may walk a whole region).  A region lies inside an image of fewer than 400 000 000 pixels:
// at most ceil(400 000 000 / 1024) = 390 625 tiles, so a lane holds at most 4 * 390 625 = 1 562 500 pixels.
//   counters      <= 1 562 500                                < 2^32
//   channel sums  <= 255 * 1 562 500 =         398 437 500    < 2^32
//   square sums   <= 255 * 255 * 1 562 500 = 101 601 562 500  > 2^32: 64 bits in the lane (a lane passes 2^32 after 66 052 white pixels)
// Everything above the lane - the wavefront, the workgroup, the region's result - is 64 bits wide.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword; count(pixel, on) for the histogram), compiled for the device
// by hipcc (qoi_stats.hip: real loads, LDS atomics) and - by tests/host/stats_host.cpp only - for the host, where the functor checks that no
// load leaves the region, so the whole tile loop is compared with the Python model on the CPU before it runs on a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QOIMI_STATS_HD __host__ __device__ __forceinline__
#else
#define QOIMI_STATS_HD inline
#endif
#if defined(__clang__)
#define QOIMI_STATS_UNROLL _Pragma("unroll")
#else
#define QOIMI_STATS_UNROLL
#endif

namespace qoimi {

constexpr uint32_t kStatsThreads = 256;       // lanes of a tile: the workgroup of stats_reduce
constexpr uint32_t kStatsLanePx = 4;          // consecutive pixels of a lane
constexpr uint32_t kStatsTilePx = kStatsThreads * kStatsLanePx;
constexpr uint32_t kStatsFlipX = 1, kStatsFlipY = 2;
constexpr uint32_t kStatsConstant = 1, kStatsOpaque = 2, kStatsTransparent = 4, kStatsGrey = 8;   // QOIMI_PS_*

// w: pixels per staged row; (x, y, cw, ch): the region; flags: kStatsFlip*
struct StatsRect { uint32_t w, x, y, cw, ch, flags; };

// What a lane keeps between two flushes (the bounds: above).
struct StatsLane { uint32_t sum[4]; uint64_t sq[4]; uint32_t mn[4], mx[4]; uint32_t opaque, transparent, grey; };

// A region's result on the device: the host sets {0 ..., mn 255, mx 0, first 0} before the first launch; the sums and counters take 64-bit
// adds, mn / mx 32-bit minima / maxima per channel, `first` one plain store.
struct StatsAcc { uint64_t sum[4], sum_sq[4], opaque, transparent, grey; uint32_t mn[4], mx[4], first, reserved; };
static_assert(sizeof(StatsAcc) == 128, "result layout");
constexpr uint32_t kStatsSums = 11;            // the leading 64-bit words of StatsAcc that are sums

QOIMI_STATS_HD uint64_t stats_tiles(uint32_t cw, uint32_t ch) { return ((uint64_t)cw * ch + kStatsTilePx - 1u) / kStatsTilePx; }

QOIMI_STATS_HD void stats_clear(StatsLane& a) {
    QOIMI_STATS_UNROLL
    for (uint32_t k = 0; k < 4u; ++k) { a.sum[k] = 0u; a.sq[k] = 0u; a.mn[k] = 255u; a.mx[k] = 0u; }
    a.opaque = 0u; a.transparent = 0u; a.grey = 0u;
}

QOIMI_STATS_HD void stats_init(StatsAcc& t) {
    for (uint32_t k = 0; k < 4u; ++k) { t.sum[k] = 0u; t.sum_sq[k] = 0u; t.mn[k] = 255u; t.mx[k] = 0u; }
    t.opaque = 0u; t.transparent = 0u; t.grey = 0u; t.first = 0u; t.reserved = 0u;
}

// One pixel r | g << 8 | b << 16 | a << 24 into a lane's share.
QOIMI_STATS_HD void stats_pixel(StatsLane& a, uint32_t px) {
    QOIMI_STATS_UNROLL
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t v = (px >> (8u * k)) & 255u;
        a.sum[k] += v;
        a.sq[k] += (uint64_t)v * v;
        a.mn[k] = v < a.mn[k] ? v : a.mn[k];
        a.mx[k] = v > a.mx[k] ? v : a.mx[k];
    }
    a.opaque += (px >> 24) == 255u ? 1u : 0u;
    a.transparent += (px >> 24) == 0u ? 1u : 0u;
    a.grey += ((px ^ (px >> 8)) & 0xFFFFu) == 0u ? 1u : 0u;          // r == g and g == b
}

// The staged pixel index of pixel (0, 0) of the flipped region: the first pixel qoimi_decode_crops would write.
QOIMI_STATS_HD uint64_t stats_first_at(const StatsRect& g) {
    const uint32_t r = (g.flags & kStatsFlipY) != 0u ? g.y + g.ch - 1u : g.y, c = (g.flags & kStatsFlipX) != 0u ? g.x + g.cw - 1u : g.x;
    return (uint64_t)r * g.w + c;
}

// Lane `lane` of tile `tile` of the region: one division by the region's width, then the walk steps from pixel to pixel.  Nothing outside
// the region is loaded.  With HIST every lane reports every step to mem.count(pixel, on) - on: the lane has a pixel at this step - so that
// the functor may look across the lanes of a wavefront; the caller reaches this function with all lanes together.
template <bool HIST, class Mem>
QOIMI_STATS_HD void stats_tile(const Mem& mem, const StatsRect& g, uint32_t tile, uint32_t lane, StatsLane& a) {
    const uint64_t npx = (uint64_t)g.cw * g.ch, p0 = (uint64_t)tile * kStatsTilePx + (uint64_t)lane * kStatsLanePx;
    const uint32_t n = p0 >= npx ? 0u : npx - p0 < kStatsLanePx ? (uint32_t)(npx - p0) : kStatsLanePx;
    const uint32_t p = n != 0u ? (uint32_t)p0 : 0u;                   // (an image holds fewer than 400 000 000 pixels)
    const uint32_t r = p / g.cw;
    uint32_t c = p - r * g.cw;
    uint64_t at = (uint64_t)(g.y + r) * g.w + g.x + c;
    uint32_t px[kStatsLanePx];
    QOIMI_STATS_UNROLL
    for (uint32_t i = 0; i < kStatsLanePx; ++i) {
        px[i] = 0u;
        if (i < n) {
            px[i] = mem.load(at);
            ++at;
            if (++c == g.cw) { c = 0u; at += g.w - g.cw; }            // from behind a row's last pixel to the next row's first
        }
    }
    QOIMI_STATS_UNROLL
    for (uint32_t i = 0; i < kStatsLanePx; ++i) {
        if (HIST) mem.count(px[i], i < n);
        if (i < n) stats_pixel(a, px[i]);
    }
}

// A lane's share into 64-bit totals (the host's stand-in for the cross-lane reduction and the atomics of stats_reduce).
QOIMI_STATS_HD void stats_fold(StatsAcc& t, const StatsLane& a) {
    for (uint32_t k = 0; k < 4u; ++k) {
        t.sum[k] += a.sum[k]; t.sum_sq[k] += a.sq[k];
        t.mn[k] = a.mn[k] < t.mn[k] ? a.mn[k] : t.mn[k];
        t.mx[k] = a.mx[k] > t.mx[k] ? a.mx[k] : t.mx[k];
    }
    t.opaque += a.opaque; t.transparent += a.transparent; t.grey += a.grey;
}

// QOIMI_PS_* of a finished result over `pixels` pixels: a function of its other fields.
QOIMI_STATS_HD uint32_t stats_flags(const StatsAcc& t, uint64_t pixels) {
    bool constant = true;
    for (uint32_t k = 0; k < 4u; ++k) constant = constant && t.mn[k] == t.mx[k];
    return (constant ? kStatsConstant : 0u) | (t.opaque == pixels ? kStatsOpaque : 0u) | (t.transparent == pixels ? kStatsTransparent : 0u) |
           (t.grey == pixels ? kStatsGrey : 0u);
}

}  // namespace qoimi

// qoi_warp_core.h — the arithmetic of qoimi_decode_warped: which output pixel a work item of a tile is, where that pixel lies in the source
// rectangle, its 2 x 2 taps and their weights, the border, the blend, and the store (the division and the sums are those of
// qoi_resize_core.h: resize_pixel takes the divisor as an argument).
//
// The definition (normative; qoi_amd/warp.py states it in Python).  A rectangle cw x rh at (x, y) of an image staged as rows of w pixels of 4
// bytes is sampled into ow x oh pixels through an affine map.  Coordinates are DOUBLED pixel-centre coordinates with 16 fractional bits: the
// centre of source column k of the rectangle lies at (2k + 1) << 16.  Output pixel (X, Y) has U = 2X + 1, V = 2Y + 1 and
//   Px = a * U + b * V + c,  Py = d * U + e * V + f          (a, b, d, e: int; c, f: long long; the identity is a = e = 65536, else 0)
// One axis: p = P - 65536, k0 = p >> 17 (arithmetic: it floors), fr = p & 131071; sample k0 has the weight 131072 - fr, sample k0 + 1 the
// weight fr; a sample with the weight 0 is not taken.  Samples outside the rectangle are never read: with kWarpReplicate their index is
// clamped into it, otherwise they have the value `fill` (r | g << 8 | b << 16 | a << 24).  N_c is the sum of wy * wx * channel c over the 2 x 2
// samples, M_c the sum of wy * wx * channel c * alpha (c = 0..2); the weights of a pixel add up to T = 2^34.
//   PLAIN           every channel is (N_c + 2^33) >> 34 - one rounding
//   ALPHA_WEIGHTED  alpha likewise; with A = N_3 > 0 the colours are (M_c + A/2) / A; with A == 0 they are the PLAIN value
// Pixel (X, Y) is written at pixel (X, Y) of the output, och = 3 or 4 bytes per pixel, tightly packed from the absolute address q.  There is no
// antialiasing: a map that reduces still takes four samples.
// With kWarpNearest (a flag of the item, so the same for every work item of a tile) the 2 x 2 taps are replaced by ONE sample - selection, for
// label maps: column k = Px >> 17, row r = Py >> 17 (arithmetic: they floor; column k covers [k << 17, (k + 1) << 17), its centre at
// (2k + 1) << 16).  Outside the rectangle the index is clamped into it with kWarpReplicate, else the pixel is `fill`; the output pixel is the
// sample byte for byte in both modes (warp_nearest).  At a pixel centre - the identity, every qoimi_warp_orient item - that is the bilinear
// result, whose one sample with a weight has all of it.
// Bounds.  ow, oh < 2^20, so U, V < 2^21 and |a * U|, |b * V| <= 2^31 * 2^21 = 2^52; |c| < 2^56: |P| < 2^56 + 2^53 < 2^57 - both positions and
// the indices made of them are 64-bit, and the border is tested on the 64-bit index before anything is narrowed.  A horizontal blend
// wx0 * v0 + wx1 * v1 <= 255 * 2^17 is 32-bit; N_c <= 255 * 2^34 < 2^42.  With alpha a value is at most 255 * 255, its horizontal blend
// below 2^33 and M_c <= 255 * 255 * 2^34 < 2^50: 64-bit.
//
// The tiles: an item is cut into tiles of kWarpTile x kWarpTile output pixels, row-major over ceil(ow / 16) x ceil(oh / 16); work item t of a
// tile is the pixel (t & 15, t >> 4) of it, so a wavefront of 64 holds 16 columns x 4 rows: whatever the map turns the grid by, its taps lie in
// a patch of the source of about that size and not in 64 different rows.  Work items beyond an edge of the output idle.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_warp.hip) and - by tests/host/warp_host.cpp only - for the host, where the functor checks and counts every access.
#pragma once
#include <stdint.h>

#include "qoi_resize_core.h"

namespace qoimi {

constexpr uint32_t kWarpTile = 16;                              // a tile is kWarpTile x kWarpTile output pixels
constexpr uint32_t kWarpThreads = kWarpTile * kWarpTile;        // its work items: the workgroup of warp_gather
constexpr uint32_t kWarpReplicate = 1;
constexpr uint32_t kWarpNearest = 4;                            // (2 is not a flag)
constexpr uint32_t kWarpMaxOut = 1u << 20;                      // ow, oh stay below it
constexpr uint64_t kWarpMaxArea = 400000000ull;                 // ow * oh stays below it
constexpr int64_t kWarpMaxOffset = 1ll << 56;                   // |c|, |f| stay below it
constexpr uint32_t kWarpHalf = 1u << 16, kWarpOne = 1u << 17;   // half a pixel and a pixel in doubled coordinates with 16 fractional bits
constexpr uint64_t kWarpTotal = 1ull << 34;                     // the weights of a pixel

// w: pixels per staged row; (x, y, cw, rh): the rectangle; ow x oh: the output; flags: the item's (kWarpReplicate, kWarpNearest; qoi_warp_cubic_core.h and qoi_warp_border_core.h have more); the map; fill
struct WarpGeom { uint32_t w, x, y, cw, rh, ow, oh, flags; int32_t a, b, d, e; uint32_t fill; int64_t c, f; };
// The two samples of one axis: i[j] the index inside the rectangle where in[j], wgt[j] the weight (0: not taken)
struct WarpAxis { uint32_t i[2], wgt[2]; bool in[2]; };

// Tiles of an item
QOIMI_RESIZE_HD uint64_t warp_tiles(uint32_t ow, uint32_t oh) {
    return (uint64_t)((ow + kWarpTile - 1u) / kWarpTile) * ((oh + kWarpTile - 1u) / kWarpTile);
}

// Work item t of tile `tile` of an ow x oh output: its pixel, false beyond an edge.
QOIMI_RESIZE_HD bool warp_place(uint32_t tile, uint32_t t, uint32_t ow, uint32_t oh, uint32_t& X, uint32_t& Y) {
    const uint32_t across = (ow + kWarpTile - 1u) / kWarpTile, ty = tile / across, tx = tile - ty * across;
    X = tx * kWarpTile + (t & (kWarpTile - 1u));
    Y = ty * kWarpTile + t / kWarpTile;
    return X < ow && Y < oh;
}

// The position m * U + n * V + o of output pixel (X, Y)
QOIMI_RESIZE_HD int64_t warp_position(int32_t m, int32_t n, int64_t o, uint32_t X, uint32_t Y) {
    return (int64_t)m * (int64_t)(2ull * X + 1u) + (int64_t)n * (int64_t)(2ull * Y + 1u) + o;
}

// The samples of the position P on an axis of n source samples.
QOIMI_RESIZE_HD void warp_axis(int64_t P, uint32_t n, bool replicate, WarpAxis& ax) {
    const int64_t p = P - (int64_t)kWarpHalf, k0 = p >> 17;
    const uint32_t fr = (uint32_t)(p & (int64_t)(kWarpOne - 1u));
    ax.wgt[0] = kWarpOne - fr; ax.wgt[1] = fr;
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < 2u; ++j) {
        int64_t k = k0 + (int64_t)j;                               // (64-bit: the border test comes before the narrowing)
        bool in = k >= 0 && k < (int64_t)n;
        if (replicate) { k = k < 0 ? 0 : (k < (int64_t)n ? k : (int64_t)n - 1); in = true; }
        ax.in[j] = in && ax.wgt[j] != 0u;
        ax.i[j] = in ? (uint32_t)k : 0u;
    }
}

// The blend of the 2 x 2 samples of the axes ax (columns) and ay (rows) as r | g << 8 | b << 16 | a << 24: up to four loads, none for a
// sample that is not taken or takes the fill (whatever made the axes: warp_axis here, warp_border_axis of qoi_warp_border_core.h).
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_blend(const Mem& mem, const WarpGeom& g, const WarpAxis& ax, const WarpAxis& ay) {
    uint32_t v[2][2];
    QOIMI_RESIZE_UNROLL
    for (uint32_t r = 0; r < 2u; ++r) {
        const uint64_t at = (uint64_t)(g.y + ay.i[r]) * g.w + g.x;
        QOIMI_RESIZE_UNROLL
        for (uint32_t k = 0; k < 2u; ++k) v[r][k] = (ay.in[r] && ax.in[k]) ? mem.load(at + ax.i[k]) : g.fill;   // (a sample without a weight: any value)
    }
    ResizeSums s;
    QOIMI_RESIZE_UNROLL
    for (uint32_t ch = 0; ch < 4u; ++ch) {
        const uint32_t sh = 8u * ch;
        const uint32_t h0 = ax.wgt[0] * ((v[0][0] >> sh) & 255u) + ax.wgt[1] * ((v[0][1] >> sh) & 255u);
        const uint32_t h1 = ax.wgt[0] * ((v[1][0] >> sh) & 255u) + ax.wgt[1] * ((v[1][1] >> sh) & 255u);
        s.S[ch] = (uint64_t)ay.wgt[0] * h0 + (uint64_t)ay.wgt[1] * h1;
    }
    QOIMI_RESIZE_UNROLL
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        if (WEIGHTED) {
            const uint32_t sh = 8u * ch;
            const uint64_t h0 = (uint64_t)ax.wgt[0] * (((v[0][0] >> sh) & 255u) * (v[0][0] >> 24)) + (uint64_t)ax.wgt[1] * (((v[0][1] >> sh) & 255u) * (v[0][1] >> 24));
            const uint64_t h1 = (uint64_t)ax.wgt[0] * (((v[1][0] >> sh) & 255u) * (v[1][0] >> 24)) + (uint64_t)ax.wgt[1] * (((v[1][1] >> sh) & 255u) * (v[1][1] >> 24));
            s.W[ch] = ay.wgt[0] * h0 + ay.wgt[1] * h1;
        } else s.W[ch] = 0u;
    }
    return resize_pixel(s, kWarpTotal, WEIGHTED);
}

// The output pixel whose position in the rectangle is (Px, Py): the axes with the border by kWarpReplicate or the fill, and their blend.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_pixel_at(const Mem& mem, const WarpGeom& g, int64_t Px, int64_t Py) {
    const bool replicate = (g.flags & kWarpReplicate) != 0u;
    WarpAxis ax, ay;
    warp_axis(Px, g.cw, replicate, ax);
    warp_axis(Py, g.rh, replicate, ay);
    return warp_blend<WEIGHTED>(mem, g, ax, ay);
}

// Output pixel (X, Y): warp_pixel_at its position under the affine map.  (Written out, each position formed where its axis takes it, not as
// a call of warp_pixel_at: handed both positions first, the compiler allots warp_gather and tensor_warp other registers than the ones
// tests/test_warp_bicubic_api.py holds them to; the results are the same.)
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_pixel(const Mem& mem, const WarpGeom& g, uint32_t X, uint32_t Y) {
    const bool replicate = (g.flags & kWarpReplicate) != 0u;
    WarpAxis ax, ay;
    warp_axis(warp_position(g.a, g.b, g.c, X, Y), g.cw, replicate, ax);
    warp_axis(warp_position(g.d, g.e, g.f, X, Y), g.rh, replicate, ay);
    return warp_blend<WEIGHTED>(mem, g, ax, ay);
}

// The output pixel at the position (Px, Py) under kWarpNearest: one load, none where the pixel takes the fill.
template <class Mem>
QOIMI_RESIZE_HD uint32_t warp_nearest_at(const Mem& mem, const WarpGeom& g, int64_t Px, int64_t Py) {
    int64_t k = Px >> 17, r = Py >> 17;                            // (64-bit: the border test comes before the narrowing)
    bool in = k >= 0 && k < (int64_t)g.cw && r >= 0 && r < (int64_t)g.rh;
    if ((g.flags & kWarpReplicate) != 0u) {
        k = k < 0 ? 0 : (k < (int64_t)g.cw ? k : (int64_t)g.cw - 1);
        r = r < 0 ? 0 : (r < (int64_t)g.rh ? r : (int64_t)g.rh - 1);
        in = true;
    }
    return in ? mem.load((uint64_t)(g.y + (uint32_t)r) * g.w + g.x + (uint32_t)k) : g.fill;
}

// Output pixel (X, Y) under kWarpNearest: warp_nearest_at its position under the affine map.
template <class Mem>
QOIMI_RESIZE_HD uint32_t warp_nearest(const Mem& mem, const WarpGeom& g, uint32_t X, uint32_t Y) {
    return warp_nearest_at(mem, g, warp_position(g.a, g.b, g.c, X, Y), warp_position(g.d, g.e, g.f, X, Y));
}

// Pixel (X, Y) to its place in the output at q: one dword where the output holds 4 bytes per pixel and the address is aligned, else och
// bytes - the item's own bytes only, never a word that would have to be read first.
template <class Mem>
QOIMI_RESIZE_HD void warp_store(const Mem& mem, uint64_t q, uint32_t ow, uint32_t och, uint32_t X, uint32_t Y, uint32_t px) {
    const uint64_t a = q + ((uint64_t)Y * ow + X) * och;
    if (och == 4u && (a & 3u) == 0u) { mem.store4(a, px); return; }
    mem.store1(a, px); mem.store1(a + 1u, px >> 8); mem.store1(a + 2u, px >> 16);
    if (och == 4u) mem.store1(a + 3u, px >> 24);
}

// The finish step of the warp tile as a sink - pixel px = (X, Y) to the output at q - for the call that writes bytes (qoi_tensor_core.h:
// TensorSink is the other one).
struct WarpByteSink {
    template <class Mem>
    QOIMI_RESIZE_HD void operator()(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t X, uint32_t Y, uint32_t px) const {
        warp_store(mem, q, g.ow, och, X, Y, px);
    }
};

// Work item t of tile `tile` of the item: its pixel computed and handed to the sink, or nothing beyond an edge.
template <bool WEIGHTED, class Mem, class Sink>
QOIMI_RESIZE_HD void warp_work(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t tile, uint32_t t, const Sink& sink) {
    uint32_t X, Y;
    if (!warp_place(tile, t, g.ow, g.oh, X, Y)) return;
    sink(mem, g, q, och, X, Y, (g.flags & kWarpNearest) != 0u ? warp_nearest(mem, g, X, Y) : warp_pixel<WEIGHTED>(mem, g, X, Y));
}

// ... stored as bytes (warp_store)
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD void warp_work(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t tile, uint32_t t) {
    warp_work<WEIGHTED>(mem, g, q, och, tile, t, WarpByteSink());
}

}  // namespace qoimi

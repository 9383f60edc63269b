// qoi_warp_super_core.h — the arithmetic of qoimi_decode_warped with QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4: the position of a sub-sample, the
// blend of its 2 x 2 taps ACCUMULATED into unrounded sums, the one rounding of an output pixel, and the work item of the tile that serves items
// with and without such a flag alike.  The taps of an axis, their weights, their indices and the border are those of qoi_warp_core.h and
// qoi_warp_border_core.h (warp_axis, warp_border_axis), the rounding and the divisions those of qoi_resize_core.h (resize_pixel, resize_div):
// shared, not restated.
//
// The definition (normative; qoi_amd/warp.py states it in Python).  kWarpSuper2: s = 2, L = 1; kWarpSuper4: s = 4, L = 2; at most one of the
// two, with the bilinear sampling only.  Output pixel (X, Y), U = 2X + 1, V = 2Y + 1, is the mean of s x s bilinear samples laid on a regular
// grid inside the pixel, with ONE rounding.  For 0 <= i, j < s:
//   Us = s * U + 2i + 1 - s,   Vs = s * V + 2j + 1 - s          (the sub-sample's centre in coordinates s times finer)
//   Px = ((a * Us + b * Vs) >> L) + c,   Py = ((d * Us + e * Vs) >> L) + f     (arithmetic shift: it floors)
// From (Px, Py) the 2 x 2 taps, their weights (131072 - fx, fx and likewise for rows), their indices and the border are exactly those of the
// bilinear warp: a tap outside the rectangle takes `fill`, under kWarpReplicate its index is clamped, under kWarpReflect / kWarpReflect101 /
// kWarpWrap it is folded, each tap on its own; a tap of weight 0 is not taken and never read.  N_c is the sum over all s^2 sub-samples and
// their four taps of wy * wx * c, M_c the same sum of wy * wx * c * alpha; the weights of a pixel add up to T = 2^(34 + 2L).
//   PLAIN           every channel is (N_c + 2^(33 + 2L)) >> (34 + 2L) - one rounding
//   ALPHA_WEIGHTED  alpha likewise; with A = N_3 > 0 the colours are (M_c + A/2) / A; with A == 0 they are the PLAIN value
// Bounds.  Us, Vs < 2^23, so |a * Us + b * Vs| < 2 * 2^31 * 2^23 = 2^55; after the shift the sum is no larger than the unflagged a * U + b * V
// can be, so |Px|, |Py| < 2^57 as there and the fold's preconditions (|k| < 2^40) hold unchanged.  One sub-sample adds at most 255 * 2^34 to
// N_c and 255 * 255 * 2^34 to M_c: N_c <= 255 * 2^38 < 2^46, M_c < 2^54: 64-bit, M_c + A/2 too.
// There is no adaptivity: s^2 sub-samples are taken whether or not the map reduces.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_warp_super.hip) and - by tests/host/warp_super_host.cpp only - for the host, where the functor checks and counts every
// access.
#pragma once
#include <stdint.h>

#include "qoi_warp_border_core.h"

namespace qoimi {

constexpr uint32_t kWarpSuper2 = 1024, kWarpSuper4 = 2048;      // (512 is not a flag)
constexpr uint32_t kWarpSupers = kWarpSuper2 | kWarpSuper4;     // an item with one of them takes the paths of this file

// L of the item's flags: s = 1 << L sub-samples along each axis of an output pixel (0 without a flag: the pixel's own centre)
QOIMI_RESIZE_HD uint32_t warp_super_log2(uint32_t flags) { return (flags & kWarpSuper4) != 0u ? 2u : ((flags & kWarpSuper2) != 0u ? 1u : 0u); }

// The position ((m * Us + n * Vs) >> L) + o of sub-sample (i, j) of output pixel (X, Y): warp_position where L == 0
QOIMI_RESIZE_HD int64_t warp_super_position(int32_t m, int32_t n, int64_t o, uint32_t X, uint32_t Y, uint32_t i, uint32_t j, uint32_t L) {
    const int64_t s = (int64_t)1 << L;
    const int64_t Us = s * (int64_t)(2ull * X + 1u) + (int64_t)(2u * i + 1u) - s, Vs = s * (int64_t)(2ull * Y + 1u) + (int64_t)(2u * j + 1u) - s;
    return (((int64_t)m * Us + (int64_t)n * Vs) >> L) + o;
}

// The 2 x 2 samples of the axes ax (columns) and ay (rows) ADDED to the sums, unrounded: warp_blend's loads - up to four, none for a sample
// that is not taken or takes the fill - and its products, without its rounding.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD void warp_super_add(const Mem& mem, const WarpGeom& g, const WarpAxis& ax, const WarpAxis& ay, ResizeSums& s) {
    uint32_t v[2][2];
    QOIMI_RESIZE_UNROLL
    for (uint32_t r = 0; r < 2u; ++r) {
        const uint64_t at = (uint64_t)(g.y + ay.i[r]) * g.w + g.x;
        QOIMI_RESIZE_UNROLL
        for (uint32_t k = 0; k < 2u; ++k) v[r][k] = (ay.in[r] && ax.in[k]) ? mem.load(at + ax.i[k]) : g.fill;   // (a sample without a weight: any value)
    }
    QOIMI_RESIZE_UNROLL
    for (uint32_t ch = 0; ch < 4u; ++ch) {
        const uint32_t sh = 8u * ch;
        const uint32_t h0 = ax.wgt[0] * ((v[0][0] >> sh) & 255u) + ax.wgt[1] * ((v[0][1] >> sh) & 255u);
        const uint32_t h1 = ax.wgt[0] * ((v[1][0] >> sh) & 255u) + ax.wgt[1] * ((v[1][1] >> sh) & 255u);
        s.S[ch] += (uint64_t)ay.wgt[0] * h0 + (uint64_t)ay.wgt[1] * h1;
    }
    if (WEIGHTED) {
        QOIMI_RESIZE_UNROLL
        for (uint32_t ch = 0; ch < 3u; ++ch) {
            const uint32_t sh = 8u * ch;
            const uint64_t h0 = (uint64_t)ax.wgt[0] * (((v[0][0] >> sh) & 255u) * (v[0][0] >> 24)) + (uint64_t)ax.wgt[1] * (((v[0][1] >> sh) & 255u) * (v[0][1] >> 24));
            const uint64_t h1 = (uint64_t)ax.wgt[0] * (((v[1][0] >> sh) & 255u) * (v[1][0] >> 24)) + (uint64_t)ax.wgt[1] * (((v[1][1] >> sh) & 255u) * (v[1][1] >> 24));
            s.W[ch] += ay.wgt[0] * h0 + ay.wgt[1] * h1;
        }
    }
}

// Output pixel (X, Y) of an item with a SUPER flag: its s x s sub-samples, each with the item's border, into one set of sums; one rounding
// (resize_pixel: a shift for the PLAIN value, resize_div for the weighted colours).
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_super_pixel(const Mem& mem, const WarpGeom& g, uint32_t X, uint32_t Y) {
    const uint32_t L = warp_super_log2(g.flags), s = 1u << L, border = g.flags & kWarpBorders;
    const bool replicate = (g.flags & kWarpReplicate) != 0u;
    const WarpFold fx = warp_fold_of(border, g.cw), fy = warp_fold_of(border, g.rh);   // (looked at under a folding border only)
    ResizeSums sums;
    resize_zero(sums);
    for (uint32_t j = 0; j < s; ++j)
        for (uint32_t i = 0; i < s; ++i) {
            const int64_t Px = warp_super_position(g.a, g.b, g.c, X, Y, i, j, L), Py = warp_super_position(g.d, g.e, g.f, X, Y, i, j, L);
            WarpAxis ax, ay;
            if (border != 0u) { warp_border_axis(Px, fx, ax); warp_border_axis(Py, fy, ay); }
            else { warp_axis(Px, g.cw, replicate, ax); warp_axis(Py, g.rh, replicate, ay); }
            warp_super_add<WEIGHTED>(mem, g, ax, ay, sums);
        }
    return resize_pixel(sums, kWarpTotal << (2u * L), WEIGHTED);
}

// Work item t of tile `tile` of the item: warp_super_pixel for an item with a SUPER flag, warp_border_work as it is for any other (the flags
// are the item's, so the branch is the tile's), handed to the sink, or nothing beyond an edge.
template <bool WEIGHTED, class Mem, class Sink>
QOIMI_RESIZE_HD void warp_super_work(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t tile, uint32_t t, const Sink& sink) {
    if ((g.flags & kWarpSupers) == 0u) { warp_border_work<WEIGHTED>(mem, g, q, och, tile, t, sink); return; }
    uint32_t X, Y;
    if (!warp_place(tile, t, g.ow, g.oh, X, Y)) return;
    sink(mem, g, q, och, X, Y, warp_super_pixel<WEIGHTED>(mem, g, X, Y));
}

}  // namespace qoimi

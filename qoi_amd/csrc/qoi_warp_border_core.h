// qoi_warp_border_core.h — the arithmetic of qoimi_decode_warped with QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 or QOIMI_WARP_WRAP: the fold of
// a sample index into the rectangle, the samples of an axis for one, two and four taps, and the work item of the tile that serves items with
// and without such a border alike.  The position, the fractions, the weights, the blends, the rounding, the clamp and the stores are those of
// qoi_warp_core.h and qoi_warp_cubic_core.h (warp_blend, warp_cubic_weights, warp_cubic_blend): shared, not restated.  Only the INDEX of a tap
// is new.
//
// The definition (normative; qoi_amd/warp.py states it in Python: fold).  Every 64-bit tap index k on an axis of n samples is folded into
// [0, n) before anything is narrowed; the fill is not used (as with kWarpReplicate).  `mod` floors: 0 <= m < P for negative k too.
//   kWarpReflect     "dcba|abcd|dcba"  P = 2n, m = k mod P, index m < n ? m : P - 1 - m
//   kWarpReflect101  "dcb|abcd|cba"    n == 1: index 0; else P = 2n - 2, m = k mod P, index m < n ? m : P - m
//   kWarpWrap        "abcd|abcd|abcd"  index k mod n
// Each tap is folded on its own - the 2 of the bilinear sampling, the 4 of the bicubic, the one of kWarpNearest.  A tap with the weight 0 is
// not taken and never read; nothing outside the rectangle is ever read.
//
// How it is computed.  All three are ONE walk: a period P (2n, max(2n - 2, 1), n), the position m = k mod P in it, and the index
// m < n ? m : E - m with E = P - 1 for kWarpReflect and E = P for kWarpReflect101 (kWarpWrap has m < n always; n == 1 under kWarpReflect101 has
// P = 1, m = 0).  The FIRST tap of an axis is folded (warp_fold_position); the next taps step m by one and wrap at P, no second fold.
// The fold: |k| < 2^40 (|P| < 2^57 >> 17) and P < 2^30 (an image has fewer than 400 000 000 pixels).  Where -P <= k < 2P - the tap lies within
// one period of the rectangle, every lane of an ordinary augmentation - a conditional add or subtract is all.  Beyond that k is first
// brought into that range with a quotient ESTIMATE in double precision: q = floor((double)k * (1.0 / (double)P)), k -= q * P.  k and P are
// exact doubles (below 2^53); the reciprocal and the product each round once, a relative error below 2^-51 of a quotient below 2^40: the
// estimate is off by less than 2^-11 before the floor, so q is the true quotient or one beside it and k - q * P lies in [-P, 2P) - exactly what
// the conditional add or subtract finishes.  The result is the exact remainder for every accepted index, not an approximation: the double
// only chooses which multiple of P the 64-bit integer subtraction takes.  No 64-bit integer division is compiled (on gfx950 a 64-by-32 udiv is
// a call-free but long software sequence; a v_rcp_f64, two conversions, a v_mul_f64, a v_floor_f64 and a 64-bit multiply-subtract replace it).
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_warp_border.hip) and - by tests/host/warp_border_host.cpp only - for the host, where the functor checks and counts every
// access.
#pragma once
#include <stdint.h>

#include "qoi_warp_cubic_core.h"

namespace qoimi {

constexpr uint32_t kWarpReflect = 64, kWarpReflect101 = 128, kWarpWrap = 256;   // (32 is not a flag)
constexpr uint32_t kWarpBorders = kWarpReflect | kWarpReflect101 | kWarpWrap;   // an item with one of them takes the paths of this file

// The walk of one axis of n samples under a border: the period P and the mirror point E (index = m < n ? m : E - m)
struct WarpFold { uint32_t n, P, E; };

QOIMI_RESIZE_HD WarpFold warp_fold_of(uint32_t border, uint32_t n) {
    if ((border & kWarpWrap) != 0u) return {n, n, 0u};                                  // (m < n always: E is not looked at)
    if ((border & kWarpReflect) != 0u) return {n, 2u * n, 2u * n - 1u};
    const uint32_t P = n > 1u ? 2u * n - 2u : 1u;
    return {n, P, P};
}

// m = k mod P, flooring, for |k| < 2^40 and 0 < P < 2^30
QOIMI_RESIZE_HD uint32_t warp_fold_position(int64_t k, uint32_t P) {
    const int64_t p = (int64_t)P;
    if (k < -p || k >= 2 * p) k -= (int64_t)__builtin_floor((double)k * (1.0 / (double)P)) * p;   // (the estimate: k is in [-P, 2P) after it)
    if (k < 0) k += p;
    else if (k >= p) k -= p;
    return (uint32_t)k;
}

// The position after m
QOIMI_RESIZE_HD uint32_t warp_fold_next(uint32_t m, const WarpFold& fo) { return m + 1u == fo.P ? 0u : m + 1u; }

// The sample at the position m
QOIMI_RESIZE_HD uint32_t warp_fold_index(uint32_t m, const WarpFold& fo) { return m < fo.n ? m : fo.E - m; }

// The index k folded into [0, n): the definition in one call (the tests walk it; the axes below fold once and step)
QOIMI_RESIZE_HD uint32_t warp_fold(int64_t k, uint32_t n, uint32_t border) {
    const WarpFold fo = warp_fold_of(border, n);
    return warp_fold_index(warp_fold_position(k, fo.P), fo);
}

// The two samples of the position P on an axis under a border: warp_axis with every index folded
QOIMI_RESIZE_HD void warp_border_axis(int64_t P, const WarpFold& fo, WarpAxis& ax) {
    const int64_t p = P - (int64_t)kWarpHalf;
    const uint32_t fr = (uint32_t)(p & (int64_t)(kWarpOne - 1u));
    ax.wgt[0] = kWarpOne - fr; ax.wgt[1] = fr;
    uint32_t m = warp_fold_position(p >> 17, fo.P);
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < 2u; ++j) {
        ax.in[j] = ax.wgt[j] != 0u;
        ax.i[j] = warp_fold_index(m, fo);
        m = warp_fold_next(m, fo);
    }
}

// The four samples: warp_cubic_axis with every index folded
QOIMI_RESIZE_HD void warp_border_cubic_axis(int64_t P, const WarpFold& fo, WarpCubicAxis& ax) {
    const int64_t p = P - (int64_t)kWarpHalf;
    warp_cubic_weights((uint32_t)(p & (int64_t)(kWarpOne - 1u)), ax.q);
    uint32_t m = warp_fold_position((p >> 17) - 1, fo.P);
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < 4u; ++j) {
        ax.in[j] = ax.q[j] != 0;
        ax.i[j] = warp_fold_index(m, fo);
        m = warp_fold_next(m, fo);
    }
}

// The output pixel at the position (Px, Py) of an item with a border flag, by its sampling: one, 2 x 2 or 4 x 4 samples, every one of them
// inside the rectangle.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_border_pixel_at(const Mem& mem, const WarpGeom& g, int64_t Px, int64_t Py) {
    const uint32_t border = g.flags & kWarpBorders;
    const WarpFold fx = warp_fold_of(border, g.cw), fy = warp_fold_of(border, g.rh);
    if ((g.flags & kWarpNearest) != 0u) {
        const uint32_t k = warp_fold_index(warp_fold_position(Px >> 17, fx.P), fx), r = warp_fold_index(warp_fold_position(Py >> 17, fy.P), fy);
        return mem.load((uint64_t)(g.y + r) * g.w + g.x + k);
    }
    if ((g.flags & kWarpBicubic) != 0u) {
        WarpCubicAxis ax, ay;
        warp_border_cubic_axis(Px, fx, ax);
        warp_border_cubic_axis(Py, fy, ay);
        return warp_cubic_blend<WEIGHTED>(mem, g, ax, ay);
    }
    WarpAxis ax, ay;
    warp_border_axis(Px, fx, ax);
    warp_border_axis(Py, fy, ay);
    return warp_blend<WEIGHTED>(mem, g, ax, ay);
}

// Output pixel (X, Y) of an item with a border flag: warp_border_pixel_at its position under the affine map.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_border_pixel(const Mem& mem, const WarpGeom& g, uint32_t X, uint32_t Y) {
    return warp_border_pixel_at<WEIGHTED>(mem, g, warp_position(g.a, g.b, g.c, X, Y), warp_position(g.d, g.e, g.f, X, Y));
}

// Work item t of tile `tile` of the item: warp_border_pixel for an item with a border flag, warp_cubic_work as it is for any other (the
// flags are the item's, so the branch is the tile's), handed to the sink, or nothing beyond an edge.
template <bool WEIGHTED, class Mem, class Sink>
QOIMI_RESIZE_HD void warp_border_work(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t tile, uint32_t t, const Sink& sink) {
    if ((g.flags & kWarpBorders) == 0u) { warp_cubic_work<WEIGHTED>(mem, g, q, och, tile, t, sink); return; }
    uint32_t X, Y;
    if (!warp_place(tile, t, g.ow, g.oh, X, Y)) return;
    sink(mem, g, q, och, X, Y, warp_border_pixel<WEIGHTED>(mem, g, X, Y));
}

}  // namespace qoimi

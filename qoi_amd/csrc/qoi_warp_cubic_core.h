// qoi_warp_cubic_core.h — the arithmetic of qoimi_decode_warped with QOIMI_WARP_BICUBIC: the four weights of an axis in 15 fractional bits
// that sum exactly, the four samples of an axis and their border, the 4 x 4 blend row by row, and the work item of the tile that serves
// bicubic, bilinear and nearest items alike.  The position, the tile, the border rule and the stores are those of qoi_warp_core.h; the cubic
// weight, the clamp, the rounding and the division are those of qoi_cubic_core.h (cubic_weight, cubic_pixel, cubic_div_round): shared, not
// restated.
//
// The definition (normative; qoi_amd/warp.py states it in Python).  Px, Py are the positions of qoi_warp_core.h.  One axis, u = 2^17:
// p = P - 65536, k0 = p >> 17 (arithmetic: it floors), fr = p & 131071.  The four samples are k0 - 1, k0, k0 + 1, k0 + 2 at the distances
// d = u + fr, fr, u - fr, 2u - fr, and
//   c(d) = 3d^3 - 5u d^2 + 2u^3                for d <= u
//   c(d) = -d^3 + 5u d^2 - 8u^2 d + 4u^3       for u < d < 2u
//   c(d) = 0                                   from 2u on
// - 2u^3 times Keys' kernel with a = -1/2 at d / u: cubic_weight(d, 0, 0, u).  The four c add up to W = 2u^3 = 2^52 for every fr (Keys' kernel
// is a partition of unity; qoi_amd/warp.py asserts it over all 2^17 fr).  q_j = (c_j + 2^36) >> 37 (arithmetic) - c_j * 2^15 / W rounded; the
// deficit 2^15 - sum q_j is added to the tap with the largest c, the lowest j on a tie: sum q_j = 2^15.  A tap with q == 0 is not taken and
// never read.  Samples outside the rectangle are never read: with kWarpReplicate each of the four indices is clamped into it (the 64-bit index
// is tested before it is narrowed), otherwise the sample has the value `fill` and KEEPS its weight - no renormalisation, as in the bilinear
// warp.  N_c is the sum of qy * qx * channel c over the 4 x 4 samples, M_c the sum of qy * qx * channel c * alpha (c = 0..2) - signed.
//   PLAIN           every channel is clamp((N_c + 2^29) >> 30, 0, 255) - one rounding
//   ALPHA_WEIGHTED  alpha is the PLAIN value; with A = N_3 > 0 the colours are clamp((M_c + A/2) / A, 0, 255), else (A <= 0: the negative
//                   lobes make that possible) the PLAIN value
// At a pixel centre (fr = 0) the weights are (0, 2^15, 0, 0): one load, the sample itself.
// Bounds.  Every term of c is below 2^56 (d < 2^18: d^3 < 2^54, 5u d^2 < 5 * 2^53, 8u^2 d < 2^55), the factors cubic_weight multiplies are
// below 2^38 and 2^18: 64 bits hold them.  |q| <= 2^15; the |q| of an axis sum to at most 5 * 2^13 = 1.25 * 2^15 (reached at fr = u / 2:
// -1/16, 9/16, 9/16, -1/16; asserted over all fr by qoi_amd/warp.py).  A horizontal blend sum qx * v is at most 255 * 1.25 * 2^15 < 2^24 in
// magnitude: 32-bit; |N_c| <= 255 * (1.25 * 2^15)^2 < 2^40.  With alpha a value is at most 255 * 255, its horizontal blend below 2^32 (64-bit)
// and |M_c| < 2^48: the sums are 64-bit two's complement in ResizeSums.
//
// A lane goes ROW BY ROW: the up to four samples of a row, their horizontal blend per channel, then one multiply-add by qy per channel - it
// holds one row of samples, not sixteen pixels.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_warp_cubic.hip) and - by tests/host/warp_bicubic_host.cpp only - for the host, where the functor checks and counts every
// access.
#pragma once
#include <stdint.h>

#include "qoi_cubic_core.h"
#include "qoi_warp_core.h"

namespace qoimi {

constexpr uint32_t kWarpBicubic = 16;                           // (8 is not a flag)

// The four samples of one axis: i[j] the index inside the rectangle where in[j] (else the sample is the fill or not taken), q[j] the weight
struct WarpCubicAxis { uint32_t i[4]; int32_t q[4]; bool in[4]; };

// The weights of the samples k0 - 1 .. k0 + 2 for the fraction fr < 2^17: they add up to kCubicOne.
QOIMI_RESIZE_HD void warp_cubic_weights(uint32_t fr, int32_t q[4]) {
    const uint32_t d[4] = {kWarpOne + fr, fr, kWarpOne - fr, 2u * kWarpOne - fr};
    int64_t best = 0;
    uint32_t jbest = 0;
    int32_t sum = 0;
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < 4u; ++j) {
        const int64_t c = cubic_weight(d[j], 0u, 0u, kWarpOne);
        if (c > best) { best = c; jbest = j; }                     // (the largest c is positive; the lowest j keeps a tie)
        q[j] = (int32_t)((c + ((int64_t)1 << 36)) >> 37);
        sum += q[j];
    }
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < 4u; ++j) q[j] += j == jbest ? kCubicOne - sum : 0;   // (no indexed write: q stays in registers)
}

// The samples of the position P on an axis of n source samples.
QOIMI_RESIZE_HD void warp_cubic_axis(int64_t P, uint32_t n, bool replicate, WarpCubicAxis& ax) {
    const int64_t p = P - (int64_t)kWarpHalf, k0 = p >> 17;
    warp_cubic_weights((uint32_t)(p & (int64_t)(kWarpOne - 1u)), ax.q);
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < 4u; ++j) {
        int64_t k = k0 + (int64_t)j - 1;                           // (64-bit: the border test comes before the narrowing)
        bool in = k >= 0 && k < (int64_t)n;
        if (replicate) { k = k < 0 ? 0 : (k < (int64_t)n ? k : (int64_t)n - 1); in = true; }
        ax.in[j] = in && ax.q[j] != 0;
        ax.i[j] = in ? (uint32_t)k : 0u;
    }
}

// The blend of the 4 x 4 samples of the axes ax (columns) and ay (rows) as r | g << 8 | b << 16 | a << 24: up to sixteen loads, four at a
// time, none for a sample that is not taken or takes the fill (whatever made the axes: warp_cubic_axis here, warp_border_cubic_axis of
// qoi_warp_border_core.h).
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_cubic_blend(const Mem& mem, const WarpGeom& g, const WarpCubicAxis& ax, const WarpCubicAxis& ay) {
    ResizeSums s;
    resize_zero(s);
    QOIMI_RESIZE_UNROLL
    for (uint32_t r = 0; r < 4u; ++r) {
        if (ay.q[r] == 0) continue;                                // (a row without a weight: nothing is read)
        const uint64_t at = (uint64_t)(g.y + ay.i[r]) * g.w + g.x;
        uint32_t v[4];
        QOIMI_RESIZE_UNROLL
        for (uint32_t k = 0; k < 4u; ++k) v[k] = (ay.in[r] && ax.in[k]) ? mem.load(at + ax.i[k]) : g.fill;   // (a sample without a weight: any value)
        const int64_t qy = ay.q[r];
        QOIMI_RESIZE_UNROLL
        for (uint32_t ch = 0; ch < 4u; ++ch) {
            const uint32_t sh = 8u * ch;
            int32_t h = 0;
            QOIMI_RESIZE_UNROLL
            for (uint32_t k = 0; k < 4u; ++k) h += ax.q[k] * (int32_t)((v[k] >> sh) & 255u);
            s.S[ch] += (uint64_t)(qy * h);
        }
        if (WEIGHTED) {
            QOIMI_RESIZE_UNROLL
            for (uint32_t ch = 0; ch < 3u; ++ch) {
                const uint32_t sh = 8u * ch;
                int64_t h = 0;
                QOIMI_RESIZE_UNROLL
                for (uint32_t k = 0; k < 4u; ++k) h += (int64_t)ax.q[k] * (int32_t)(((v[k] >> sh) & 255u) * (v[k] >> 24));
                s.W[ch] += (uint64_t)(qy * h);
            }
        }
    }
    return cubic_pixel(s, WEIGHTED);
}

// The output pixel whose position in the rectangle is (Px, Py): the axes with the border by kWarpReplicate or the fill, and their blend.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_cubic_pixel_at(const Mem& mem, const WarpGeom& g, int64_t Px, int64_t Py) {
    const bool replicate = (g.flags & kWarpReplicate) != 0u;
    WarpCubicAxis ax, ay;
    warp_cubic_axis(Px, g.cw, replicate, ax);
    warp_cubic_axis(Py, g.rh, replicate, ay);
    return warp_cubic_blend<WEIGHTED>(mem, g, ax, ay);
}

// Output pixel (X, Y): warp_cubic_pixel_at its position under the affine map.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD uint32_t warp_cubic_pixel(const Mem& mem, const WarpGeom& g, uint32_t X, uint32_t Y) {
    return warp_cubic_pixel_at<WEIGHTED>(mem, g, warp_position(g.a, g.b, g.c, X, Y), warp_position(g.d, g.e, g.f, X, Y));
}

// Work item t of tile `tile` of the item: its pixel computed - 4 x 4 samples for an item with kWarpBicubic, warp_nearest / warp_pixel as they
// are for any other (the flags are the item's, so the branch is the tile's) - and handed to the sink, or nothing beyond an edge.
template <bool WEIGHTED, class Mem, class Sink>
QOIMI_RESIZE_HD void warp_cubic_work(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t tile, uint32_t t, const Sink& sink) {
    uint32_t X, Y;
    if (!warp_place(tile, t, g.ow, g.oh, X, Y)) return;
    uint32_t px;
    if ((g.flags & kWarpBicubic) != 0u) px = warp_cubic_pixel<WEIGHTED>(mem, g, X, Y);
    else px = (g.flags & kWarpNearest) != 0u ? warp_nearest(mem, g, X, Y) : warp_pixel<WEIGHTED>(mem, g, X, Y);
    sink(mem, g, q, och, X, Y, px);
}

}  // namespace qoimi

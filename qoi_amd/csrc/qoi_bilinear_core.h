// qoi_bilinear_core.h — the arithmetic of qoimi_decode_bilinear: the first source sample with a weight, the closed-form tent weights, how an
// output pixel's source columns are shared among lanes, one lane's weighted sums over its share, D(X, Y), and the finish (the division and the
// stores are those of qoi_resize_core.h: resize_pixel, resize_div_round take the divisor as an argument).
//
// The definition (normative; qoi_amd/bilinear.py states it in Python).  A rectangle cw x rh at (x, y) of an image staged as rows of w pixels of 4
// bytes is resampled to ow x oh pixels.  One axis, n_src samples to n_out, on a line of length 2 * n_src * n_out: source sample k has its centre
// at (2k + 1) * n_out, output sample X at (2X + 1) * n_src; rad = 2 * max(n_src, n_out); t(X, k) = max(0, rad - |(2X+1) * n_src - (2k+1) * n_out|)
// for 0 <= k < n_src; W(X) = sum_k t(X, k) >= 1 (samples outside the rectangle do not exist: the weights are renormalised, not clamped).
// tx, Wx from (cw, ow), ty, Wy from (rh, oh).  D = Wx(X) * Wy(Y); N_c is the sum of ty * tx * channel c over the rectangle, M_c the sum of
// ty * tx * channel c * alpha (c = 0..2).
//   PLAIN           every channel is (N_c + D/2) / D - integer divisions: floor, a half rounds up; one rounding, no intermediate
//   ALPHA_WEIGHTED  alpha is (N_3 + D/2) / D; with A = N_3 > 0 the colours are (M_c + A/2) / A; with A == 0 they are the PLAIN value
// Pixel (X, Y) of that result is written at pixel (FLIP_X ? ow - 1 - X : X, FLIP_Y ? oh - 1 - Y : Y) of the output, och = 3 or 4 bytes per
// pixel, tightly packed from the absolute address q.
// cw <= 32 * ow, rh <= 32 * oh and max(cw, ow) * max(rh, oh) < 2^30.  The samples with a weight lie in an open interval of length 2 * rad and
// are 2 * n_out apart: at most ceil(rad / n_out) of them - 2 when enlarging, up to 64 when reducing (bilinear_taps).  One t <= rad, so one
// weight ty * tx <= 4 * max(cw, ow) * max(rh, oh) < 2^32: 32 bits.  W <= taps * rad <= 128 * max(n_src, n_out), D < 2^44, N_c <= 255 * D < 2^52,
// M_c <= 255 * 255 * D < 2^60: the sums are 64-bit, each tap one 32 x 32 -> 64 multiply-add.  Positions on the line are 64-bit
// (2 * n_src * n_out may pass 2^32).
//
// The split: the columns with a weight are shared by L = 1 << lg <= 16 neighbouring lanes, c = ceil(taps / L) <= 4 columns each; work item
// (Y * ow + X) * L + l is lane l's share: the columns [k0 + l*c, + c) with a weight, k0 = bilinear_first(X, cw, ow), in every row with a weight.
// A lane also adds up its column weights (wx) and the row weights it walks (wy): the lanes' wx add up to Wx(X), the wy of lane 0 - whose
// first column always has a weight - is Wy(Y).
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_resize.hip) and - by tests/host/bilinear_host.cpp only - for the host, where the functor checks and counts every access.
#pragma once
#include <stdint.h>

#include "qoi_resize_core.h"

namespace qoimi {

constexpr uint32_t kBilinearMaxRatio = 32;
constexpr uint64_t kBilinearMaxArea = 1ull << 30;   // max(cw, ow) * max(rh, oh) stays below it
constexpr uint32_t kBilinearMaxCols = 4;            // 64 taps over 16 lanes

// v: the sums of resize_pixel; wx: sum of this lane's column weights; wy: sum of the row weights this lane walked
struct BilinearSums { ResizeSums v; uint64_t wx, wy; };

QOIMI_RESIZE_HD uint32_t bilinear_rad(uint32_t n_src, uint32_t n_out) { return 2u * (n_src > n_out ? n_src : n_out); }

// The first source sample with a weight for output sample Z: the smallest k >= 0 with (2k+1) * n_out > (2Z+1) * n_src - rad, which is
// floor(((2Z+1) * n_src + n_out - rad) / (2 * n_out)) where that numerator is positive and 0 else (at Z = 0 it is negative when reducing).
QOIMI_RESIZE_HD uint32_t bilinear_first(uint32_t Z, uint32_t n_src, uint32_t n_out) {
    const uint64_t a = (2ull * Z + 1u) * n_src + n_out, rad = bilinear_rad(n_src, n_out);
    return a > rad ? (uint32_t)resize_div(a - rad, 2ull * n_out) : 0u;
}

// t for an output centre o = (2Z+1) * n_src and source sample k (the caller keeps k below n_src)
QOIMI_RESIZE_HD uint32_t bilinear_tent(uint64_t o, uint32_t k, uint32_t n_out, uint32_t rad) {
    const uint64_t c = (2ull * k + 1u) * n_out, d = o > c ? o - c : c - o;
    return d < rad ? (uint32_t)(rad - d) : 0u;
}

// An upper bound of the source columns with a weight for one output column: ceil(rad / n_out).
QOIMI_RESIZE_HD uint32_t bilinear_taps(uint32_t n_src, uint32_t n_out) {
    return n_src <= n_out ? 2u : (uint32_t)((2ull * n_src + n_out - 1u) / n_out);
}

// How an output pixel's columns are split over lanes: lg = log2(L), c = columns per lane (at most 4 under the cap of 32).
QOIMI_RESIZE_HD void bilinear_split(uint32_t cw, uint32_t ow, uint32_t& lg, uint32_t& c) {
    const uint32_t t = bilinear_taps(cw, ow);
    lg = 0;
    while (lg < kResizeMaxLg && ((t + (1u << lg) - 1u) >> lg) > kBilinearMaxCols) ++lg;
    c = (t + (1u << lg) - 1u) >> lg;
}

// Tiles of kResizeThreads work items of an item (ow * oh * L of them); an accepted item has fewer than 2^30 output pixels.
QOIMI_RESIZE_HD uint64_t bilinear_tiles(uint32_t cw, uint32_t ow, uint32_t oh) {
    uint32_t lg, c;
    bilinear_split(cw, ow, lg, c);
    return ((((uint64_t)ow * oh) << lg) + kResizeThreads - 1u) / kResizeThreads;
}

// Lane l's share of output pixel (X, Y) of the unflipped result: c columns from k0 + l * c (lg, c: bilinear_split), every row with a weight.
// Only pixels with a weight are loaded: columns below cw, rows below rh of the rectangle.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD void bilinear_lane(const Mem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t c, BilinearSums& s) {
    resize_zero(s.v);
    s.wx = 0u; s.wy = 0u;
    const uint32_t radx = bilinear_rad(g.cw, g.ow), rady = bilinear_rad(g.rh, g.oh);
    const uint64_t ox = (2ull * X + 1u) * g.cw, oy = (2ull * Y + 1u) * g.rh;
    const uint32_t k0 = bilinear_first(X, g.cw, g.ow) + l * c;
    uint32_t wx[kBilinearMaxCols];
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < kBilinearMaxCols; ++j) {
        wx[j] = (j < c && k0 + j < g.cw) ? bilinear_tent(ox, k0 + j, g.ow, radx) : 0u;
        s.wx += wx[j];
    }
    if (wx[0] == 0u) return;                                   // (the weights of a pixel's columns are contiguous: nothing is left for this lane)
    for (uint32_t r = bilinear_first(Y, g.rh, g.oh); r < g.rh; ++r) {
        const uint32_t wy = bilinear_tent(oy, r, g.oh, rady);
        if (wy == 0u) break;                                   // (the first row has a weight; the rows with one are contiguous)
        s.wy += wy;
        const uint64_t at = (uint64_t)(g.y + r) * g.w + g.x + k0;
        QOIMI_RESIZE_UNROLL
        for (uint32_t j = 0; j < kBilinearMaxCols; ++j) {
            if (wx[j] == 0u) continue;
            resize_tap<WEIGHTED>(s.v, mem.load(at + j), wy * wx[j]);   // (the weight is below 2^32)
        }
    }
}

// D(X, Y) from the sums of a pixel: wx added over its lanes, wy of lane 0
QOIMI_RESIZE_HD uint64_t bilinear_divisor(const BilinearSums& s) { return s.wx * s.wy; }

// The sums of pixel (X, Y) divided by D and stored at its place in the output at q (qoi_resize_core.h: resize_store).
template <class Mem>
QOIMI_RESIZE_HD void bilinear_finish(const Mem& mem, const ResizeGeom& g, uint64_t q, uint32_t och, bool weighted, uint32_t X, uint32_t Y, const BilinearSums& s) {
    resize_store(mem, g, q, och, X, Y, resize_pixel(s.v, bilinear_divisor(s), weighted));
}

}  // namespace qoimi

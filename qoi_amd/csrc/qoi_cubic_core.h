// qoi_cubic_core.h — the arithmetic of qoimi_decode_tensors with QOIMI_FILTER_BICUBIC: the cubic weight, the first source sample that may have
// one, the normalisation of an output column's or row's weights to 15 fractional bits that sum exactly, which columns and rows a tile
// normalises, one lane's signed sums over its share of a pixel, and the sums of a pixel to its clamped bytes (the stores are a sink's:
// qoi_tensor_core.h).
//
// The definition (normative; qoi_amd/bicubic.py states it in Python).  A rectangle cw x rh at (x, y) of an image staged as rows of w pixels of 4
// bytes is resampled to ow x oh pixels.  One axis, n_src samples to n_out, on a line of length 2 * n_src * n_out: source sample k has its centre
// at (2k + 1) * n_out, output sample X at (2X + 1) * n_src; u = 2 * max(n_src, n_out); for 0 <= k < n_src, d = |(2X+1) * n_src - (2k+1) * n_out| and
//   c(X, k) = 3d^3 - 5u d^2 + 2u^3 = (d - u)(3d^2 - 2ud - 2u^2)          for d <= u
//   c(X, k) = -d^3 + 5u d^2 - 8u^2 d + 4u^3 = -(d - u)(d - 2u)^2          for u < d < 2u
//   c(X, k) = 0                                                           from 2u on
// - 2u^3 times Keys' kernel with a = -1/2 at d / u.  W(X) = sum_k c(X, k) > 0 (samples outside the rectangle do not exist: the weights are
// renormalised, not clamped).  q(X, k) = (c(X, k) * 2^15 + W/2) / W, every division floors; the deficit 2^15 - sum_k q(X, k) is added to
// the tap with the largest c, the lowest such k on a tie: sum_k q(X, k) = 2^15.  qx from (cw, ow), qy from (rh, oh).  N_c is the sum of
// qy * qx * channel c over the rectangle, M_c the sum of qy * qx * channel c * alpha (c = 0..2) - signed.
//   PLAIN           every channel is clamp((N_c + 2^29) >> 30, 0, 255) - the shift floors; one rounding, no intermediate
//   ALPHA_WEIGHTED  alpha is the PLAIN value; with A = N_3 > 0 the colours are clamp((M_c + A/2) / A, 0, 255), else the PLAIN value
// Pixel (X, Y) of that result goes to pixel (FLIP_X ? ow - 1 - X : X, FLIP_Y ? oh - 1 - Y : Y) of the output.
// cw <= 16 * ow, rh <= 16 * oh, max(cw, ow) <= 16384 and max(rh, oh) <= 16384.  The samples with a weight lie in an open interval of length
// 4u and are 2 * n_out apart: at most ceil(2u / n_out) of them - 4 when enlarging, up to 64 when reducing (cubic_taps).  u <= 2^15 and d < 2u
// where c is evaluated: a factor of c is below 2^33, |c| <= 2u^3 <= 2^46, c * 2^15 < 2^62; at most 33 samples have c > 0, so W < 2^52 - a
// double holds it exactly.  -2^13 <= q <= 5 * 2^13 (qoi_amd/bicubic.py: why, and asserted there): q + 2^13 is kept in 16 bits, qy * qx in
// 32; sum |q| <= 3 * 2^14 per axis, so |N_c| < 2^40 and |M_c| < 2^48: the sums are 64-bit two's complement in ResizeSums.  Positions on the
// line are below 2^29: 32 bits.
//
// The split is the tent filter's with this filter's taps: the columns that may have a weight are shared by L = 1 << lg <= 16 neighbouring
// lanes, c = ceil(taps / L) <= 4 columns each; work item (Y * ow + X) * L + l is lane l's share: the columns [k0 + l*c, + c) with q != 0,
// k0 = cubic_first(X, cw, ow), in every row with q != 0.
//
// A tile of kResizeThreads work items holds P = kResizeThreads >> lg consecutive output pixels.  Before its lanes run, the weights of every
// output column and row it holds are normalised ONCE (cubic_norm, one work item per column or row) into two tables of 16-bit entries
// q + kCubicBias: sx = c << lg entries per column, sy = cubic_taps(rh, oh) per row, entry j being sample first + j (0 behind the last sample).
// The columns: all ow of them where ow <= P (then ow * sx <= 1024), else that of each of the tile's pixels (P * sx <= 1024); the rows: those
// the pixels lie in - at most P of them (P * sy <= 16384).
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword), compiled for the device by hipcc (qoi_cubic.hip: the tables
// are LDS) and - by tests/host/bicubic_host.cpp only - for the host, where the functor checks and counts every access.
#pragma once
#include <stdint.h>

#include "qoi_resize_core.h"

namespace qoimi {

constexpr uint32_t kCubicMaxRatio = 16;
constexpr uint32_t kCubicMaxSize = 16384;          // max(cw, ow) and max(rh, oh) stay at or below it
constexpr uint32_t kCubicMaxCols = 4;              // 64 taps over 16 lanes
constexpr int32_t kCubicOne = 1 << 15;             // the weights of an output sample add up to it
constexpr int32_t kCubicBias = 1 << 13;            // a table entry is q + kCubicBias, 0 .. 6 * 2^13
constexpr uint32_t kCubicColSlots = 1024;          // entries of a tile's column table
constexpr uint32_t kCubicRowSlots = 16384;         // ... of its row table

QOIMI_RESIZE_HD uint32_t cubic_unit(uint32_t n_src, uint32_t n_out) { return 2u * (n_src > n_out ? n_src : n_out); }

// The first source sample that may have a weight for output sample Z under a kernel that is 0 from `lobes` * u on (2: this filter, 3:
// qoi_lanczos_core.h): the smallest k >= 0 with (2k+1) * n_out > (2Z+1) * n_src - lobes * u, which is
// floor(((2Z+1) * n_src + n_out - lobes * u) / (2 * n_out)) where that numerator is positive and 0 else.
QOIMI_RESIZE_HD uint32_t filter_first(uint32_t Z, uint32_t n_src, uint32_t n_out, uint32_t lobes) {
    const uint32_t a = (2u * Z + 1u) * n_src + n_out, ul = lobes * cubic_unit(n_src, n_out);
    return a > ul ? (a - ul) / (2u * n_out) : 0u;
}
QOIMI_RESIZE_HD uint32_t cubic_first(uint32_t Z, uint32_t n_src, uint32_t n_out) { return filter_first(Z, n_src, n_out, 2u); }

// c for an output centre o = (2Z+1) * n_src and source sample k (the caller keeps k below n_src)
QOIMI_RESIZE_HD int64_t cubic_weight(uint32_t o, uint32_t k, uint32_t n_out, uint32_t u) {
    const uint32_t s = (2u * k + 1u) * n_out, du = o > s ? o - s : s - o;
    if (du >= 2u * u) return 0;
    const int64_t d = du, U = u;
    if (du <= u) return (d - U) * (3 * d * d - 2 * U * d - 2 * U * U);
    return -(d - U) * ((d - 2 * U) * (d - 2 * U));
}

// An upper bound of the source samples with a weight for one output sample: ceil(2u / n_out).
QOIMI_RESIZE_HD uint32_t cubic_taps(uint32_t n_src, uint32_t n_out) {
    return n_src <= n_out ? 4u : (4u * n_src + n_out - 1u) / n_out;
}

// How the t columns of an output pixel are split over lanes: lg = log2(L), c = columns per lane (at most max_cols under the cap of 16).
QOIMI_RESIZE_HD void filter_split(uint32_t t, uint32_t max_cols, uint32_t& lg, uint32_t& c) {
    lg = 0;
    while (lg < kResizeMaxLg && ((t + (1u << lg) - 1u) >> lg) > max_cols) ++lg;
    c = (t + (1u << lg) - 1u) >> lg;
}
QOIMI_RESIZE_HD void cubic_split(uint32_t cw, uint32_t ow, uint32_t& lg, uint32_t& c) { filter_split(cubic_taps(cw, ow), kCubicMaxCols, lg, c); }

// Tiles of kResizeThreads work items of an item (ow * oh << lg of them); an accepted item has at most 2^28 output pixels.
QOIMI_RESIZE_HD uint64_t split_tiles(uint32_t lg, uint32_t ow, uint32_t oh) {
    return ((((uint64_t)ow * oh) << lg) + kResizeThreads - 1u) / kResizeThreads;
}
QOIMI_RESIZE_HD uint64_t cubic_tiles(uint32_t cw, uint32_t ow, uint32_t oh) {
    uint32_t lg, c;
    cubic_split(cw, ow, lg, c);
    return split_tiles(lg, ow, oh);
}

// floor(n / W) for 0 < W < 2^53 and |n / W| < 2^17: the quotient of two doubles is off by far less than 1, so one step either way mends it
// (the result is exact whatever the rounding of the division).
QOIMI_RESIZE_HD int32_t cubic_quot(int64_t n, int64_t W) {
    int64_t q = (int64_t)((double)n / (double)W);
    const int64_t r = n - q * W;
    if (r < 0) --q;
    else if (r >= W) ++q;
    return (int32_t)q;
}

// The weights of output sample Z, normalised: tab[j] = q(Z, first + j) + kCubicBias for j < slots (slots >= cubic_taps(n_src, n_out);
// kCubicBias where there is no sample or no weight).
QOIMI_RESIZE_HD void cubic_norm(uint32_t Z, uint32_t n_src, uint32_t n_out, uint32_t slots, uint16_t* tab) {
    const uint32_t u = cubic_unit(n_src, n_out), o = (2u * Z + 1u) * n_src, k0 = cubic_first(Z, n_src, n_out);
    const uint32_t t = cubic_taps(n_src, n_out), n = n_src - k0 < t ? n_src - k0 : t;
    int64_t W = 0, best = 0;
    uint32_t jbest = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const int64_t c = cubic_weight(o, k0 + j, n_out, u);
        W += c;
        if (c > best) { best = c; jbest = j; }                 // (the largest c is positive; the lowest j keeps a tie)
    }
    int32_t sum = 0;
    for (uint32_t j = 0; j < slots; ++j) {
        const int32_t q = j < n ? cubic_quot(cubic_weight(o, k0 + j, n_out, u) * kCubicOne + W / 2, W) : 0;
        sum += q;
        tab[j] = (uint16_t)(q + kCubicBias);
    }
    tab[jbest] = (uint16_t)(tab[jbest] + (kCubicOne - sum));
}

// What a tile normalises.  o0: its first output pixel, px: its pixels; nx columns of sx entries - column slot i is output column
// cubic_tile_column(i), pixel o at column X reads slot cubic_tile_slot(o, X) -, ny rows of sy entries from output row Y0.
// (The bookkeeping does not know the filter: table_tile takes sy, the entries of a row - qoi_lanczos_core.h uses it with its own.)
struct CubicTile { uint64_t o0; uint32_t px, X0, Y0, nx, ny, sx, sy, wrap; };

QOIMI_RESIZE_HD CubicTile table_tile(const ResizeGeom& g, uint32_t lg, uint32_t c, uint32_t sy, uint64_t tile) {
    CubicTile t;
    const uint32_t per = kResizeThreads >> lg;
    const uint64_t all = (uint64_t)g.ow * g.oh;
    t.o0 = tile * per;
    t.px = all - t.o0 < per ? (uint32_t)(all - t.o0) : per;
    t.Y0 = (uint32_t)resize_div(t.o0, g.ow);
    t.X0 = (uint32_t)(t.o0 - (uint64_t)t.Y0 * g.ow);
    t.ny = (uint32_t)resize_div(t.o0 + t.px - 1u, g.ow) - t.Y0 + 1u;
    t.wrap = g.ow > per ? 1u : 0u;
    t.nx = t.wrap ? t.px : g.ow;
    t.sx = c << lg;
    t.sy = sy;
    return t;
}
QOIMI_RESIZE_HD CubicTile cubic_tile(const ResizeGeom& g, uint32_t lg, uint32_t c, uint64_t tile) { return table_tile(g, lg, c, cubic_taps(g.rh, g.oh), tile); }

QOIMI_RESIZE_HD uint32_t cubic_tile_column(const CubicTile& t, const ResizeGeom& g, uint32_t i) {
    if (!t.wrap) return i;
    return t.X0 + i < g.ow ? t.X0 + i : t.X0 + i - g.ow;       // (fewer pixels than a row: the tile wraps once at most)
}

QOIMI_RESIZE_HD uint32_t cubic_tile_slot(const CubicTile& t, uint64_t o, uint32_t X) { return t.wrap ? (uint32_t)(o - t.o0) : X; }

// Work item i < nx + ny of the normalisation of a tile: one column into qx or one row into qy.
QOIMI_RESIZE_HD void cubic_tile_norm(const CubicTile& t, const ResizeGeom& g, uint32_t i, uint16_t* qx, uint16_t* qy) {
    if (i < t.nx) cubic_norm(cubic_tile_column(t, g, i), g.cw, g.ow, t.sx, qx + i * t.sx);
    else cubic_norm(t.Y0 + (i - t.nx), g.rh, g.oh, t.sy, qy + (i - t.nx) * t.sy);
}

// One tap: staged pixel px with the signed weight w = qy * qx into the sums (two's complement in ResizeSums).
template <bool WEIGHTED>
QOIMI_RESIZE_HD void cubic_tap(ResizeSums& s, uint32_t px, int64_t w) {
    const int32_t al = (int32_t)(px >> 24);
    s.S[0] += (uint64_t)(w * (int32_t)(px & 255u)); s.S[1] += (uint64_t)(w * (int32_t)((px >> 8) & 255u));
    s.S[2] += (uint64_t)(w * (int32_t)((px >> 16) & 255u)); s.S[3] += (uint64_t)(w * al);
    if (WEIGHTED) {
        s.W[0] += (uint64_t)(w * ((int32_t)(px & 255u) * al)); s.W[1] += (uint64_t)(w * ((int32_t)((px >> 8) & 255u) * al));
        s.W[2] += (uint64_t)(w * ((int32_t)((px >> 16) & 255u) * al));
    }
}

// Lane l's share of output pixel (X, Y) of the unflipped result: c columns from k0 + l * c, every row.  qx: the sx entries of the pixel's
// column, qy: the sy entries of its row, each q + BIAS.  Only pixels with a weight are loaded: q is 0 for columns from cw and rows from rh on.
// LOBES: filter_first's; COLS: the most columns of a lane; Prod: the type qy * qx is formed in.
template <bool WEIGHTED, uint32_t LOBES, uint32_t COLS, int32_t BIAS, class Prod, class Mem>
QOIMI_RESIZE_HD void filter_lane(const Mem& mem, const ResizeGeom& g, const uint16_t* qx, const uint16_t* qy, uint32_t sy, uint32_t X, uint32_t Y,
                                 uint32_t l, uint32_t c, ResizeSums& s) {
    resize_zero(s);
    const uint32_t k0 = filter_first(X, g.cw, g.ow, LOBES) + l * c;
    int32_t wx[COLS], any = 0;
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < COLS; ++j) {
        wx[j] = j < c ? (int32_t)qx[l * c + j] - BIAS : 0;
        any |= wx[j];
    }
    if (any == 0) return;
    const uint64_t at0 = (uint64_t)(g.y + filter_first(Y, g.rh, g.oh, LOBES)) * g.w + g.x + k0;
    for (uint32_t i = 0; i < sy; ++i) {
        const int32_t wy = (int32_t)qy[i] - BIAS;
        if (wy == 0) continue;                                 // (a weight may be 0 inside the support: d = u)
        const uint64_t at = at0 + (uint64_t)i * g.w;
        QOIMI_RESIZE_UNROLL
        for (uint32_t j = 0; j < COLS; ++j) {
            if (wx[j] == 0) continue;
            cubic_tap<WEIGHTED>(s, mem.load(at + j), (Prod)wy * wx[j]);
        }
    }
}

// ... of this filter: |qy * qx| <= 25 * 2^26 < 2^31
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD void cubic_lane(const Mem& mem, const ResizeGeom& g, const uint16_t* qx, const uint16_t* qy, uint32_t sy, uint32_t X, uint32_t Y,
                                uint32_t l, uint32_t c, ResizeSums& s) {
    filter_lane<WEIGHTED, 2u, kCubicMaxCols, kCubicBias, int32_t>(mem, g, qx, qy, sy, X, Y, l, c, s);
}

QOIMI_RESIZE_HD uint32_t cubic_clamp(int64_t v) { return v < 0 ? 0u : (v > 255 ? 255u : (uint32_t)v); }

// floor((m + a/2) / a) for a > 0, m of either sign
QOIMI_RESIZE_HD int64_t cubic_div_round(int64_t m, int64_t a) {
    const int64_t n = m + a / 2;
    return n >= 0 ? (int64_t)resize_div((uint64_t)n, (uint64_t)a) : -(int64_t)resize_div((uint64_t)(-n) + (uint64_t)a - 1u, (uint64_t)a);
}

// The output pixel as r | g << 8 | b << 16 | a << 24 from the sums over all its taps.  weighted: QOIMI_RESIZE_ALPHA_WEIGHTED (the caller
// passes false for 3 output channels).
QOIMI_RESIZE_HD uint32_t cubic_pixel(const ResizeSums& s, bool weighted) {
    const int64_t half = (int64_t)1 << 29, A = (int64_t)s.S[3];
    const uint32_t a = cubic_clamp((A + half) >> 30);
    uint32_t c[3];
    if (weighted && A > 0) {
        for (int k = 0; k < 3; ++k) c[k] = cubic_clamp(cubic_div_round((int64_t)s.W[k], A));
    } else {
        for (int k = 0; k < 3; ++k) c[k] = cubic_clamp(((int64_t)s.S[k] + half) >> 30);
    }
    return c[0] | (c[1] << 8) | (c[2] << 16) | (a << 24);
}

}  // namespace qoimi

// qoi_lanczos_core.h — the arithmetic of qoimi_decode_tensors with QOIMI_FILTER_LANCZOS: the weight from the kernel table, the tap count and
// the lane split, and the normalisation of an output column's or row's weights to 15 fractional bits that sum exactly.  Everything else is
// qoi_cubic_core.h's by parameter: the first sample (filter_first with 3 lobes), the tile's bookkeeping (table_tile, cubic_tile_column,
// cubic_tile_slot), the quotient (cubic_quot), one lane's sums (filter_lane over cubic_tap) and the pixel (cubic_pixel).
//
// The definition (normative; qoi_amd/lanczos.py states it in Python).  Geometry, line, u, d, flips, PLAIN / ALPHA_WEIGHTED and the clamp as for
// the bicubic filter.  T[i] = round(2^30 * sinc(i / 1024) * sinc(i / 3072)), i = 0 .. 3072 (qoi_lanczos_table.h, generated).  c(X, k) = 0 for
// d >= 3u; else z = 1024 * d, i = z / u, r = z - i * u and c(X, k) = T[i] * (u - r) + T[i + 1] * r - u times the table interpolated linearly.
// W(X) = sum_k c(X, k) > 0, q(X, k) = (c(X, k) * 2^15 + W/2) / W, the deficit 2^15 - sum_k q to the tap with the largest c, the lowest k on
// a tie.  cw <= 16 * ow, rh <= 16 * oh, max(cw, ow) <= 16384 and max(rh, oh) <= 16384.
// Derived: at most ceil(3u / n_out) samples have a weight - 6 when enlarging, up to 96 when reducing (lanczos_taps); u <= 2^15 and d < 3u where
// c is evaluated: z < 2^27 and i <= 3071 (32 bits, inside the table); |T| <= 2^30 and (u - r) + r = u: |c| <= 2^45, c * 2^15 <= 2^60.
// Asserted by the model, not proven (qoi_amd/lanczos.py: over which geometries): 0 < W < 2^50 - cubic_quot's doubles hold it -;
// -2^14 <= q < 3 * 2^14, so q + kLanczosBias is kept in 16 bits (measured: -9362 .. 42130); sum |q| <= 2^16 per axis, so |N_c| < 2^40 and
// |M_c| < 2^48.  qy * qx does not fit 32 bits under these bounds: the lanes form it in 64.
//
// The split: the columns that may have a weight are shared by L = 1 << lg <= 16 neighbouring lanes, c = ceil(taps / L) <= 6 columns each.
// A tile of kResizeThreads work items holds P = kResizeThreads >> lg consecutive output pixels and first normalises the weights of every output
// column and row it holds ONCE (lanczos_tile_norm, one work item per column or row) into two tables of 16-bit entries q + kLanczosBias:
// sx = c << lg entries per column, sy = lanczos_taps(rh, oh) per row.  The worst splits: the columns take P * sx = kResizeThreads * c <= 1536
// entries (3 KB; ow * sx <= P * sx where a tile holds all ow columns) - 16 pixels of 96 at lg = 4 -, the rows at most P * sy <= 256 * 96 =
// 24576 entries (48 KB: a tile of 256 one-lane pixels of a one-column output reduced by 16 in y).  51 KB of LDS: three workgroups per CU.
//
// Plain sequential code over a memory functor `Mem` and a table pointer, compiled for the device by hipcc (qoi_lanczos.hip: the kernel table is
// device memory, the weight tables LDS) and - by tests/host/lanczos_host.cpp only - for the host.
#pragma once
#include <stdint.h>

#include "qoi_cubic_core.h"

namespace qoimi {

constexpr uint32_t kLanczosLobes = 3;
constexpr uint32_t kLanczosSteps = 1024;           // table entries per unit of d / u
constexpr uint32_t kLanczosEntries = kLanczosLobes * kLanczosSteps + 1u;
constexpr uint32_t kLanczosMaxRatio = 16;
constexpr uint32_t kLanczosMaxSize = 16384;        // max(cw, ow) and max(rh, oh) stay at or below it
constexpr uint32_t kLanczosMaxCols = 6;            // 96 taps over 16 lanes
constexpr int32_t kLanczosBias = 1 << 14;          // a table entry is q + kLanczosBias, 0 .. 2^16 - 1
constexpr uint32_t kLanczosColSlots = 1536;        // entries of a tile's column table
constexpr uint32_t kLanczosRowSlots = 24576;       // ... of its row table

// An upper bound of the source samples with a weight for one output sample: ceil(3u / n_out).
QOIMI_RESIZE_HD uint32_t lanczos_taps(uint32_t n_src, uint32_t n_out) {
    return n_src <= n_out ? 2u * kLanczosLobes : (2u * kLanczosLobes * n_src + n_out - 1u) / n_out;
}

QOIMI_RESIZE_HD void lanczos_split(uint32_t cw, uint32_t ow, uint32_t& lg, uint32_t& c) { filter_split(lanczos_taps(cw, ow), kLanczosMaxCols, lg, c); }

QOIMI_RESIZE_HD uint64_t lanczos_tiles(uint32_t cw, uint32_t ow, uint32_t oh) {
    uint32_t lg, c;
    lanczos_split(cw, ow, lg, c);
    return split_tiles(lg, ow, oh);
}

QOIMI_RESIZE_HD CubicTile lanczos_tile(const ResizeGeom& g, uint32_t lg, uint32_t c, uint64_t tile) {
    return table_tile(g, lg, c, lanczos_taps(g.rh, g.oh), tile);
}

// c for an output centre o = (2Z+1) * n_src and source sample k (the caller keeps k below n_src); T: the kLanczosEntries of the kernel table
QOIMI_RESIZE_HD int64_t lanczos_weight(const int32_t* T, uint32_t o, uint32_t k, uint32_t n_out, uint32_t u) {
    const uint32_t s = (2u * k + 1u) * n_out, d = o > s ? o - s : s - o;
    if (d >= kLanczosLobes * u) return 0;
    const uint32_t z = kLanczosSteps * d, i = z / u, r = z - i * u;
    return (int64_t)T[i] * (int32_t)(u - r) + (int64_t)T[i + 1u] * (int32_t)r;
}

// The weights of output sample Z, normalised: tab[j] = q(Z, first + j) + kLanczosBias for j < slots (slots >= lanczos_taps(n_src, n_out);
// kLanczosBias where there is no sample or no weight).
QOIMI_RESIZE_HD void lanczos_norm(const int32_t* T, uint32_t Z, uint32_t n_src, uint32_t n_out, uint32_t slots, uint16_t* tab) {
    const uint32_t u = cubic_unit(n_src, n_out), o = (2u * Z + 1u) * n_src, k0 = filter_first(Z, n_src, n_out, kLanczosLobes);
    const uint32_t t = lanczos_taps(n_src, n_out), n = n_src - k0 < t ? n_src - k0 : t;
    int64_t W = 0, best = 0;
    uint32_t jbest = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const int64_t c = lanczos_weight(T, o, k0 + j, n_out, u);
        W += c;
        if (c > best) { best = c; jbest = j; }                 // (the largest c is positive; the lowest j keeps a tie)
    }
    int32_t sum = 0;
    for (uint32_t j = 0; j < slots; ++j) {
        const int32_t q = j < n ? cubic_quot(lanczos_weight(T, o, k0 + j, n_out, u) * kCubicOne + W / 2, W) : 0;
        sum += q;
        tab[j] = (uint16_t)(q + kLanczosBias);
    }
    tab[jbest] = (uint16_t)(tab[jbest] + (kCubicOne - sum));
}

// Work item i < nx + ny of the normalisation of a tile: one column into qx or one row into qy.
QOIMI_RESIZE_HD void lanczos_tile_norm(const int32_t* T, const CubicTile& t, const ResizeGeom& g, uint32_t i, uint16_t* qx, uint16_t* qy) {
    if (i < t.nx) lanczos_norm(T, cubic_tile_column(t, g, i), g.cw, g.ow, t.sx, qx + i * t.sx);
    else lanczos_norm(T, t.Y0 + (i - t.nx), g.rh, g.oh, t.sy, qy + (i - t.nx) * t.sy);
}

// Lane l's share of output pixel (X, Y): filter_lane with this filter's support, columns and bias, qy * qx in 64 bits.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD void lanczos_lane(const Mem& mem, const ResizeGeom& g, const uint16_t* qx, const uint16_t* qy, uint32_t sy, uint32_t X, uint32_t Y,
                                  uint32_t l, uint32_t c, ResizeSums& s) {
    filter_lane<WEIGHTED, kLanczosLobes, kLanczosMaxCols, kLanczosBias, int64_t>(mem, g, qx, qy, sy, X, Y, l, c, s);
}

}  // namespace qoimi

// qoi_mode_core.h — the arithmetic of qoimi_decode_tensors with QOIMI_FILTER_MODE: the cell of source pixels an output pixel looks at, how
// that cell is split over the lanes that share the output pixel, what a lane learns about its pixels from another lane's, the packed word
// whose maximum is the winner, and the pixel that word stands for.  A majority vote, not an average and not a selection: for REDUCING label
// maps (segmentation masks, instance ids, palette indices), where QOIMI_FILTER_NEAREST looks at one pixel of each cell.
//
// The definition (normative; qoi_amd/mode.py: mode states it in Python).  A rectangle cw x rh at (x, y) of an image staged as rows of w
// pixels of 4 bytes is reduced to ow x oh pixels.  All arithmetic is integer, every division floors.  On an axis of n_src source and n_out
// output samples the cell of output sample Z is [first(Z), first(Z + 1)) with
//   first(Z) = (2 * Z * n_src + n_out - 1) / (2 * n_out)
// - the source samples whose centre (2k + 1) * n_out lies in [2Z * n_src, (2Z + 2) * n_src), on the line of qoi_nearest_core.h -; an empty
// cell (only when enlarging on that axis) is replaced by the single sample nearest_index(Z, n_src, n_out).  Output pixel (X, Y) of the
// unflipped result looks at the pixels in columns cell(X) x rows cell(Y).  A pixel votes as a whole, all four bytes as staged.  The count of
// a value is the number of pixels equal to it, the winners are the values with the largest count.  One winner is the output; of several
// the pixel at (nearest_index(X), nearest_index(Y)) if it is a winner, else the winner with the lowest key = r << 24 | g << 16 | b << 8 | a.
// There are no modes: PLAIN and ALPHA_WEIGHTED give the same bytes.  The flips and the drop of alpha for och 3 are the sink's.
// Bounds.  cw <= kModeMaxRatio * ow, rh <= kModeMaxRatio * oh: a cell has at most ceil(n_src / n_out) <= 16 samples per axis, 256 pixels.
// cw, rh, ow, oh <= kModeMaxSize = 2^14: 2 * Z * n_src + n_out - 1 < 2^29 + 2^14 for Z <= n_out - first is one 32-bit division; ow * oh <=
// 2^28 and L <= 2^6, so a work item's number within its item is below 2^34: 64-bit, as the tile walk keeps it.
//
// The lanes.  L = 2^lg neighbouring lanes share an output pixel: work item i of an item is lane i % L of output pixel o = i / L, which is
// (o % ow, o / ow); a tile is kResizeThreads consecutive work items.  mode_split chooses lg - the item's, so that every lane of a workgroup
// takes the same steps - as the smallest for which the item's largest cell, ceil(cw / ow) x ceil(rh / oh) pixels, leaves a lane at most
// kModeHold = 4 of them.  Of a cell of nx x ny pixels lane l holds the pixels p = l, l + L, l + 2L, l + 3L below nx * ny, p being column
// p % nx and row p / nx of the cell: n of them, the first n of its four registers - a count, not a sentinel: pixels are arbitrary words.
// The vote.  Every lane meets every lane of its group once (its own included) and adds to each of its pixels' counts the pixels of the other
// that equal it (mode_meet): after L meetings a held pixel knows its count.  The lane's best pixel and then the group's is the maximum of
// the word count << 33 | (is the centre pixel) << 32 | ~key (mode_word): the largest count, then the centre, then the lowest key.  A lane
// without pixels has the word 0, below every real one (a count is at least 1).  mode_pick turns the word back into the pixel.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store2 / store4(address, value)), compiled for the
// device by hipcc (qoi_mode.hip, which moves pixels between lanes) and - by tests/host/mode_host.cpp only - for the host, where the lanes
// are walked in a loop and the functor checks every access.
#pragma once
#include <stdint.h>

#include "qoi_nearest_core.h"

namespace qoimi {

constexpr uint32_t kModeMaxRatio = 16;        // a rectangle is reduced by at most this in an axis: a cell is at most 16 x 16
constexpr uint32_t kModeMaxSize = 16384;      // no width or height of a rectangle or an output above it
constexpr uint32_t kModeHold = 4;             // pixels a lane holds at most
constexpr uint32_t kModeMaxLg = 6;            // 64 lanes per output pixel at most: a wavefront

// The first source sample whose centre is not below the lower end of output sample Z's extent, Z <= n_out
QOIMI_RESIZE_HD uint32_t mode_first(uint32_t Z, uint32_t n_src, uint32_t n_out) { return (2u * Z * n_src + n_out - 1u) / (2u * n_out); }

// The range [lo, lo + n) of source samples output sample Z looks at: its cell, or the nearest sample if the cell is empty
QOIMI_RESIZE_HD void mode_range(uint32_t Z, uint32_t n_src, uint32_t n_out, uint32_t& lo, uint32_t& n) {
    lo = mode_first(Z, n_src, n_out);
    n = mode_first(Z + 1u, n_src, n_out) - lo;
    if (n == 0u) { lo = nearest_index(Z, n_src, n_out); n = 1u; }
}

// How an output pixel's cell is split over lanes: lg = log2(L), c = pixels per lane at most (1..kModeHold), for sizes within the limits
QOIMI_RESIZE_HD void mode_split(uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, uint32_t& lg, uint32_t& c) {
    const uint64_t cells = (((uint64_t)cw + ow - 1u) / ow) * (((uint64_t)rh + oh - 1u) / oh);
    lg = 0;
    while (lg < kModeMaxLg && ((cells + (1u << lg) - 1u) >> lg) > kModeHold) ++lg;
    const uint64_t per = (cells + (1u << lg) - 1u) >> lg;
    c = per > kModeHold ? kModeHold : (uint32_t)per;                // (above the limits: no call accepts the item)
}

// Tiles of kResizeThreads work items of an item (ow * oh * L of them); 2^32 for an output no call accepts (2^40 pixels or more).
QOIMI_RESIZE_HD uint64_t mode_tiles(uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh) {
    uint32_t lg, c;
    mode_split(cw, rh, ow, oh, lg, c);
    const uint64_t px = (uint64_t)ow * oh;
    if (px >= (1ull << 40)) return 1ull << 32;
    return ((px << lg) + kResizeThreads - 1u) / kResizeThreads;
}

// What a lane holds of its output pixel's cell: v[0..n), and which of them is the centre pixel (kModeHold: none of this lane's)
struct ModeHeld { uint32_t v[kModeHold]; uint32_t n, centre; };

QOIMI_RESIZE_HD void mode_none(ModeHeld& h) {
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < kModeHold; ++j) h.v[j] = 0u;
    h.n = 0u; h.centre = kModeHold;
}

// Lane l of 2^lg of output pixel (X, Y): its pixels loaded - aligned dwords of the staged image, inside the rectangle
template <class Mem>
QOIMI_RESIZE_HD void mode_hold(const Mem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t lg, ModeHeld& h) {
    uint32_t k0, nx, r0, ny;
    mode_range(X, g.cw, g.ow, k0, nx);
    mode_range(Y, g.rh, g.oh, r0, ny);
    const uint32_t pc = (nearest_index(Y, g.rh, g.oh) - r0) * nx + (nearest_index(X, g.cw, g.ow) - k0);   // the centre lies in the range
    mode_none(h);
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < kModeHold; ++j) {
        const uint32_t p = l + (j << lg);
        if (p < nx * ny) {
            const uint32_t pr = p / nx, pk = p - pr * nx;
            h.v[j] = mem.load((uint64_t)(g.y + r0 + pr) * g.w + g.x + k0 + pk);
            h.n = j + 1u;
            if (p == pc) h.centre = j;
        }
    }
}

// A meeting: count[j] of the lane's pixel j grows by the pixels of the other lane (ov[0..on)) that equal it.  Pixels the lane does not hold
// collect counts nobody reads.
QOIMI_RESIZE_HD void mode_meet(const ModeHeld& h, const uint32_t (&ov)[kModeHold], uint32_t on, uint32_t (&count)[kModeHold]) {
    QOIMI_RESIZE_UNROLL
    for (uint32_t i = 0; i < kModeHold; ++i) {
        const bool there = i < on;
        QOIMI_RESIZE_UNROLL
        for (uint32_t j = 0; j < kModeHold; ++j) count[j] += (there && ov[i] == h.v[j]) ? 1u : 0u;
    }
}

// r << 24 | g << 16 | b << 8 | a of the staged pixel r | g << 8 | b << 16 | a << 24, and back: the bytes reversed
QOIMI_RESIZE_HD uint32_t mode_key(uint32_t px) { return (px >> 24) | ((px >> 8) & 0xFF00u) | ((px << 8) & 0xFF0000u) | (px << 24); }

// The word whose maximum wins: the count (1..256), then the centre pixel, then the lowest key
QOIMI_RESIZE_HD uint64_t mode_word(uint32_t count, bool centre, uint32_t px) {
    return ((uint64_t)count << 33) | ((uint64_t)(centre ? 1u : 0u) << 32) | (uint32_t)~mode_key(px);
}

// The best word of a lane's own pixels; 0 for a lane that holds none
QOIMI_RESIZE_HD uint64_t mode_best(const ModeHeld& h, const uint32_t (&count)[kModeHold]) {
    uint64_t best = 0u;
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < kModeHold; ++j) {
        const uint64_t wd = mode_word(count[j], h.centre == j, h.v[j]);
        if (j < h.n && wd > best) best = wd;
    }
    return best;
}

// The pixel of a word
QOIMI_RESIZE_HD uint32_t mode_pick(uint64_t word) { return mode_key(~(uint32_t)word); }

}  // namespace qoimi

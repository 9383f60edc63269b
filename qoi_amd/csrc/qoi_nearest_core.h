// qoi_nearest_core.h — the arithmetic of qoimi_decode_tensors with QOIMI_FILTER_NEAREST: which output pixel a work item of a tile is, which
// source pixel of the rectangle that output pixel takes, the one load, and the hand-over to the sink.  Selection, not averaging: for label
// maps (segmentation masks, instance ids, palette indices), whose values must not be mixed.
//
// The definition (normative; qoi_amd/nearest.py: nearest states it in Python).  A rectangle cw x rh at (x, y) of an image staged as rows of w
// pixels of 4 bytes is sampled into ow x oh pixels.  All arithmetic is integer, every division floors.  Output pixel (X, Y) of the unflipped
// result is pixel (k, r) of the rectangle byte for byte, with
//   k = ((2X + 1) * cw) / (2 * ow),  r = ((2Y + 1) * rh) / (2 * oh)
// - on the line of length 2 * n_src * n_out that the tent filter uses (qoi_bilinear_core.h), where output sample X has its centre at
// (2X + 1) * n_src and source sample k covers [2k * n_out, (2k + 2) * n_out): the source pixel whose cell holds the output pixel's centre; a
// centre on the boundary of two cells belongs to the upper one.  (2X + 1) * cw <= (2 * ow - 1) * cw < 2 * ow * cw, so k < cw: nothing outside
// the rectangle is read.  There are no modes: PLAIN and ALPHA_WEIGHTED give the same bytes.  The flips are the sink's (g.flags).
// Bounds.  cw, rh, ow, oh <= kNearestMaxSize = 2^14: (2X + 1) * cw < 2^15 * 2^14 = 2^29 and 2 * ow <= 2^15 - the index is one 32-bit division;
// ow * oh <= 2^28, so a work item's number within its item is 32-bit.  There is no ratio limit: every output pixel is one load.
//
// The tiles: work item i of an item is output pixel (i % ow, i / ow) of the unflipped result, a tile is kResizeThreads consecutive work
// items: consecutive lanes hold consecutive X of a row (one lane per pixel: nothing is summed, there is no lane split).
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store2 / store4(address, value)), compiled for the
// device by hipcc (qoi_nearest.hip) and - by tests/host/nearest_host.cpp only - for the host, where the functor checks every access.
#pragma once
#include <stdint.h>

#include "qoi_resize_core.h"

namespace qoimi {

constexpr uint32_t kNearestMaxSize = 16384;   // no width or height of a rectangle or an output above it

// One lane per output pixel, one column each (the fields of ResizeEntry::cfg the other filters fill from their splits)
QOIMI_RESIZE_HD void nearest_split(uint32_t, uint32_t, uint32_t& lg, uint32_t& c) { lg = 0u; c = 1u; }

// Tiles of kResizeThreads work items of an item (ow * oh of them); 2^32 for an output no call accepts (2^40 pixels or more).
QOIMI_RESIZE_HD uint64_t nearest_tiles(uint32_t, uint32_t ow, uint32_t oh) {
    const uint64_t px = (uint64_t)ow * oh;
    if (px >= (1ull << 40)) return 1ull << 32;
    return (px + kResizeThreads - 1u) / kResizeThreads;
}

// The source sample of output sample Z on an axis of n_src source and n_out output samples, both at most kNearestMaxSize
QOIMI_RESIZE_HD uint32_t nearest_index(uint32_t Z, uint32_t n_src, uint32_t n_out) { return ((2u * Z + 1u) * n_src) / (2u * n_out); }

// Work item `item` of the item with the geometry g: its pixel loaded - one aligned dword of the staged image - and handed to the sink, or
// nothing behind the last pixel.
template <class Mem, class Sink>
QOIMI_RESIZE_HD void nearest_work(const Mem& mem, const ResizeGeom& g, uint64_t q, uint32_t och, uint64_t item, const Sink& sink) {
    if (item >= (uint64_t)g.ow * g.oh) return;
    const uint32_t o = (uint32_t)item, Y = o / g.ow, X = o - Y * g.ow;
    const uint32_t k = nearest_index(X, g.cw, g.ow), r = nearest_index(Y, g.rh, g.oh);
    sink(mem, g, q, och, X, Y, mem.load((uint64_t)(g.y + r) * g.w + g.x + k));
}

}  // namespace qoimi

// qoi_table_tiles.h — the tile of the filters whose weights are normalised per output column and row (qoi_cubic.hip: tensor_cubic,
// qoi_lanczos.hip: tensor_lanczos): two phases with a barrier between them.  Phase 1: one work item per output column and row the tile holds
// normalises its weights into the two LDS tables; phase 2: every lane reads its column weights and walks its rows, the sums of a pixel's
// lanes are added by butterfly steps and lane 0 hands the clamped pixel to the sink.  A filter is a type with
//   tile(g, lg, c, tile) -> CubicTile          what the tile holds and the strides of its tables (qoi_cubic_core.h: table_tile)
//   norm(t, g, i, qx, qy)                      work item i < t.nx + t.ny of phase 1
//   lane<WEIGHTED>(mem, g, qx, qy, sy, X, Y, l, c, s)    lane l's share of pixel (X, Y) from the pixel's column and row entries
// Device only.
#pragma once
#include "qoi_gather_tiles.h"
#include "qoi_cubic_core.h"

namespace qoimi {

// One tile of an item: work items [tile * kResizeThreads, + kResizeThreads) as far as the item has them.
template <class Filter, bool WEIGHTED, class Sink>
__device__ __forceinline__ void table_tile_run(const GatherMem& mem, u64 q, const ResizeEntry& e, uint32_t tile, uint16_t* qx, uint16_t* qy, const Sink& sink) {
    const uint32_t lg = e.cfg & 255u, c = (e.cfg >> 8) & 255u, och = (e.cfg >> 16) & 255u;
    const ResizeGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 28};
    const CubicTile t = Filter::tile(g, lg, c, tile);
    __syncthreads();                                              // (the tile before this one has read its tables)
    for (uint32_t i = threadIdx.x; i < t.nx + t.ny; i += kResizeThreads) Filter::norm(t, g, i, qx, qy);
    __syncthreads();
    const uint32_t p = threadIdx.x >> lg, l = threadIdx.x & ((1u << lg) - 1u);
    const bool valid = p < t.px;                                  // (a pixel's lanes are valid or not together)
    const u64 o = t.o0 + p;
    const uint32_t Y = valid ? (uint32_t)resize_div(o, e.ow) : 0u, X = valid ? (uint32_t)(o - (u64)Y * e.ow) : 0u;
    ResizeSums s;
    if (valid) Filter::template lane<WEIGHTED>(mem, g, qx + cubic_tile_slot(t, o, X) * t.sx, qy + (Y - t.Y0) * t.sy, t.sy, X, Y, l, c, s);
    else resize_zero(s);
    for (uint32_t step = 1u; step < (1u << lg); step <<= 1) {    // (lg is the item's: the whole workgroup takes the same steps)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) s.S[k] = xor_add(s.S[k], step);
        if (WEIGHTED) {
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) s.W[k] = xor_add(s.W[k], step);
        }
    }
    if (valid && l == 0u) sink(mem, g, q, och, X, Y, cubic_pixel(s, WEIGHTED));
}

// The tiles of a launch of such a kernel, each with its entry's alpha mode; qx, qy: the kernel's LDS tables.
template <class Filter, class Sink>
__device__ __forceinline__ void table_tiles(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                            uint16_t* qx, uint16_t* qy, const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const ResizeEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        if ((e.cfg >> 24) & 1u) table_tile_run<Filter, true>(mem, q, e, tile, qx, qy, sink);
        else table_tile_run<Filter, false>(mem, q, e, tile, qx, qy, sink);
    });
}

}  // namespace qoimi

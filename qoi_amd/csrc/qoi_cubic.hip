// qoi_cubic.hip — qoimi_decode_tensors with QOIMI_FILTER_BICUBIC: the antialiased bicubic filter (Keys, a = -1/2) over rectangles of staged
// images, written as tensors by the kernel tensor_cubic.  gfx950, wave64.  The host side: qoi_host_tensor.hip (qoi_kernels.h declares the
// launcher); the arithmetic and its normative statement: qoi_cubic_core.h.
//
//   tensor_cubic  The table, the tile walk (qoi_dev.h: walk_tiles), the tile of 256 work items, the 1 to 16 lanes per output pixel with at
//                 most 4 columns each, the butterfly over a pixel's lanes and the store (qoi_tensor_core.h: TensorSink - for u8 HWC the byte
//                 store of the other filters) are those of tensor_tent.  What differs: the weights are signed and normalised per output
//                 column and row - a sum, up to 64 quotients and a deficit tap each - so a tile works in two phases with a barrier between
//                 them.  Phase 1: one work item per output column and row the tile holds (at most 256 + 3 of them) normalises its weights
//                 into LDS, 16 bits each: 2 KB for the columns, 32 KB for the rows (a tile of 256 single-lane pixels of a one-column output
//                 holds 256 rows of up to 64 taps) - four workgroups per CU by LDS.  The quotient is a double division mended by one integer
//                 step (cubic_quot), not a 64-bit integer division.  Phase 2: every lane reads its 4 column weights and walks its rows,
//                 reading one row weight per row (the lanes of a pixel and the pixels of a row read the same address: a broadcast) and
//                 loading only pixels whose weight is not 0; sums are 64-bit, no per-lane array is indexed by a variable (no scratch).
#include "qoi_gather_tiles.h"
#include "qoi_cubic_core.h"
#include "qoi_tensor_core.h"

namespace qoimi {

// One tile of an item: work items [tile * kResizeThreads, + kResizeThreads) as far as the item has them.
template <bool WEIGHTED, class Sink>
__device__ __forceinline__ void cubic_tile_run(const GatherMem& mem, u64 q, const ResizeEntry& e, uint32_t tile, uint16_t* qx, uint16_t* qy, const Sink& sink) {
    const uint32_t lg = e.cfg & 255u, c = (e.cfg >> 8) & 255u, och = (e.cfg >> 16) & 255u;
    const ResizeGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 28};
    const CubicTile t = cubic_tile(g, lg, c, tile);
    __syncthreads();                                              // (the tile before this one has read its tables)
    for (uint32_t i = threadIdx.x; i < t.nx + t.ny; i += kResizeThreads) cubic_tile_norm(t, g, i, qx, qy);
    __syncthreads();
    const uint32_t p = threadIdx.x >> lg, l = threadIdx.x & ((1u << lg) - 1u);
    const bool valid = p < t.px;                                  // (a pixel's lanes are valid or not together)
    const u64 o = t.o0 + p;
    const uint32_t Y = valid ? (uint32_t)resize_div(o, e.ow) : 0u, X = valid ? (uint32_t)(o - (u64)Y * e.ow) : 0u;
    ResizeSums s;
    if (valid) cubic_lane<WEIGHTED>(mem, g, qx + cubic_tile_slot(t, o, X) * t.sx, qy + (Y - t.Y0) * t.sy, t.sy, X, Y, l, c, s);
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

__global__ __launch_bounds__(kResizeThreads) void tensor_cubic(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                uint8_t* out, TensorFormat fmt) {
    __shared__ uint16_t qx[kCubicColSlots];
    __shared__ uint16_t qy[kCubicRowSlots];
    const TensorSink sink{fmt};
    walk_tiles(tab, m, tiles, [&](const ResizeEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        if ((e.cfg >> 24) & 1u) cubic_tile_run<true>(mem, q, e, tile, qx, qy, sink);
        else cubic_tile_run<false>(mem, q, e, tile, qx, qy, sink);
    });
}

void launch_tensor_cubic(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_cubic, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

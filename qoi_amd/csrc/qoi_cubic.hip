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
#include "qoi_table_tiles.h"
#include "qoi_tensor_core.h"

namespace qoimi {

// The two phases of a tile are table_tile_run's (qoi_table_tiles.h: tensor_lanczos runs them too); this filter's part of them:
struct CubicFilter {
    static __device__ __forceinline__ CubicTile tile(const ResizeGeom& g, uint32_t lg, uint32_t c, uint32_t tile) { return cubic_tile(g, lg, c, tile); }
    static __device__ __forceinline__ void norm(const CubicTile& t, const ResizeGeom& g, uint32_t i, uint16_t* qx, uint16_t* qy) { cubic_tile_norm(t, g, i, qx, qy); }
    template <bool WEIGHTED>
    static __device__ __forceinline__ void lane(const GatherMem& mem, const ResizeGeom& g, const uint16_t* qx, const uint16_t* qy, uint32_t sy, uint32_t X, uint32_t Y,
                                                uint32_t l, uint32_t c, ResizeSums& s) {
        cubic_lane<WEIGHTED>(mem, g, qx, qy, sy, X, Y, l, c, s);
    }
};

__global__ __launch_bounds__(kResizeThreads) void tensor_cubic(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                uint8_t* out, TensorFormat fmt) {
    __shared__ uint16_t qx[kCubicColSlots];
    __shared__ uint16_t qy[kCubicRowSlots];
    table_tiles<CubicFilter>(stage, tab, m, tiles, out, qx, qy, TensorSink{fmt});
}

void launch_tensor_cubic(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_cubic, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

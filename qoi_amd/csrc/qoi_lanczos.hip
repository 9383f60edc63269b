// qoi_lanczos.hip — qoimi_decode_tensors with QOIMI_FILTER_LANCZOS: the antialiased Lanczos filter with three lobes over rectangles of staged
// images, written as tensors by the kernel tensor_lanczos.  gfx950, wave64.  The host side: qoi_host_tensor.hip (qoi_kernels.h declares the
// launcher); the arithmetic and its normative statement: qoi_lanczos_core.h.
//
//   tensor_lanczos  tensor_cubic with another kernel function: the table, the tile walk, the tile of 256 work items in two phases with a
//                   barrier between them (qoi_table_tiles.h), the butterfly over a pixel's 1 to 16 lanes and the store (TensorSink) are the
//                   same.  What differs: a weight is not a polynomial but the kernel table of 3073 dwords (12 KB, generated:
//                   qoi_lanczos_table.h) interpolated linearly; it sits in device memory and only phase 1 reads it - one work item per output
//                   column and row of the tile, two entries per tap, twice - so it stays in the caches and costs no LDS.  Up to 96 taps per
//                   axis: a lane holds at most 6 column weights in registers, and the LDS tables are 3 KB for the columns and 48 KB for the
//                   rows (a tile of 256 single-lane pixels of a one-column output holds 256 rows of up to 96 taps) - 51 KB, three workgroups
//                   per CU by LDS.  qy * qx is formed in 64 bits (qoi_lanczos_core.h: why).
#define QOIMI_LANCZOS_TABLE_SPACE static __device__
#include "qoi_lanczos_table.h"
#include "qoi_table_tiles.h"
#include "qoi_lanczos_core.h"
#include "qoi_tensor_core.h"

namespace qoimi {

static_assert(sizeof(kLanczosTable) == kLanczosEntries * sizeof(int32_t), "the table the core indexes");

struct LanczosFilter {
    static __device__ __forceinline__ CubicTile tile(const ResizeGeom& g, uint32_t lg, uint32_t c, uint32_t tile) { return lanczos_tile(g, lg, c, tile); }
    static __device__ __forceinline__ void norm(const CubicTile& t, const ResizeGeom& g, uint32_t i, uint16_t* qx, uint16_t* qy) {
        lanczos_tile_norm(kLanczosTable, t, g, i, qx, qy);
    }
    template <bool WEIGHTED>
    static __device__ __forceinline__ void lane(const GatherMem& mem, const ResizeGeom& g, const uint16_t* qx, const uint16_t* qy, uint32_t sy, uint32_t X, uint32_t Y,
                                                uint32_t l, uint32_t c, ResizeSums& s) {
        lanczos_lane<WEIGHTED>(mem, g, qx, qy, sy, X, Y, l, c, s);
    }
};

__global__ __launch_bounds__(kResizeThreads) void tensor_lanczos(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                  uint8_t* out, TensorFormat fmt) {
    __shared__ uint16_t qx[kLanczosColSlots];
    __shared__ uint16_t qy[kLanczosRowSlots];
    table_tiles<LanczosFilter>(stage, tab, m, tiles, out, qx, qy, TensorSink{fmt});
}

void launch_tensor_lanczos(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_lanczos, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

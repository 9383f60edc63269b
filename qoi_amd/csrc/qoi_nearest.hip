// qoi_nearest.hip — qoimi_decode_tensors with QOIMI_FILTER_NEAREST: rectangles of staged images sampled to a fixed size by selection - one
// source pixel per output pixel, nothing averaged - and written as tensors by the kernel tensor_nearest: label maps on their way to a loss
// function (with QOIMI_TENSOR_I64 and QOIMI_TENSOR_HW: N x H x W class indices).  gfx950, wave64.  The host side: qoi_host_tensor.hip
// (qoi_kernels.h declares the launcher); the arithmetic and its normative statement: qoi_nearest_core.h.
//
//   tensor_nearest  The table of ResizeEntry and the tile walk of the other filters (qoi_dev.h: walk_tiles; one launch per sub-batch), a tile
//                   of 256 work items - but a walk of its own, not filter_tiles: there are no sums, no lane split and no butterfly, so the
//                   body is four lines (nearest_work) and the filter tiles keep their code.  One work item per output pixel: two 32-bit
//                   divisions for (X, Y) -> (k, r) (every size is at most 2^14: no 64-bit division), one aligned dword load from the staged
//                   4-channel image, the sink (TensorSink: the pixel goes from the register it was loaded into to its elements).  Consecutive
//                   lanes take consecutive X of a row: the stores of a plane are consecutive elements; the loads of a wavefront lie in one
//                   or two source rows, cw / ow pixels apart - when reducing much, one cache line per lane, which is what selection costs.
//                   No LDS, no barrier, no scratch.
#include "qoi_gather_tiles.h"
#include "qoi_nearest_core.h"
#include "qoi_tensor_core.h"

namespace qoimi {

__global__ __launch_bounds__(kResizeThreads) void tensor_nearest(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                  uint8_t* out, TensorFormat fmt) {
    const TensorSink sink{fmt};
    walk_tiles(tab, m, tiles, [&](const ResizeEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const ResizeGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 28};
        nearest_work(mem, g, q, (e.cfg >> 16) & 255u, (u64)tile * kResizeThreads + threadIdx.x, sink);
    });
}

void launch_tensor_nearest(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_nearest, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

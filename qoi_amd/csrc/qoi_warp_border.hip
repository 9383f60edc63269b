// qoi_warp_border.hip — qoimi_decode_warped and qoimi_decode_warped_tensors for calls with a QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 or
// QOIMI_WARP_WRAP item: the tiles of warp_gather with every tap index folded into the rectangle, as bytes (warp_border_bytes) or as a tensor
// (warp_border_tensor).  gfx950, wave64.  The host side: gather_warped of qoi_staged.h picks these launchers for a call that carries one of
// the three flags and the kernels of qoi_warp.hip, qoi_tensor.hip and qoi_warp_cubic.hip, exactly as before, for one that does not
// (qoi_kernels.h declares the launchers).
//
// The result (normative; qoi_amd/warp.py: warp and fold state it in Python, qoi_warp_border_core.h holds the arithmetic).
//
//   warp_border_bytes, warp_border_tensor
//                 The table (WarpEntry), the walk (qoi_dev.h: walk_tiles) and the tile - 16 x 16 output pixels of one item, thread t its pixel
//                 (t & 15, t >> 4) - are warp_gather's.  A tile of an item with a border flag takes warp_border_pixel; a tile of any other
//                 item goes through warp_cubic_work as it is (warp_cubic_pixel / warp_pixel / warp_nearest), so a mixed table is one launch
//                 and an item without such a flag keeps its bytes.  Border and sampling are the entry's: uniform over the workgroup.
//                 A lane computes both positions in 64 bits and the weights of its sampling as ever, folds the FIRST 64-bit tap index of
//                 each axis into the period of the border - a conditional add or subtract where the tap lies within one period of the
//                 rectangle, else a quotient estimate in double precision, one 64-bit multiply-subtract and that same correction: exact,
//                 no integer division - and steps the other taps from it with a compare and a select.  Every tap is inside the rectangle:
//                 no fill, no load for a tap without a weight.  The loads, the blend, the one rounding, the clamp and the sink's store are
//                 warp_blend / warp_cubic_blend and WarpByteSink / TensorSink.  No LDS, no barrier, no atomics, no scratch; not one byte
//                 outside an item's output is written.
#include "qoi_gather_tiles.h"
#include "qoi_tensor_core.h"
#include "qoi_warp_border_core.h"

namespace qoimi {

// The tiles of a launch, each with its entry's alpha mode, sampling and border (warp_walk of qoi_gather_tiles.h with the work item of this file).
template <class Sink>
__device__ __forceinline__ void warp_border_walk(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                                  const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const WarpEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const WarpGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 16, e.a, e.b, e.d, e.e, e.fill, e.c, e.f};
        const uint32_t och = e.cfg & 255u;
        if ((e.cfg >> 8) & 1u) warp_border_work<true>(mem, g, q, och, tile, threadIdx.x, sink);
        else warp_border_work<false>(mem, g, q, och, tile, threadIdx.x, sink);
    });
}

__global__ __launch_bounds__(kWarpThreads) void warp_border_bytes(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                             uint8_t* out) {
    warp_border_walk(stage, tab, m, tiles, out, WarpByteSink());
}

__global__ __launch_bounds__(kWarpThreads) void warp_border_tensor(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m,
                                                                    uint32_t tiles, uint8_t* out, TensorFormat fmt) {
    warp_border_walk(stage, tab, m, tiles, out, TensorSink{fmt});
}

void launch_warp_border(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_border_bytes, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_tensor_warp_border(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_border_tensor, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

// qoi_warp_cubic.hip — qoimi_decode_warped and qoimi_decode_warped_tensors for calls with a QOIMI_WARP_BICUBIC item: the tiles of warp_gather
// with 4 x 4 samples under Keys' cubic (a = -1/2) in exact integers, as bytes (warp_bicubic_bytes) or as a tensor (warp_bicubic_tensor).  gfx950,
// wave64.  The host side: gather_warped of qoi_staged.h picks these launchers for a call that carries the flag and the kernels of qoi_warp.hip
// and qoi_tensor.hip, exactly as before, for one that does not (qoi_kernels.h declares the launchers).
//
// The result (normative; qoi_amd/warp.py: warp states it in Python, qoi_warp_cubic_core.h holds the arithmetic).
//
//   warp_bicubic_bytes, warp_bicubic_tensor
//                 The table (WarpEntry), the walk (qoi_dev.h: walk_tiles) and the tile - 16 x 16 output pixels of one item, thread t its pixel
//                 (t & 15, t >> 4) - are warp_gather's.  A tile of an item with the flag takes the 4 x 4 path; a tile of any other item calls
//                 warp_pixel / warp_nearest as they are, so a mixed table is one launch and a bilinear or nearest item keeps its bytes.  The
//                 branch is the entry's: uniform over the workgroup.
//                 A lane computes both positions in 64 bits, the four weights of each axis from the cubic in 64-bit integers (they sum to
//                 2^15 exactly), tests the border on the 64-bit indices, and then goes row by row: up to four staged pixels as aligned dwords
//                 - plain loads; none for a sample that takes the fill or has no weight -, their horizontal blend per channel in 32 bits
//                 (64 with alpha), one 64-bit multiply-add by the row's weight.  It holds one row of samples, never sixteen pixels.  One
//                 rounding, a clamp (the negative lobes overshoot), and the sink's store: WarpByteSink or TensorSink.  No LDS, no barrier, no
//                 atomics, no scratch; not one byte outside an item's output is written.
//                 Not built: staging the tile's source footprint in LDS (DESIGN.md 4i-2 says what measurement would justify it).
#include "qoi_gather_tiles.h"
#include "qoi_tensor_core.h"
#include "qoi_warp_cubic_core.h"

namespace qoimi {

// The tiles of a launch, each with its entry's alpha mode and sampling (warp_walk of qoi_gather_tiles.h with the work item of this file).
template <class Sink>
__device__ __forceinline__ void warp_cubic_walk(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                                 const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const WarpEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const WarpGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 16, e.a, e.b, e.d, e.e, e.fill, e.c, e.f};
        const uint32_t och = e.cfg & 255u;
        if ((e.cfg >> 8) & 1u) warp_cubic_work<true>(mem, g, q, och, tile, threadIdx.x, sink);
        else warp_cubic_work<false>(mem, g, q, och, tile, threadIdx.x, sink);
    });
}

__global__ __launch_bounds__(kWarpThreads) void warp_bicubic_bytes(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                              uint8_t* out) {
    warp_cubic_walk(stage, tab, m, tiles, out, WarpByteSink());
}

__global__ __launch_bounds__(kWarpThreads) void warp_bicubic_tensor(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m,
                                                                     uint32_t tiles, uint8_t* out, TensorFormat fmt) {
    warp_cubic_walk(stage, tab, m, tiles, out, TensorSink{fmt});
}

void launch_warp_cubic(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_bicubic_bytes, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_tensor_warp_cubic(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_bicubic_tensor, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

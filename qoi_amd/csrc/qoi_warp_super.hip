// qoi_warp_super.hip — qoimi_decode_warped and qoimi_decode_warped_tensors for calls with a QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4 item: the
// tiles of warp_gather with s x s bilinear sub-samples per output pixel and one rounding, as bytes (warp_super_bytes) or as a tensor
// (warp_super_tensor).  gfx950, wave64.  The host side: gather_warped of qoi_staged.h picks these launchers for a call that carries one of
// the two flags and the kernels of qoi_warp.hip, qoi_tensor.hip, qoi_warp_cubic.hip and qoi_warp_border.hip, exactly as before, for one that
// does not (qoi_kernels.h declares the launchers).
//
// The result (normative; qoi_amd/warp.py: warp states it in Python, qoi_warp_super_core.h holds the arithmetic).
//
//   warp_super_bytes, warp_super_tensor
//                 The table (WarpEntry), the walk (qoi_dev.h: walk_tiles) and the tile - 16 x 16 output pixels of one item, thread t its pixel
//                 (t & 15, t >> 4) - are warp_gather's.  A tile of an item with a SUPER flag takes warp_super_pixel; a tile of any other item
//                 goes through warp_border_work as it is (warp_border_pixel / warp_cubic_pixel / warp_pixel / warp_nearest), so a mixed
//                 table is one launch and an item without such a flag keeps its bytes.  s and the border are the entry's: uniform over the
//                 workgroup, so the loop over the s^2 sub-samples has one trip count for all lanes of a tile.
//                 A lane computes both positions of a sub-sample in 64 bits, its 2 x 2 taps and weights with the item's border (warp_axis or
//                 warp_border_axis), loads up to four pixels directly - 4 s^2 per output pixel; the footprint of a tile at 4 : 1 is about
//                 64 x 64 source pixels, which neighbouring lanes share through the cache -, adds the products to seven 64-bit sums in
//                 registers, and after the last sub-sample rounds once (a shift; the alpha-weighted colours through resize_div) and
//                 stores once through WarpByteSink / TensorSink.  No LDS, no barrier, no atomics, no scratch; not one byte outside an
//                 item's output is written.
#include "qoi_gather_tiles.h"
#include "qoi_tensor_core.h"
#include "qoi_warp_super_core.h"

namespace qoimi {

// The tiles of a launch, each with its entry's alpha mode, sampling, border and sub-samples (warp_walk of qoi_gather_tiles.h with the work item of this file).
template <class Sink>
__device__ __forceinline__ void warp_super_walk(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                                 const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const WarpEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const WarpGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 16, e.a, e.b, e.d, e.e, e.fill, e.c, e.f};
        const uint32_t och = e.cfg & 255u;
        if ((e.cfg >> 8) & 1u) warp_super_work<true>(mem, g, q, och, tile, threadIdx.x, sink);
        else warp_super_work<false>(mem, g, q, och, tile, threadIdx.x, sink);
    });
}

__global__ __launch_bounds__(kWarpThreads) void warp_super_bytes(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                            uint8_t* out) {
    warp_super_walk(stage, tab, m, tiles, out, WarpByteSink());
}

__global__ __launch_bounds__(kWarpThreads) void warp_super_tensor(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m,
                                                                   uint32_t tiles, uint8_t* out, TensorFormat fmt) {
    warp_super_walk(stage, tab, m, tiles, out, TensorSink{fmt});
}

void launch_warp_super(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_super_bytes, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_tensor_warp_super(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_super_tensor, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

// qoi_warp_vote.hip — qoimi_decode_warped and qoimi_decode_warped_tensors for calls with a QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4 item: the
// tiles of warp_gather with the majority vote of s x s nearest sub-samples per output pixel, as bytes (warp_vote_bytes) or as a tensor
// (warp_vote_tensor).  gfx950, wave64.  The host side: gather_warped of qoi_staged.h picks these launchers for a call that carries one of
// the two flags and the kernels of qoi_warp.hip, qoi_tensor.hip, qoi_warp_cubic.hip, qoi_warp_border.hip and qoi_warp_super.hip, exactly as
// before, for one that does not (qoi_kernels.h declares the launchers).
//
// The result (normative; qoi_amd/warp.py: warp states it in Python, qoi_warp_vote_core.h holds the arithmetic).
//
//   warp_vote_bytes, warp_vote_tensor
//                 The table (WarpEntry), the walk (qoi_dev.h: walk_tiles) and the tile - 16 x 16 output pixels of one item, thread t its pixel
//                 (t & 15, t >> 4) - are warp_gather's.  A tile of an item with a VOTE flag takes warp_vote_pixel; a tile of any other item
//                 goes through warp_super_work as it is (warp_super_pixel / warp_border_pixel / warp_cubic_pixel / warp_pixel /
//                 warp_nearest), so a mixed table is one launch and an item without such a flag keeps its bytes.  s and the border are the
//                 entry's: uniform over the workgroup, so every lane of a tile takes the same instantiation of the pixel function.
//                 A lane computes both positions of a sub-sample in 64 bits, brings the index of its one sample into the rectangle with the
//                 item's border or takes the fill, and loads it directly - s^2 + 1 loads per output pixel at most, the last for the centre
//                 value that decides a tie; the footprint of a tile at 4 : 1 is about 64 x 64 source pixels, which neighbouring lanes share
//                 through the cache.  It holds the up to 16 sub-sample dwords and the centre value in registers (the pixel function is
//                 instantiated per L and fully unrolled: no value is indexed dynamically), counts by comparison, keeps the largest
//                 mode_word, and stores once through WarpByteSink / TensorSink.  No LDS, no barrier, no atomics, no scratch; not one byte
//                 outside an item's output is written.
#include "qoi_gather_tiles.h"
#include "qoi_tensor_core.h"
#include "qoi_warp_vote_core.h"

namespace qoimi {

// The tiles of a launch, each with its entry's alpha mode, sampling, border and sub-samples (warp_walk of qoi_gather_tiles.h with the work item of this file).
template <class Sink>
__device__ __forceinline__ void warp_vote_walk(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                                const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const WarpEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const WarpGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 16, e.a, e.b, e.d, e.e, e.fill, e.c, e.f};
        const uint32_t och = e.cfg & 255u;
        if ((e.cfg >> 8) & 1u) warp_vote_work<true>(mem, g, q, och, tile, threadIdx.x, sink);
        else warp_vote_work<false>(mem, g, q, och, tile, threadIdx.x, sink);
    });
}

__global__ __launch_bounds__(kWarpThreads) void warp_vote_bytes(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                           uint8_t* out) {
    warp_vote_walk(stage, tab, m, tiles, out, WarpByteSink());
}

__global__ __launch_bounds__(kWarpThreads) void warp_vote_tensor(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m,
                                                                  uint32_t tiles, uint8_t* out, TensorFormat fmt) {
    warp_vote_walk(stage, tab, m, tiles, out, TensorSink{fmt});
}

void launch_warp_vote(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_vote_bytes, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_tensor_warp_vote(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_vote_tensor, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

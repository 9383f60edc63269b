// qoi_warp_proj.hip — qoimi_decode_warped and qoimi_decode_warped_tensors for calls with a QOIMI_WARP_PROJECTIVE item: the tiles of
// warp_gather with the position of an output pixel divided by the item's linear denominator, as bytes (warp_proj_bytes) or as a tensor
// (warp_proj_tensor).  gfx950, wave64.  The host side: gather_warped of qoi_staged.h picks these launchers for a call that carries the flag
// and the kernels of qoi_warp.hip, qoi_tensor.hip, qoi_warp_cubic.hip, qoi_warp_border.hip, qoi_warp_super.hip and qoi_warp_vote.hip,
// exactly as before, for one that does not (qoi_kernels.h declares the launchers).
//
// The result (normative; qoi_amd/warp.py: positions and warp state it in Python, qoi_warp_proj_core.h holds the arithmetic).
//
//   warp_proj_bytes, warp_proj_tensor
//                 The table (WarpEntry), the walk (qoi_dev.h: walk_tiles) and the tile - 16 x 16 output pixels of one item, thread t its pixel
//                 (t & 15, t >> 4) - are warp_gather's.  A tile of an item with the flag (bit 9 of WarpEntry::cfg: cfg's upper half holds the
//                 16 older flag bits) takes warp_proj_work's own path; a tile of any other item goes through warp_vote_work as it is
//                 (warp_vote_pixel / warp_super_pixel / warp_border_pixel / warp_cubic_pixel / warp_pixel / warp_nearest), so a mixed table
//                 is one launch and an item without the flag keeps its bytes.  F, g and h are the entry's: uniform over the workgroup.
//                 A lane forms its denominator W = 2^F + g * Uc + h * Vc and both affine positions in 64 bits, takes ONE reciprocal of W in
//                 double precision and brings floor(N * 2^F / W) down in two or three stages per position - each a conversion, a v_mul_f64, a
//                 v_floor_f64, a conversion back, a 64-bit multiply-subtract and a +-1 correction; the integer subtraction makes every
//                 stage exact, the double only picks the multiple.  No 64-bit integer division and no 128-bit arithmetic is compiled.  From
//                 the two positions on the lane runs the older code: one, 2 x 2 or 4 x 4 taps with the item's border or the fill, the
//                 blend, one store through WarpByteSink / TensorSink.  No LDS, no barrier, no atomics, no scratch; not one byte outside an
//                 item's output is written.
#include "qoi_gather_tiles.h"
#include "qoi_tensor_core.h"
#include "qoi_warp_proj_core.h"

namespace qoimi {

// The tiles of a launch, each with its entry's alpha mode, sampling, border, sub-samples and denominator (warp_walk of qoi_gather_tiles.h with the work item of this file).
template <class Sink>
__device__ __forceinline__ void warp_proj_walk(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                                const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const WarpEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const uint32_t flags = (e.cfg >> 16) | ((e.cfg & kWarpEntryProjective) != 0u ? kWarpProjective : 0u);
        const WarpGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, flags, e.a, e.b, e.d, e.e, e.fill, e.c, e.f};
        const WarpProj pj = {e.g, e.h};
        const uint32_t och = e.cfg & 255u;
        if ((e.cfg >> 8) & 1u) warp_proj_work<true>(mem, g, pj, q, och, tile, threadIdx.x, sink);
        else warp_proj_work<false>(mem, g, pj, q, och, tile, threadIdx.x, sink);
    });
}

__global__ __launch_bounds__(kWarpThreads) void warp_proj_bytes(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                           uint8_t* out) {
    warp_proj_walk(stage, tab, m, tiles, out, WarpByteSink());
}

__global__ __launch_bounds__(kWarpThreads) void warp_proj_tensor(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m,
                                                                  uint32_t tiles, uint8_t* out, TensorFormat fmt) {
    warp_proj_walk(stage, tab, m, tiles, out, TensorSink{fmt});
}

void launch_warp_proj(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_proj_bytes, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_tensor_warp_proj(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_proj_tensor, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

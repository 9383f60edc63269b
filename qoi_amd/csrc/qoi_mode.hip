// qoi_mode.hip — qoimi_decode_tensors with QOIMI_FILTER_MODE: rectangles of staged images reduced to a fixed size by a majority vote over
// the cell of source pixels of each output pixel - whole pixels vote, nothing is averaged - and written as tensors by the kernel
// tensor_mode: label maps on their way to a loss function.  gfx950, wave64.  The host side: qoi_host_tensor.hip (qoi_kernels.h declares the
// launcher); the arithmetic and its normative statement: qoi_mode_core.h.
//
//   tensor_mode  The table of ResizeEntry and the tile walk of the other filters (qoi_dev.h: walk_tiles; one launch per sub-batch), a tile of
//                256 work items.  L = 2^lg neighbouring lanes (1..64, the entry's: qoi_mode_core.h: mode_split) share an output pixel; a
//                lane loads at most four pixels of the cell into registers (aligned dwords of the staged 4-channel image) and keeps how
//                many it holds.  Counting: the lane compares its pixels with its own, then in L - 1 steps with those of the lane s further
//                on in its group (five __shfl of width L per step: four pixels and the count), 16 compares a step - afterwards every held
//                pixel knows how many pixels of the cell equal it.  Picking: the maximum of the 64-bit word count | centre | ~key over the
//                lane's pixels, then a butterfly of lg __shfl_xor steps over the group; the group's first lane hands the pixel to the sink
//                (TensorSink).  lg is the entry's and the walk hands a tile to the whole workgroup, so every cross-lane operation is
//                reached by all 256 lanes: lanes behind the item's last pixel take part holding nothing.  All lanes of a group lie in one
//                wavefront (L divides 64).  No LDS, no barrier, no scratch; the bounds: qoi_mode_core.h.
#include "qoi_gather_tiles.h"
#include "qoi_mode_core.h"
#include "qoi_tensor_core.h"

namespace qoimi {

__device__ __forceinline__ u64 xor_max(u64 v, uint32_t step) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)step);
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}

__global__ __launch_bounds__(kResizeThreads) void tensor_mode(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               uint8_t* out, TensorFormat fmt) {
    const TensorSink sink{fmt};
    walk_tiles(tab, m, tiles, [&](const ResizeEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const ResizeGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 28};
        const uint32_t lg = e.cfg & 255u, L = 1u << lg, och = (e.cfg >> 16) & 255u;
        const u64 item = (u64)tile * kResizeThreads + threadIdx.x, o = item >> lg;
        const uint32_t l = (uint32_t)item & (L - 1u);
        const bool valid = o < (u64)e.ow * e.oh;                      // (a pixel's lanes are valid or not together)
        const uint32_t Y = valid ? (uint32_t)o / e.ow : 0u, X = valid ? (uint32_t)o - Y * e.ow : 0u;
        ModeHeld h;
        if (valid) mode_hold(mem, g, X, Y, l, lg, h);
        else mode_none(h);
        uint32_t count[kModeHold] = {0u, 0u, 0u, 0u};
        mode_meet(h, h.v, h.n, count);
        for (uint32_t s = 1u; s < L; ++s) {                           // (lg is the item's: the whole workgroup takes the same steps)
            uint32_t ov[kModeHold];
#pragma unroll
            for (uint32_t j = 0; j < kModeHold; ++j) ov[j] = (uint32_t)__shfl((int)h.v[j], (int)(l + s), (int)L);
            const uint32_t on = (uint32_t)__shfl((int)h.n, (int)(l + s), (int)L);
            mode_meet(h, ov, on, count);
        }
        u64 best = mode_best(h, count);
        for (uint32_t step = 1u; step < L; step <<= 1) best = xor_max(best, step);
        if (valid && l == 0u) sink(mem, g, q, och, X, Y, mode_pick(best));
    });
}

void launch_tensor_mode(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_mode, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

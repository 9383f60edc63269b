// qoi_gather_tiles.h — the tiles of the resampling kernels, shared by the kernels that write bytes (qoi_resize.hip: resize_filter,
// bilinear_filter; qoi_warp.hip: warp_gather) and those that write tensors (qoi_tensor.hip): everything up to the rounded pixel in a register
// is one body, the finish step is a SINK - sink(mem, geometry, q, och, X, Y, pixel) - that the kernel chooses (qoi_resize_core.h:
// ResizeByteSink, qoi_warp_core.h: WarpByteSink, qoi_tensor_core.h: TensorSink).  Device only; qoi_resize.hip and qoi_warp.hip describe the
// tiles.
#pragma once
#include "qoi_dev.h"
#include "qoi_bilinear_core.h"
#include "qoi_warp_core.h"

namespace qoimi {

// Staged pixels as aligned dwords - plain loads: items may share source pixels -, elements of the output as whole aligned stores.
struct GatherMem {
    const uint32_t* src;
    __device__ __forceinline__ uint32_t load(u64 i) const { return src[i]; }
    __device__ __forceinline__ void store1(u64 a, uint32_t v) const { *reinterpret_cast<uint8_t*>(a) = (uint8_t)v; }
    __device__ __forceinline__ void store2(u64 a, uint32_t v) const { *reinterpret_cast<uint16_t*>(a) = (uint16_t)v; }
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
};

__device__ __forceinline__ u64 xor_add(u64 v, uint32_t step) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)step);
    return v + (((u64)hi << 32) | lo);
}

// A filter: the sums of a lane, its share of a pixel (lane), the sums of a lane without one (zero), one butterfly step over the sums that
// cross lanes (shared, add_own), and sums to rounded pixel (pixel).
struct AreaFilter {
    using Sums = ResizeSums;
    template <bool WEIGHTED>
    static __device__ __forceinline__ void lane(const GatherMem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t c, Sums& s) {
        resize_lane<WEIGHTED>(mem, g, X, Y, l, c, s);
    }
    static __device__ __forceinline__ void zero(Sums& s) { resize_zero(s); }
    static __device__ __forceinline__ ResizeSums& shared(Sums& s) { return s; }
    static __device__ __forceinline__ void add_own(Sums&, uint32_t) {}
    static __device__ __forceinline__ uint32_t pixel(const ResizeGeom& g, bool weighted, const Sums& s) { return resize_pixel(s, (u64)g.cw * g.rh, weighted); }
};

struct TentFilter {
    using Sums = BilinearSums;
    template <bool WEIGHTED>
    static __device__ __forceinline__ void lane(const GatherMem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t c, Sums& s) {
        bilinear_lane<WEIGHTED>(mem, g, X, Y, l, c, s);
    }
    static __device__ __forceinline__ void zero(Sums& s) { resize_zero(s.v); s.wx = 0u; s.wy = 0u; }
    static __device__ __forceinline__ ResizeSums& shared(Sums& s) { return s.v; }
    static __device__ __forceinline__ void add_own(Sums& s, uint32_t step) { s.wx = xor_add(s.wx, step); }   // (wy stays the lane's own: lane 0 holds Wy)
    static __device__ __forceinline__ uint32_t pixel(const ResizeGeom&, bool weighted, const Sums& s) { return resize_pixel(s.v, bilinear_divisor(s), weighted); }
};

// One tile of an item: work items [base, base + kResizeThreads) as far as the item has them.
template <class Filter, bool WEIGHTED, class Sink>
__device__ __forceinline__ void filter_tile(const GatherMem& mem, u64 q, const ResizeEntry& e, u64 base, const Sink& sink) {
    const uint32_t lg = e.cfg & 255u, c = (e.cfg >> 8) & 255u, och = (e.cfg >> 16) & 255u;
    const ResizeGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 28};
    const u64 item = base + threadIdx.x, o = item >> lg;
    const uint32_t l = (uint32_t)item & ((1u << lg) - 1u);
    const bool valid = o < (u64)e.ow * e.oh;                      // (a pixel's lanes are valid or not together)
    const uint32_t Y = valid ? (uint32_t)resize_div(o, e.ow) : 0u, X = valid ? (uint32_t)(o - (u64)Y * e.ow) : 0u;
    typename Filter::Sums s;
    if (valid) Filter::template lane<WEIGHTED>(mem, g, X, Y, l, c, s);
    else Filter::zero(s);
    ResizeSums& v = Filter::shared(s);
    for (uint32_t step = 1u; step < (1u << lg); step <<= 1) {    // (lg is the item's: the whole workgroup takes the same steps)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) v.S[k] = xor_add(v.S[k], step);
        if (WEIGHTED) {
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) v.W[k] = xor_add(v.W[k], step);
        }
        Filter::add_own(s, step);
    }
    if (valid && l == 0u) sink(mem, g, q, och, X, Y, Filter::pixel(g, WEIGHTED, s));
}

// The tiles of a launch of a filter kernel, each with its entry's alpha mode.
template <class Filter, class Sink>
__device__ __forceinline__ void filter_tiles(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                             const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const ResizeEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const u64 base = (u64)tile * kResizeThreads;
        if ((e.cfg >> 24) & 1u) filter_tile<Filter, true>(mem, q, e, base, sink);
        else filter_tile<Filter, false>(mem, q, e, base, sink);
    });
}

// The tiles of a launch of a warp kernel, each with its entry's alpha mode.
template <class Sink>
__device__ __forceinline__ void warp_walk(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out,
                                           const Sink& sink) {
    walk_tiles(tab, m, tiles, [&](const WarpEntry& e, uint32_t tile) {
        const GatherMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const WarpGeom g = {e.w, e.x, e.y, e.cw, e.rh, e.ow, e.oh, e.cfg >> 16, e.a, e.b, e.d, e.e, e.fill, e.c, e.f};
        const uint32_t och = e.cfg & 255u;
        if ((e.cfg >> 8) & 1u) warp_work<true>(mem, g, q, och, tile, threadIdx.x, sink);
        else warp_work<false>(mem, g, q, och, tile, threadIdx.x, sink);
    });
}

}  // namespace qoimi

// qoi_resize.hip — qoimi_decode_resized and qoimi_decode_bilinear: rectangles of a sub-batch of decoded images resampled to caller-chosen sizes
// by an exact integer area filter (resize_filter) or by an antialiased bilinear (triangle) filter in exact integers (bilinear_filter).  gfx950,
// wave64.  The host side: qoi_host_staged.hip (qoi_kernels.h holds the table and declares the launchers).
//
// The result (normative; qoi_amd/resize.py: resize and qoi_amd/bilinear.py: bilinear state it in Python, qoi_resize_core.h and
// qoi_bilinear_core.h hold the arithmetic): image i stands in the staging arena as w x rows pixels of 4 bytes (the decoder's output at 4 channels
// down to the last row an item needs: a 256-aligned slot, every pixel an aligned dword); an item is a rectangle cw x rh of it, resampled to
// ow x oh pixels - with the weights wy * wx of the overlaps, or with the weights ty * tx of the tents around the output pixel's centre
// renormalised by their sum -, rounded once, plain or with the colours weighted by alpha, rows and / or columns reversed, written tightly packed
// with och = 3 or 4 bytes per pixel at any byte address.
//
//   filter_tile   What both kernels run.  Work is cut over the OUTPUT.  An output pixel has up to 65 x 65 staged pixels with a weight under the
//                 area filter (cw <= 64 * ow, rh <= 64 * oh), up to 64 x 64 under the tents (cw <= 32 * ow, rh <= 32 * oh; 2 x 2 when enlarging).
//                 Its columns belong to L = 1, 2, 4, 8 or 16 neighbouring lanes, chosen from the item's bound of columns per output column
//                 (resize_taps, bilinear_taps) so that a lane holds at most four of them (five for the area filter's 65); lane l takes the
//                 columns [k0 + l*c, + c) in every row with a weight.  A WORK ITEM is one lane's share; work item = (output pixel of the
//                 unflipped result, row-major) * L + l, so consecutive lanes read consecutive addresses of a staged row.  TILES of
//                 kResizeThreads work items of ONE item are laid over the table the host builds (a ResizeEntry holds its item's first tile);
//                 a workgroup takes a contiguous range of tiles (qoi_dev.h: walk_tiles), so one launch serves every item of a sub-batch.
//                 A lane computes its column weights once and a row weight per row from the closed form (no table in memory), loads its
//                 pixels as aligned dwords - plain loads: items may share source pixels - and adds weight * channel into 64-bit sums (four,
//                 seven with alpha weighting), one 32 x 32 -> 64 multiply-add each; under the tents it adds its column weights into an eighth.
//                 The L lanes of a pixel add their sums with log2(L) butterfly steps over both halves of each sum (L divides 64 and work
//                 items are numbered so that a pixel's lanes are neighbours in one wavefront); the first of them divides - by cw * rh, or by
//                 Wx * Wy: it has walked every row with a weight and holds their sum - and stores the pixel at its place, mirrored or not
//                 (qoi_resize_core.h: resize_pixel, resize_store): one dword where the output holds 4 bytes per pixel and the address is
//                 aligned, else 3 or 4 bytes - never a word it would have to read first, two outputs may share one.  No LDS, no barrier, no
//                 atomics; not one byte outside an item's output is written.
//                 The direct 2-D form of the tents takes (2s)^2 taps per pixel at a reduction s where the area filter takes s^2; a separable
//                 two-pass form is not built here.
#include "qoi_dev.h"
#include "qoi_bilinear_core.h"

namespace qoimi {

struct FilterMem {
    const uint32_t* src;
    __device__ __forceinline__ uint32_t load(u64 i) const { return src[i]; }
    __device__ __forceinline__ void store1(u64 a, uint32_t v) const { *reinterpret_cast<uint8_t*>(a) = (uint8_t)v; }
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
};

__device__ __forceinline__ u64 xor_add(u64 v, uint32_t step) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)step);
    return v + (((u64)hi << 32) | lo);
}

// A filter: the sums of a lane, its share of a pixel (lane), the sums of a lane without one (zero), one butterfly step over the sums that
// cross lanes (shared, add_own), and sums to stored pixel (finish).
struct AreaFilter {
    using Sums = ResizeSums;
    template <bool WEIGHTED>
    static __device__ __forceinline__ void lane(const FilterMem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t c, Sums& s) {
        resize_lane<WEIGHTED>(mem, g, X, Y, l, c, s);
    }
    static __device__ __forceinline__ void zero(Sums& s) { resize_zero(s); }
    static __device__ __forceinline__ ResizeSums& shared(Sums& s) { return s; }
    static __device__ __forceinline__ void add_own(Sums&, uint32_t) {}
    static __device__ __forceinline__ void finish(const FilterMem& mem, const ResizeGeom& g, u64 q, uint32_t och, bool weighted, uint32_t X, uint32_t Y, const Sums& s) {
        resize_finish(mem, g, q, och, weighted, X, Y, s);
    }
};

struct TentFilter {
    using Sums = BilinearSums;
    template <bool WEIGHTED>
    static __device__ __forceinline__ void lane(const FilterMem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t c, Sums& s) {
        bilinear_lane<WEIGHTED>(mem, g, X, Y, l, c, s);
    }
    static __device__ __forceinline__ void zero(Sums& s) { resize_zero(s.v); s.wx = 0u; s.wy = 0u; }
    static __device__ __forceinline__ ResizeSums& shared(Sums& s) { return s.v; }
    static __device__ __forceinline__ void add_own(Sums& s, uint32_t step) { s.wx = xor_add(s.wx, step); }   // (wy stays the lane's own: lane 0 holds Wy)
    static __device__ __forceinline__ void finish(const FilterMem& mem, const ResizeGeom& g, u64 q, uint32_t och, bool weighted, uint32_t X, uint32_t Y, const Sums& s) {
        bilinear_finish(mem, g, q, och, weighted, X, Y, s);
    }
};

// One tile of an item: work items [base, base + kResizeThreads) as far as the item has them.
template <class Filter, bool WEIGHTED>
__device__ __forceinline__ void filter_tile(const FilterMem& mem, u64 q, const ResizeEntry& e, u64 base) {
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
    if (valid && l == 0u) Filter::finish(mem, g, q, och, WEIGHTED, X, Y, s);
}

// The tiles of a launch, each with its entry's alpha mode.
template <class Filter>
__device__ __forceinline__ void filter_tiles(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles, uint8_t* out) {
    walk_tiles(tab, m, tiles, [&](const ResizeEntry& e, uint32_t tile) {
        const FilterMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const u64 base = (u64)tile * kResizeThreads;
        if ((e.cfg >> 24) & 1u) filter_tile<Filter, true>(mem, q, e, base);
        else filter_tile<Filter, false>(mem, q, e, base);
    });
}

__global__ __launch_bounds__(kResizeThreads) void resize_filter(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                 uint8_t* out) {
    filter_tiles<AreaFilter>(stage, tab, m, tiles, out);
}

__global__ __launch_bounds__(kResizeThreads) void bilinear_filter(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                   uint8_t* out) {
    filter_tiles<TentFilter>(stage, tab, m, tiles, out);
}

void launch_resize(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(resize_filter, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_bilinear(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(bilinear_filter, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out);
}

}  // namespace qoimi

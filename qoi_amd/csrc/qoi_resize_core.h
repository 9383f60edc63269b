// qoi_resize_core.h — the arithmetic of qoimi_decode_resized: how an output pixel's source columns are shared among lanes, one lane's weighted
// sums over its share, the sums of a pixel to its bytes, and with which stores they are written.
//
// The definition (normative; qoi_amd/resize.py states it in Python).  A rectangle cw x rh at (x, y) of an image staged as rows of w pixels of 4
// bytes is resampled to ow x oh pixels.  Output column X weighs source column k of the rectangle with the overlap of [X*cw, (X+1)*cw) and
// [k*ow, (k+1)*ow) - wx(X, k), summing to cw over k; wy(Y, r) is the same with rh, oh.  T = cw * rh.  N_c is the sum of wy * wx * channel c over
// the rectangle, M_c the sum of wy * wx * channel c * alpha (c = 0..2).
//   PLAIN           every channel is (N_c + T/2) / T - integer divisions: floor, a half rounds up; one rounding, no intermediate
//   ALPHA_WEIGHTED  alpha is (N_3 + T/2) / T; with A = N_3 > 0 the colours are (M_c + A/2) / A; with A == 0 they are the PLAIN value
// Pixel (X, Y) of that result is written at pixel (FLIP_X ? ow - 1 - X : X, FLIP_Y ? oh - 1 - Y : Y) of the output, och = 3 or 4 bytes per
// pixel, tightly packed from the absolute address q.
// One weight wy * wx is at most min(cw, ow) * min(rh, oh) <= T < 400 000 000: 32 bits.  N_c <= 255 * T < 2^37 and M_c <= 255 * 255 * T < 2^45:
// the sums are 64-bit, each tap one 32 x 32 -> 64 multiply-add.
//
// The split: an output column overlaps at most resize_taps(cw, ow) <= 65 source columns (cw <= 64 * ow).  They are shared by L = 1 << lg <= 16
// neighbouring lanes, c = ceil(taps / L) columns each (at most 4; 5 for 65 taps); work item (Y * ow + X) * L + l is lane l's share: the
// columns [k0 + l*c, + c) with a weight, k0 = X*cw / ow, in every row with a weight.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_resize.hip: real loads and stores, the lanes' sums added with butterfly steps) and - by tests/host/resize_host.cpp only - for the
// host, where the functor checks and counts every access, so the whole walk is compared with the Python model on the CPU before it runs on a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QOIMI_RESIZE_HD __host__ __device__ __forceinline__
#else
#define QOIMI_RESIZE_HD inline
#endif
#if defined(__clang__)
#define QOIMI_RESIZE_UNROLL _Pragma("unroll")
#else
#define QOIMI_RESIZE_UNROLL
#endif

namespace qoimi {

constexpr uint32_t kResizeThreads = 256;      // work items of a tile: the workgroup of resize_filter
constexpr uint32_t kResizeFlipX = 1, kResizeFlipY = 2;
constexpr uint32_t kResizeMaxRatio = 64;
constexpr uint32_t kResizeMaxLg = 4;          // 16 lanes per output pixel at most
constexpr uint32_t kResizeMaxCols = 5;        // ceil(65 / 16)

// w: pixels per staged row; (x, y, cw, rh): the rectangle; ow x oh: the output; flags: kResizeFlip*
struct ResizeGeom { uint32_t w, x, y, cw, rh, ow, oh, flags; };
// S[c]: sum of weight * channel c (r, g, b, a); W[c]: sum of weight * channel c * alpha
struct ResizeSums { uint64_t S[4], W[3]; };

// n / d, d >= 1: the 32-bit division where both fit
QOIMI_RESIZE_HD uint64_t resize_div(uint64_t n, uint64_t d) {
    if (((n | d) >> 32) == 0u) return (uint32_t)n / (uint32_t)d;
    return n / d;
}

// An upper bound of the source columns one output column overlaps: cw / ow where that is whole, else two more than the floor.
QOIMI_RESIZE_HD uint32_t resize_taps(uint32_t cw, uint32_t ow) { return cw / ow + (cw % ow != 0u ? 2u : 0u); }

// How an output pixel's columns are split over lanes: lg = log2(L), c = columns per lane.
QOIMI_RESIZE_HD void resize_split(uint32_t cw, uint32_t ow, uint32_t& lg, uint32_t& c) {
    const uint32_t t = resize_taps(cw, ow);
    lg = 0;
    while (lg < kResizeMaxLg && ((t + (1u << lg) - 1u) >> lg) > 4u) ++lg;
    c = (t + (1u << lg) - 1u) >> lg;
}

// Tiles of kResizeThreads work items of an item (ow * oh * L of them); 2^32 for an output no call accepts (2^40 pixels or more).
QOIMI_RESIZE_HD uint64_t resize_tiles(uint32_t cw, uint32_t ow, uint32_t oh) {
    uint32_t lg, c;
    resize_split(cw, ow, lg, c);
    const uint64_t px = (uint64_t)ow * oh;
    if (px >= (1ull << 40)) return 1ull << 32;
    return ((px << lg) + kResizeThreads - 1u) / kResizeThreads;
}

// The overlap of [lo, lo + len) with [a, a + step)
QOIMI_RESIZE_HD uint32_t resize_overlap(uint64_t lo, uint64_t len, uint64_t a, uint64_t step) {
    const uint64_t b = lo > a ? lo : a, e = lo + len < a + step ? lo + len : a + step;
    return e > b ? (uint32_t)(e - b) : 0u;
}

// All sums at zero
QOIMI_RESIZE_HD void resize_zero(ResizeSums& s) {
    QOIMI_RESIZE_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) s.S[i] = 0u;
    QOIMI_RESIZE_UNROLL
    for (uint32_t i = 0; i < 3u; ++i) s.W[i] = 0u;
}

// One tap: staged pixel px with the weight wgt (32 bits) into the sums - what every filter over ResizeSums does per pixel it loads.
template <bool WEIGHTED>
QOIMI_RESIZE_HD void resize_tap(ResizeSums& s, uint32_t px, uint32_t wgt) {
    const uint32_t al = px >> 24;
    s.S[0] += (uint64_t)wgt * (px & 255u); s.S[1] += (uint64_t)wgt * ((px >> 8) & 255u);
    s.S[2] += (uint64_t)wgt * ((px >> 16) & 255u); s.S[3] += (uint64_t)wgt * al;
    if (WEIGHTED) {
        s.W[0] += (uint64_t)wgt * ((px & 255u) * al); s.W[1] += (uint64_t)wgt * (((px >> 8) & 255u) * al);
        s.W[2] += (uint64_t)wgt * (((px >> 16) & 255u) * al);
    }
}

// Lane l's share of output pixel (X, Y) of the unflipped result: c columns from k0 + l * c (lg, c: resize_split), every row with a weight.
// Only pixels with a weight are loaded: columns below cw, rows below rh of the rectangle.
template <bool WEIGHTED, class Mem>
QOIMI_RESIZE_HD void resize_lane(const Mem& mem, const ResizeGeom& g, uint32_t X, uint32_t Y, uint32_t l, uint32_t c, ResizeSums& s) {
    resize_zero(s);
    const uint64_t xlo = (uint64_t)X * g.cw, ylo = (uint64_t)Y * g.rh;
    const uint32_t k0 = (uint32_t)resize_div(xlo, g.ow) + l * c;
    uint32_t wx[kResizeMaxCols];
    QOIMI_RESIZE_UNROLL
    for (uint32_t j = 0; j < kResizeMaxCols; ++j) wx[j] = j < c ? resize_overlap(xlo, g.cw, (uint64_t)(k0 + j) * g.ow, g.ow) : 0u;
    if (wx[0] == 0u) return;                                   // (the weights of a pixel's columns are contiguous: nothing is left for this lane)
    uint32_t r = (uint32_t)resize_div(ylo, g.oh);
    for (uint64_t a = (uint64_t)r * g.oh;; ++r, a += g.oh) {
        const uint32_t wy = resize_overlap(ylo, g.rh, a, g.oh);
        if (wy == 0u) break;                                   // (the first row has a weight; behind the last one a >= ylo + rh)
        const uint64_t at = (uint64_t)(g.y + r) * g.w + g.x + k0;
        QOIMI_RESIZE_UNROLL
        for (uint32_t j = 0; j < kResizeMaxCols; ++j) {
            if (wx[j] == 0u) continue;
            resize_tap<WEIGHTED>(s, mem.load(at + j), wy * wx[j]);
        }
    }
}

// (n + d/2) / d for d >= 1; a power of two is a shift.
QOIMI_RESIZE_HD uint32_t resize_div_round(uint64_t n, uint64_t d) {
    n += d >> 1;
    if ((d & (d - 1u)) == 0u) return (uint32_t)(n >> (uint32_t)__builtin_ctzll(d));
    return (uint32_t)resize_div(n, d);
}

// The output pixel as r | g << 8 | b << 16 | a << 24 from the sums over all its taps.  weighted: QOIMI_RESIZE_ALPHA_WEIGHTED (the caller passes
// false for 3 output channels).
QOIMI_RESIZE_HD uint32_t resize_pixel(const ResizeSums& s, uint64_t T, bool weighted) {
    const uint32_t a = resize_div_round(s.S[3], T);
    uint32_t c[3];
    if (weighted && s.S[3] != 0u) {
        for (int k = 0; k < 3; ++k) c[k] = resize_div_round(s.W[k], s.S[3]);
    } else {
        for (int k = 0; k < 3; ++k) c[k] = resize_div_round(s.S[k], T);
    }
    return c[0] | (c[1] << 8) | (c[2] << 16) | (a << 24);
}

// Pixel px = (X, Y) of the unflipped result to its place in the output at q: one dword where the output holds 4 bytes per pixel and the address
// is aligned, else och bytes - the item's own bytes only, never a word that would have to be read first.
template <class Mem>
QOIMI_RESIZE_HD void resize_store(const Mem& mem, const ResizeGeom& g, uint64_t q, uint32_t och, uint32_t X, uint32_t Y, uint32_t px) {
    const uint32_t xo = (g.flags & kResizeFlipX) != 0u ? g.ow - 1u - X : X, yo = (g.flags & kResizeFlipY) != 0u ? g.oh - 1u - Y : Y;
    const uint64_t a = q + ((uint64_t)yo * g.ow + xo) * och;
    if (och == 4u && (a & 3u) == 0u) { mem.store4(a, px); return; }
    mem.store1(a, px); mem.store1(a + 1u, px >> 8); mem.store1(a + 2u, px >> 16);
    if (och == 4u) mem.store1(a + 3u, px >> 24);
}

// The finish step of a filter tile as a sink - pixel px = (X, Y) of the unflipped result to the output at q - for the calls that write bytes
// (qoi_tensor_core.h: TensorSink is the other one).
struct ResizeByteSink {
    template <class Mem>
    QOIMI_RESIZE_HD void operator()(const Mem& mem, const ResizeGeom& g, uint64_t q, uint32_t och, uint32_t X, uint32_t Y, uint32_t px) const {
        resize_store(mem, g, q, och, X, Y, px);
    }
};

// The sums of pixel (X, Y) divided by T = cw * rh and stored (resize_store).
template <class Mem>
QOIMI_RESIZE_HD void resize_finish(const Mem& mem, const ResizeGeom& g, uint64_t q, uint32_t och, bool weighted, uint32_t X, uint32_t Y, const ResizeSums& s) {
    resize_store(mem, g, q, och, X, Y, resize_pixel(s, (uint64_t)g.cw * g.rh, weighted));
}

}  // namespace qoimi

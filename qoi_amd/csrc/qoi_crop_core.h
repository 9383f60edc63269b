// qoi_crop_core.h — the item arithmetic of qoimi_decode_crops: which bytes of a crop's output an item covers, which staged pixels they come
// from, how the 16 bytes of a word are put together and with which stores they are written.
//
// The definition (normative; qoi_amd/crops.py states it in Python).  A crop cw x ch at (x, y) of an image staged as rows of w pixels of 4 bytes
// is written as B = cw * ch * och bytes, row-major, at the absolute address q; output pixel (r, c) is the source pixel
// (FLIP_Y ? y + ch - 1 - r : y + r,  FLIP_X ? x + cw - 1 - c : x + c), its alpha dropped at och == 3.  An ITEM is one aligned 16-byte word that
// [q, q + B) touches: a crop has ((q + B + 15) >> 4) - (q >> 4) of them, item k covers the output bytes [16 * ((q >> 4) + k) - q, + 16) cut to
// [0, B).  A word wholly inside the output is one 16-byte store; the first and the last word of a crop can be partial and are written with
// 1-, 2- and 4-byte stores of the crop's own bytes, each naturally aligned - never a read-modify-write, so two crops may share a word.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store2 / store4 / store16(address, ...)), compiled
// for the device by hipcc (qoi_crop.hip: real loads and stores) and - by tests/host/crop_host.cpp only - for the host, where the functor
// counts what is written, so the whole item loop is compared with the Python model on the CPU before it runs on a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QOIMI_CROP_HD __host__ __device__ __forceinline__
#else
#define QOIMI_CROP_HD inline
#endif
#if defined(__clang__)
#define QOIMI_CROP_UNROLL _Pragma("unroll")
#else
#define QOIMI_CROP_UNROLL
#endif

namespace qoimi {

constexpr uint32_t kCropThreads = 256;        // items of a tile: the workgroup of crop_gather
constexpr uint32_t kCropFlipX = 1, kCropFlipY = 2;

// w: pixels per staged row; (x, y, cw, ch): the rectangle; flags: kCropFlip*
struct CropRect { uint32_t w, x, y, cw, ch, flags; };

// Items of an output of B >= 1 bytes at address q, and the tiles of kCropThreads items they take.
QOIMI_CROP_HD uint64_t crop_items(uint64_t q, uint64_t B) { return ((q + B + 15u) >> 4) - (q >> 4); }
QOIMI_CROP_HD uint64_t crop_tiles(uint64_t q, uint64_t B) { return (crop_items(q, B) + kCropThreads - 1u) / kCropThreads; }

// The low dword of {hi, lo} >> 8 * s, s = 0..3.
QOIMI_CROP_HD uint32_t crop_align(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * s));
#endif
}

// W = the output bytes [b0, b0 + n), 1 <= n <= 16, b0 + n <= B: byte t of them is byte t & 3 of W[t >> 2].  Only the pixels those bytes come
// from are loaded (at most 6 at OCH == 3, 5 at OCH == 4): one division by the crop's width, then the walk steps from pixel to pixel.
template <uint32_t OCH, class Mem>
QOIMI_CROP_HD void crop_word(const Mem& mem, const CropRect& g, uint32_t b0, uint32_t n, uint32_t (&W)[4]) {
    constexpr uint32_t kMost = OCH == 3u ? 6u : 5u;
    const uint32_t p = b0 / OCH, sub = b0 - p * OCH;
    const uint32_t np = (sub + n + OCH - 1u) / OCH;
    const uint32_t r = p / g.cw;
    uint32_t c = p - r * g.cw;
    const bool fx = (g.flags & kCropFlipX) != 0u, fy = (g.flags & kCropFlipY) != 0u;
    const int64_t dx = fx ? -1 : 1, row = (fy ? -(int64_t)g.w : (int64_t)g.w) - dx * (int64_t)g.cw;   // from behind a row's last pixel to the next row's first
    int64_t at = (int64_t)(fy ? g.y + g.ch - 1u - r : g.y + r) * (int64_t)g.w + (int64_t)(fx ? g.x + g.cw - 1u - c : g.x + c);
    uint32_t px[kMost];
    QOIMI_CROP_UNROLL
    for (uint32_t i = 0; i < kMost; ++i) {
        px[i] = 0u;
        if (i < np) {
            px[i] = mem.load((uint64_t)at);
            at += dx;
            if (++c == g.cw) { c = 0u; at += row; }
        }
    }
    if (OCH == 4u) {
        QOIMI_CROP_UNROLL
        for (uint32_t i = 0; i < 4u; ++i) W[i] = crop_align(px[i + 1u], px[i], sub);
    } else {
        uint32_t m[kMost], P[5];
        QOIMI_CROP_UNROLL
        for (uint32_t i = 0; i < kMost; ++i) m[i] = px[i] & 0x00FFFFFFu;
        P[0] = m[0] | (m[1] << 24); P[1] = (m[1] >> 8) | (m[2] << 16); P[2] = (m[2] >> 16) | (m[3] << 8);
        P[3] = m[4] | (m[5 % kMost] << 24); P[4] = m[5 % kMost] >> 8;
        QOIMI_CROP_UNROLL
        for (uint32_t i = 0; i < 4u; ++i) W[i] = crop_align(P[i + 1u], P[i], sub);
    }
}

// W >> 8 * s over all four dwords, s = 1..3
QOIMI_CROP_HD void crop_shift(uint32_t (&W)[4], uint32_t s) {
    W[0] = crop_align(W[1], W[0], s); W[1] = crop_align(W[2], W[1], s); W[2] = crop_align(W[3], W[2], s); W[3] >>= 8u * s;
}

// The first n bytes of W to the address a.  n == 16 (then a is a multiple of 16): one store.  Else the largest naturally aligned pieces:
// a byte and a halfword up to a dword boundary, dwords, a halfword and a byte behind them.
template <class Mem>
QOIMI_CROP_HD void crop_store(const Mem& mem, uint64_t a, uint32_t n, uint32_t (&W)[4]) {
    if (n == 16u) { mem.store16(a, W); return; }
    if ((a & 1u) != 0u) { mem.store1(a, W[0]); crop_shift(W, 1u); a += 1u; n -= 1u; }      // (n >= 1)
    if ((a & 2u) != 0u && n >= 2u) { mem.store2(a, W[0]); crop_shift(W, 2u); a += 2u; n -= 2u; }
    QOIMI_CROP_UNROLL
    for (uint32_t i = 0; i < 3u; ++i)
        if (n >= 4u) { mem.store4(a, W[0]); W[0] = W[1]; W[1] = W[2]; W[2] = W[3]; a += 4u; n -= 4u; }
    if (n >= 2u) { mem.store2(a, W[0]); crop_shift(W, 2u); a += 2u; n -= 2u; }
    if (n >= 1u) mem.store1(a, W[0]);
}

// Item k < crop_items(q, B) of a crop whose output of B = cw * ch * OCH bytes begins at the address q.
template <uint32_t OCH, class Mem>
QOIMI_CROP_HD void crop_item(const Mem& mem, const CropRect& g, uint64_t q, uint32_t B, uint32_t k) {
    const int64_t lo = (int64_t)16 * (int64_t)k - (int64_t)(q & 15u);        // the word's first byte as a byte of the output
    const uint32_t b0 = lo < 0 ? 0u : (uint32_t)lo;
    const uint32_t b1 = lo + 16 < (int64_t)B ? (uint32_t)(lo + 16) : B;
    uint32_t W[4];
    crop_word<OCH>(mem, g, b0, b1 - b0, W);
    crop_store(mem, q + b0, b1 - b0, W);
}

}  // namespace qoimi

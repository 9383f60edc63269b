// qoi_ingest_core.h — tensors as the source of qoimi_encode_tiles (QOIMI_TILE_SRC): the item arithmetic of the kernel tensor_ingest, which a
// tensor call runs in tile_gather's place - which elements an item reads, how an element becomes a byte, how four pixels become the dwords
// of the slot.
//
// The definition (normative; qoi_amd/tiles.py: convert states it in Python).  The image a tile names is a tensor of w x h pixels of sch = 3
// or 4 elements: u8, binary16, bfloat16 or binary32 (element size E = 1 / 2 / 2 / 4), tightly packed at an address that is a multiple of
// E; element (c, Y, X) stands at element index (Y * w + X) * sch + c (HWC) or (c * h + Y) * w + X (CHW).  x is the element widened exactly
// to binary32 (f16 and bf16 widen without rounding).
//   UNIT        t = x * 255.0f, rounded to binary32
//   SYMMETRIC   m = x * 127.5f, rounded; t = m + 127.5f, rounded - TWO roundings, never a fused multiply-add (qoi_tensor_core.h's convention)
//   BYTES       t = x
//   U8          the byte is the element
// The byte is 0 if t is NaN or t <= 0 (-inf and -0.0 with them), 255 if t >= 255 (+inf with them), otherwise t rounded to the nearest
// integer, ties to even.  Every channel, alpha included, goes the same way.  Whether subnormals are flushed cannot change a byte: |t| < 0.5
// gives 0 either way.  B, the h x w x sch byte image this defines, then is what qoi_tile_core.h's f == 1 tile takes: the rectangle, the
// flips, och (4 to 3 drops alpha, 3 to 4 sets 255).  Tensor sources have factor 1 only.
//
// An ITEM is kIngestPixels = 4 consecutive pixels of the tile's OUTPUT in output order: 12 or 16 bytes at a dword-aligned address of the
// 256-aligned slot, stored as whole dwords - one 16-byte store at och == 4, one 12-byte store at och == 3 (the last item of an och == 3
// tile stores only the dwords that hold one of the tile's bytes; at och == 4 a last item may store behind the tile's bytes inside the
// slot's padding, as tile_copy_item does).  256 items to a tile of the walk (kTileThreads), ceil(cw * ch / 4) items to an entry.
// Consecutive lanes hold consecutive pixels of a row of the rectangle.  CHW: where an item's four pixels lie in one row, each plane gives
// them as four consecutive elements - one load of 4 * E bytes where that address is a multiple of 4 * E, else element by element (u8: the
// two aligned dwords that hold them).  HWC: a pixel of four elements is one load of 4 * E bytes where its address is a multiple of that,
// else element by element; a u8 pixel is tile_fetch's one or two aligned dwords.  Nothing is read but whole, naturally aligned elements of
// the image - for u8 the aligned dwords that hold one of its bytes.
//
// The table entry is qoi_tile_core.h's TileEntry, 56 bytes, with kind kTileKindIngest in cfg; an ingest entry has tw = cw, th = ch and - the
// factor being 1 - holds the image's HEIGHT in `f` (the plane pitch of CHW).  The format stands in bits 0..15 of cfg, which the other kinds
// use for their lane split: ingest_cfg.
//
// Plain sequential code over a memory functor `Mem` (load2 / load4(aligned address) -> the 2 / 4 bytes, load8 / load16(aligned address,
// dwords), store4 / store12 / store16(address, dwords)), compiled for the device by hipcc (qoi_ingest.hip) and - by tests/host/ingest_host.cpp
// only - for the host, where the functor checks every address against the image and the slot.
#pragma once
#include <stdint.h>

#include "qoi_tile_core.h"

namespace qoimi {

constexpr uint32_t kTileKindIngest = 3;
constexpr uint32_t kIngestPixels = 4;                      // output pixels of an item

// qoimi_tile.flags: the source format of a tensor call
constexpr uint32_t kTileSrc = 16, kTileSrcCHW = 32, kTileSrcDtypeShift = 6, kTileSrcRangeShift = 8;
constexpr uint32_t kTileSrcMask = kTileSrc | kTileSrcCHW | (3u << kTileSrcDtypeShift) | (3u << kTileSrcRangeShift);
constexpr uint32_t kIngestU8 = 0, kIngestF16 = 1, kIngestBF16 = 2, kIngestF32 = 3;     // QOIMI_TENSOR_U8 .. _F32
constexpr uint32_t kIngestUnit = 0, kIngestSymmetric = 1, kIngestBytes = 2;            // (3 is not a range)

QOIMI_CROP_HD uint32_t ingest_dtype(uint32_t src_flags) { return (src_flags >> kTileSrcDtypeShift) & 3u; }
QOIMI_CROP_HD uint32_t ingest_range(uint32_t src_flags) { return (src_flags >> kTileSrcRangeShift) & 3u; }
QOIMI_CROP_HD uint32_t ingest_elem(uint32_t dtype) { return dtype == kIngestU8 ? 1u : dtype == kIngestF32 ? 4u : 2u; }

// cfg of an ingest entry: dtype | chw << 2 | range << 3 | sch << 16 | och << 20 | kTileKindIngest << 25 | flips << 28
QOIMI_CROP_HD uint32_t ingest_cfg(uint32_t src_flags, uint32_t sch, uint32_t och, uint32_t flags) {
    return ingest_dtype(src_flags) | ((src_flags & kTileSrcCHW) != 0u ? 4u : 0u) | (ingest_range(src_flags) << 3) | (sch << 16) | (och << 20) |
           (kTileKindIngest << 25) | ((flags & (kCropFlipX | kCropFlipY)) << 28);
}

// Items of a tile of cw x ch pixels (cw * ch < 400 000 000) and the tiles of kTileThreads items they take.
QOIMI_CROP_HD uint64_t ingest_items(uint32_t cw, uint32_t ch) { return ((uint64_t)cw * ch + kIngestPixels - 1u) / kIngestPixels; }
QOIMI_CROP_HD uint64_t ingest_tiles(uint32_t cw, uint32_t ch) { return (ingest_items(cw, ch) + kTileThreads - 1u) / kTileThreads; }

QOIMI_CROP_HD float ingest_float(uint32_t bits) { float f; __builtin_memcpy(&f, &bits, 4); return f; }

// The element with the bits `bits` widened exactly to binary32.
QOIMI_CROP_HD float ingest_widen(uint32_t bits, uint32_t dtype) {
    if (dtype == kIngestF32) return ingest_float(bits);
    if (dtype == kIngestBF16) return ingest_float(bits << 16);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint16_t u = (uint16_t)bits; _Float16 h; __builtin_memcpy(&h, &u, 2); return (float)h;
#else
    const uint32_t sign = (bits & 0x8000u) << 16, e = (bits >> 10) & 31u, m = bits & 0x3FFu;
    if (e == 31u) return ingest_float(sign | 0x7F800000u | (m << 13));             // infinity, NaN
    if (e != 0u) return ingest_float(sign | ((e + 112u) << 23) | (m << 13));
    const float v = (float)m * 5.9604644775390625e-08f;                            // m * 2^-24: exact
    return sign != 0u ? -v : v;
#endif
}

QOIMI_CROP_HD float ingest_rint(float t) { return __builtin_rintf(t); }            // (v_rndne_f32; the host runs in round-to-nearest)

// x * 127.5 + 127.5 with both roundings
QOIMI_CROP_HD float ingest_symmetric(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)                                     // (whatever the build's -ffp-contract says)
    const float m = x * 127.5f;
    return m + 127.5f;
#else
    float m = x * 127.5f;
    __asm__ volatile("" : "+m"(m));                                // (the product is rounded before the sum sees it: no contraction)
    return m + 127.5f;
#endif
}

// The byte of the float element x.
QOIMI_CROP_HD uint32_t ingest_byte(float x, uint32_t range) {
    const float t = range == kIngestUnit ? x * 255.0f : range == kIngestSymmetric ? ingest_symmetric(x) : x;
    if (!(t > 0.0f)) return 0u;                                    // NaN, -inf, -0.0
    if (t >= 255.0f) return 255u;
    return (uint32_t)ingest_rint(t);
}

// The byte of the element with the bits `bits`.
template <uint32_t DT>
QOIMI_CROP_HD uint32_t ingest_element(uint32_t bits, uint32_t range) {
    return DT == kIngestU8 ? bits & 255u : ingest_byte(ingest_widen(bits, DT), range);
}

// One element of E bytes at the address a (a multiple of E) as its bits; a byte comes out of the aligned dword that holds it.
template <uint32_t DT, class Mem>
QOIMI_CROP_HD uint32_t ingest_load(const Mem& mem, uint64_t a) {
    if (DT == kIngestU8) return (mem.load4(a & ~(uint64_t)3u) >> (8u * ((uint32_t)a & 3u))) & 255u;
    if (DT == kIngestF32) return mem.load4(a);
    return mem.load2(a);
}

// Four consecutive elements from the address a (a multiple of E) as their bits.
template <uint32_t DT, class Mem>
QOIMI_CROP_HD void ingest_load_run(const Mem& mem, uint64_t a, uint32_t (&v)[4]) {
    if (DT == kIngestU8) {
        const uint32_t s = (uint32_t)a & 3u;
        const uint32_t lo = mem.load4(a - s), hi = s != 0u ? mem.load4(a - s + 4u) : 0u;
        const uint32_t w = crop_align(hi, lo, s);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
    } else if (DT == kIngestF32) {
        if ((a & 15u) == 0u) mem.load16(a, v);
        else { v[0] = mem.load4(a); v[1] = mem.load4(a + 4u); v[2] = mem.load4(a + 8u); v[3] = mem.load4(a + 12u); }
    } else {
        if ((a & 7u) == 0u) {
            uint32_t w[2];
            mem.load8(a, w);
            v[0] = w[0] & 0xFFFFu; v[1] = w[0] >> 16; v[2] = w[1] & 0xFFFFu; v[3] = w[1] >> 16;
        } else { v[0] = mem.load2(a); v[1] = mem.load2(a + 2u); v[2] = mem.load2(a + 4u); v[3] = mem.load2(a + 6u); }
    }
}

// The pixel at (col, row) of the image at `base` as r | g << 8 | b << 16 | a << 24 (a = 255 at SCH == 3).
template <uint32_t DT, bool CHW, uint32_t SCH, class Mem>
QOIMI_CROP_HD uint32_t ingest_pixel(const Mem& mem, const TileEntry& e, uint64_t base, uint64_t row, uint64_t col, uint32_t range) {
    constexpr uint32_t E = DT == kIngestU8 ? 1u : DT == kIngestF32 ? 4u : 2u;
    const uint64_t at = row * e.w + col;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (CHW) {
        const uint64_t plane = (uint64_t)e.f * e.w;                                // (f holds the image's height)
        QOIMI_CROP_UNROLL
        for (uint32_t c = 0; c < SCH; ++c) v[c] = ingest_load<DT>(mem, base + (c * plane + at) * E);
    } else {
        const uint64_t A = base + at * (SCH * E);
        if (DT == kIngestU8) return tile_fetch<SCH>(mem, A);
        if (SCH == 4u) ingest_load_run<DT>(mem, A, v);
        else {
            QOIMI_CROP_UNROLL
            for (uint32_t c = 0; c < SCH; ++c) v[c] = ingest_load<DT>(mem, A + c * E);
        }
    }
    uint32_t px = SCH == 3u ? 0xFF000000u : 0u;
    QOIMI_CROP_UNROLL
    for (uint32_t c = 0; c < SCH; ++c) px |= ingest_element<DT>(v[c], range) << (8u * c);
    return px;
}

// Item k < ingest_items of the entry e, whose image begins at the address `base` and whose output begins at the 256-aligned address q.
template <uint32_t DT, bool CHW, uint32_t SCH, class Mem>
QOIMI_CROP_HD void ingest_item(const Mem& mem, const TileEntry& e, uint64_t base, uint64_t q, uint32_t k) {
    constexpr uint32_t E = DT == kIngestU8 ? 1u : DT == kIngestF32 ? 4u : 2u;
    const uint32_t range = (e.cfg >> 3) & 3u, och = (e.cfg >> 20) & 15u, flags = e.cfg >> 28;
    const bool fx = (flags & kCropFlipX) != 0u, fy = (flags & kCropFlipY) != 0u;
    const uint32_t P = e.cw * e.ch, p0 = kIngestPixels * k;                      // (an image holds fewer than 400 000 000 pixels)
    const uint32_t n = P - p0 < kIngestPixels ? P - p0 : kIngestPixels;
    uint32_t r = p0 / e.cw, c = p0 - r * e.cw;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    if (CHW && n == kIngestPixels && c + kIngestPixels <= e.cw) {                // four pixels of one row: a run of four elements per plane
        const uint64_t row = fy ? e.y + e.ch - 1u - r : e.y + r, col = fx ? e.x + e.cw - kIngestPixels - c : e.x + c;     // the lowest of the four
        const uint64_t plane = (uint64_t)e.f * e.w, at = row * e.w + col;
        QOIMI_CROP_UNROLL
        for (uint32_t s = 0; s < SCH; ++s) {
            uint32_t v[4];
            ingest_load_run<DT>(mem, base + (s * plane + at) * E, v);
            QOIMI_CROP_UNROLL
            for (uint32_t j = 0; j < 4u; ++j) px[j] |= ingest_element<DT>(v[fx ? 3u - j : j], range) << (8u * s);
        }
        if (SCH == 3u) { px[0] |= 0xFF000000u; px[1] |= 0xFF000000u; px[2] |= 0xFF000000u; px[3] |= 0xFF000000u; }
    } else {
        QOIMI_CROP_UNROLL
        for (uint32_t j = 0; j < 4u; ++j) {
            if (j < n) {
                const uint64_t row = fy ? e.y + e.ch - 1u - r : e.y + r, col = fx ? e.x + e.cw - 1u - c : e.x + c;
                px[j] = ingest_pixel<DT, CHW, SCH>(mem, e, base, row, col, range);
                if (++c == e.cw) { c = 0u; ++r; }
            }
        }
    }
    if (och == 4u) { mem.store16(q + 16u * (uint64_t)k, px); return; }
    uint32_t W[3];
    const uint32_t a0 = px[0] & 0xFFFFFFu, a1 = px[1] & 0xFFFFFFu, a2 = px[2] & 0xFFFFFFu, a3 = px[3] & 0xFFFFFFu;
    W[0] = a0 | (a1 << 24); W[1] = (a1 >> 8) | (a2 << 16); W[2] = (a2 >> 16) | (a3 << 8);
    const uint64_t a = q + 12u * (uint64_t)k;
    if (n == kIngestPixels) { mem.store12(a, W); return; }
    const uint32_t nd = (3u * n + 3u) >> 2;                                      // the dwords that hold one of the tile's bytes
    QOIMI_CROP_UNROLL
    for (uint32_t d = 0; d < 3u; ++d)
        if (d < nd) mem.store4(a + 4u * d, W[d]);
}

}  // namespace qoimi

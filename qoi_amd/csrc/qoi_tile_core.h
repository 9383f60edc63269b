// qoi_tile_core.h — the item arithmetic of qoimi_encode_tiles: the table entry of a tile, its items and tiles, which source bytes an item
// reads and how a pixel is put together from aligned dwords.
//
// The definition (normative; qoi_amd/tiles.py: tile states it in Python).  The source image stands in the CALLER's memory as rows of w pixels
// of sch = 3 or 4 bytes, tightly packed, at any byte address; the tile's rectangle cw x ch at (x, y) is box-reduced by f (qoi_thumb_core.h:
// the blocks, the sums, the division - a 3-byte pixel enters the sums with alpha 255), which gives tw x th pixels; pixel (X, Y) of them goes
// to (FLIP_X ? tw - 1 - X : X, FLIP_Y ? th - 1 - Y : Y) of the output, which is written tightly packed with och = 3 or 4 bytes per pixel
// (alpha dropped, or 255 behind a 3-byte source) at a 256-aligned slot of the context's staging arena.
//
// Two kinds of items, 256 to a tile (the workgroup of tile_gather):
//   f == 1   a strided copy.  An ITEM is one aligned 16-byte word of the output (the slot is 256-aligned and rounded up to 256 bytes, so
//            every word is stored whole; what a last word holds behind the tile's bytes is not looked at by anyone).  The pixels of a word
//            are found as qoi_crop_core.h: crop_word finds them - one division by the tile's width, then a walk - and fetched from the
//            caller's memory; four 4-byte pixels of one row at a 16-byte aligned address are one 16-byte load.
//   f >= 2   the lane split of qoi_thumb_core.h unchanged: an ITEM is one lane's share (at most 4 columns) of a block, the rectangle taking
//            the place of the image.
// A pixel at the byte address A is read as the aligned dword that holds A and - only where the pixel reaches into it - the next one: never
// a word that holds no byte of the image.
// The two reductions for label maps - a selection and a majority vote in the place of the box average - stand at the end of this file.
//
// Plain sequential code over a memory functor `Mem` (load4(aligned address) -> dword, load16(16-aligned address, dwords), store16(address,
// dwords)), compiled for the device by hipcc (qoi_tile.hip) and - by tests/host/tile_host.cpp only - for the host, where the functor checks
// every address against the image, so the whole item loop is compared with the Python model on the CPU before it runs on a GPU.
#pragma once
#include <stdint.h>

#include "qoi_crop_core.h"
#include "qoi_mode_core.h"
#include "qoi_thumb_core.h"

namespace qoimi {

constexpr uint32_t kTileThreads = 256;        // items of a tile: the workgroup of tile_gather
static_assert(kTileThreads == kThumbThreads, "thumb_tiles counts tiles of that many items");

// One tile of the call.  src_off: the image's first byte from d_pixels; dst_off: the pixel part of the tile's slot from the staging's
// start (a multiple of 256); w: pixels per source row; (x, y, cw, ch): the rectangle; tw x th: the output; f: the factor.
// cfg: log2(L) | c << 8 (thumb_split of f) | sch << 16 | och << 20 | (alpha weighted ? 1 : 0) << 24 | flags << 28
struct TileEntry { uint64_t src_off, dst_off; uint32_t w, x, y, cw, ch, tw, th, f, first_tile, cfg; };
static_assert(sizeof(TileEntry) == 56, "table layout");

QOIMI_CROP_HD uint32_t tile_cfg(uint32_t f, uint32_t sch, uint32_t och, bool weighted, uint32_t flags) {
    uint32_t lg, c;
    thumb_split(f, lg, c);
    return lg | (c << 8) | (sch << 16) | (och << 20) | ((weighted ? 1u : 0u) << 24) | (flags << 28);
}

// Items of a tile of tw x th output pixels (its rectangle: cw x ch) and the tiles of kTileThreads items they take.
QOIMI_CROP_HD uint64_t tile_items(uint32_t cw, uint32_t ch, uint32_t f, uint32_t och) {
    if (f == 1u) return ((uint64_t)cw * ch * och + 15u) >> 4;
    uint32_t lg, c;
    thumb_split(f, lg, c);
    return ((uint64_t)thumb_extent(cw, f) * thumb_extent(ch, f)) << lg;
}
QOIMI_CROP_HD uint64_t tile_tiles(uint32_t cw, uint32_t ch, uint32_t f, uint32_t och) { return (tile_items(cw, ch, f, och) + kTileThreads - 1u) / kTileThreads; }

// The pixel of SCH bytes at the byte address A as r | g << 8 | b << 16 | a << 24 (a = 255 at SCH == 3).
template <uint32_t SCH, class Mem>
QOIMI_CROP_HD uint32_t tile_fetch(const Mem& mem, uint64_t A) {
    const uint32_t s = (uint32_t)A & 3u;
    const uint64_t a = A - s;
    const uint32_t lo = mem.load4(a);
    const uint32_t hi = s + SCH > 4u ? mem.load4(a + 4u) : 0u;
    const uint32_t px = crop_align(hi, lo, s);
    return SCH == 3u ? px | 0xFF000000u : px;
}

// crop_word's memory: pixel i of the image at `base`.
template <uint32_t SCH, class Mem>
struct TilePixels {
    const Mem& mem; uint64_t base;
    QOIMI_CROP_HD uint32_t load(uint64_t i) const { return tile_fetch<SCH>(mem, base + i * SCH); }
};

// f == 1: item k < tile_items of a tile whose image begins at the address `base` and whose output begins at the 16-aligned address q.
template <uint32_t SCH, uint32_t OCH, class Mem>
QOIMI_CROP_HD void tile_copy_item(const Mem& mem, const TileEntry& e, uint64_t base, uint64_t q, uint32_t k) {
    const uint32_t flags = e.cfg >> 28;
    const uint32_t B = e.cw * e.ch * OCH, b0 = 16u * k;            // (an image holds fewer than 400 000 000 pixels)
    const uint32_t n = B - b0 < 16u ? B - b0 : 16u;
    uint32_t W[4];
    if (SCH == 4u && OCH == 4u && n == 16u) {                    // four whole pixels: one load where they are neighbours at an aligned address
        const uint32_t p = b0 >> 2, r = p / e.cw, c = p - r * e.cw;
        if (c + 4u <= e.cw) {
            const bool fx = (flags & kCropFlipX) != 0u, fy = (flags & kCropFlipY) != 0u;
            const uint64_t row = fy ? e.y + e.ch - 1u - r : e.y + r, col = fx ? e.x + e.cw - 4u - c : e.x + c;   // the lowest of the four
            const uint64_t A = base + (row * e.w + col) * 4u;
            if ((A & 15u) == 0u) {
                mem.load16(A, W);
                if (fx) { uint32_t t = W[0]; W[0] = W[3]; W[3] = t; t = W[1]; W[1] = W[2]; W[2] = t; }
                mem.store16(q + b0, W);
                return;
            }
        }
    }
    const CropRect g = {e.w, e.x, e.y, e.cw, e.ch, flags};
    const TilePixels<SCH, Mem> px = {mem, base};
    crop_word<OCH>(px, g, b0, n, W);
    mem.store16(q + b0, W);
}

// f >= 2: the sums of item `item`'s share of its block - rb = S_r | S_b << 16, ga = S_g | S_a << 16 (a lane sees at most 4 x 64 pixels:
// 256 * 255 < 2^16), Wt the alpha-weighted sums (WEIGHTED only) - added to what the caller passes.  sh: thumb_share of the item over the
// rectangle; nothing is read where sh.o is behind the output or sh.n == 0.
template <uint32_t SCH, bool WEIGHTED, class Mem>
QOIMI_CROP_HD void tile_share_sums(const Mem& mem, const TileEntry& e, uint64_t base, const ThumbShare& sh, uint32_t& rb, uint32_t& ga, uint32_t (&Wt)[3]) {
    if (sh.o >= e.tw * e.th || sh.n == 0u) return;
    const uint64_t pitch = (uint64_t)e.w * SCH;
    uint64_t A = base + ((uint64_t)(e.y + sh.y0) * e.w + e.x + sh.x0) * SCH;
    const bool wide = SCH == 4u && sh.n == 4u && ((A | pitch) & 15u) == 0u;     // 16-byte aligned in every row
    for (uint32_t r = sh.y0; r < sh.y1; ++r, A += pitch) {
        uint32_t px[4] = {0u, 0u, 0u, 0u};
        if (wide) mem.load16(A, px);
        else {
            QOIMI_CROP_UNROLL
            for (uint32_t k = 0; k < 4u; ++k)
                if (k < sh.n) px[k] = tile_fetch<SCH>(mem, A + (uint64_t)k * SCH);
        }
        QOIMI_CROP_UNROLL
        for (uint32_t k = 0; k < 4u; ++k)
            if (k < sh.n) {
                rb += px[k] & 0x00FF00FFu;
                ga += (px[k] >> 8) & 0x00FF00FFu;
                if (WEIGHTED) {
                    const uint32_t a = px[k] >> 24;
                    Wt[0] += (px[k] & 255u) * a; Wt[1] += ((px[k] >> 8) & 255u) * a; Wt[2] += ((px[k] >> 16) & 255u) * a;
                }
            }
    }
}

// Where pixel o (row-major) of the reduced rectangle stands in the output.
QOIMI_CROP_HD uint32_t tile_dest(const TileEntry& e, uint32_t o) {
    const uint32_t flags = e.cfg >> 28;
    const uint32_t Y = o / e.tw, X = o - Y * e.tw;
    return ((flags & kCropFlipY) != 0u ? e.th - 1u - Y : Y) * e.tw + ((flags & kCropFlipX) != 0u ? e.tw - 1u - X : X);
}

// ---- QOIMI_TILE_NEAREST / QOIMI_TILE_MODE: label maps (the kernel tile_select) ----
//
// The definition (normative; qoi_amd/tiles.py: tile states it in Python).  The rectangle is taken at 4 bytes per pixel - a 3-byte pixel has
// alpha 255, and that alpha takes part.  The block of output pixel (X, Y) is the box filter's: columns [X * f, min((X + 1) * f, cw)), nx of
// them, rows [Y * f, min((Y + 1) * f, ch)), ny of them; its centre pixel is column X * f + nx / 2, row Y * f + ny / 2 (the divisions
// floor).  NEAREST: the output pixel is the centre pixel.  MODE: the vote of qoi_mode_core.h over the block - whole pixels vote, the largest
// count wins, of several winners the centre pixel if it is one, else the lowest r << 24 | g << 16 | b << 8 | a -, f <= kTileModeMaxFactor:
// a block is at most 16 x 16.  Flips, och and the slot as above; 4 to 3 drops alpha after the vote.
//
// The kind stands in bits 25..27 of cfg (0: the box filter above; bit 24 is its alone), and for the two kinds here bits 0..15 hold the
// vote's split, mode_split(f, f, 1, 1), in the place of thumb_split's: L = 2^lg neighbouring lanes share an output pixel, item i of the entry
// is lane i % L of output pixel i / L (row-major, unflipped) and holds the pixels p = l, l + L, l + 2L, l + 3L below nx * ny of its block,
// p being column p % nx and row p / nx.  NEAREST and f == 1 have lg = 0, c = 1.  f == 1 is tile_copy_item in both kinds.
constexpr uint32_t kTileKindBox = 0, kTileKindNearest = 1, kTileKindMode = 2;
constexpr uint32_t kTileModeMaxFactor = kModeMaxRatio;

QOIMI_CROP_HD uint32_t tile_select_cfg(uint32_t kind, uint32_t f, uint32_t sch, uint32_t och, uint32_t flags) {
    uint32_t lg = 0u, c = 1u;
    if (kind == kTileKindMode) mode_split(f, f, 1u, 1u, lg, c);
    return lg | (c << 8) | (sch << 16) | (och << 20) | (kind << 25) | (flags << 28);
}

// Items of a tile of the two kinds (f == 1: the copy's) and the tiles of kTileThreads items they take.  (cw * ch < 400 000 000 and f >= 2:
// fewer than 2^28 output pixels of at most 64 lanes; the kernel numbers items in 64 bits.)
QOIMI_CROP_HD uint64_t tile_select_items(uint32_t kind, uint32_t cw, uint32_t ch, uint32_t f, uint32_t och) {
    if (f == 1u) return tile_items(cw, ch, 1u, och);
    return ((uint64_t)thumb_extent(cw, f) * thumb_extent(ch, f)) << (tile_select_cfg(kind, f, 0u, 0u, 0u) & 255u);
}
QOIMI_CROP_HD uint64_t tile_select_tiles(uint32_t kind, uint32_t cw, uint32_t ch, uint32_t f, uint32_t och) {
    return (tile_select_items(kind, cw, ch, f, och) + kTileThreads - 1u) / kTileThreads;
}

// The block of pixel o (row-major) of the reduced rectangle: its first column and row within the rectangle and its extent.
struct TileBlock { uint32_t x0, y0, nx, ny; };
QOIMI_CROP_HD TileBlock tile_block(const TileEntry& e, uint32_t o) {
    const uint32_t Y = o / e.tw, X = o - Y * e.tw;
    const uint32_t x0 = X * e.f, y0 = Y * e.f;
    return {x0, y0, e.cw - x0 < e.f ? e.cw - x0 : e.f, e.ch - y0 < e.f ? e.ch - y0 : e.f};
}

// The pixel at column k, row r of the rectangle.
template <uint32_t SCH, class Mem>
QOIMI_CROP_HD uint32_t tile_rect_pixel(const Mem& mem, const TileEntry& e, uint64_t base, uint32_t k, uint32_t r) {
    return tile_fetch<SCH>(mem, base + ((uint64_t)(e.y + r) * e.w + e.x + k) * SCH);
}

// NEAREST: the centre pixel of the block of pixel o < tw * th.
template <uint32_t SCH, class Mem>
QOIMI_CROP_HD uint32_t tile_centre_pixel(const Mem& mem, const TileEntry& e, uint64_t base, uint32_t o) {
    const TileBlock b = tile_block(e, o);
    return tile_rect_pixel<SCH>(mem, e, base, b.x0 + b.nx / 2u, b.y0 + b.ny / 2u);
}

// MODE: what lane l of 2^lg holds of the block of pixel o < tw * th (mode_hold over the block).
template <uint32_t SCH, class Mem>
QOIMI_CROP_HD void tile_vote_hold(const Mem& mem, const TileEntry& e, uint64_t base, uint32_t o, uint32_t l, uint32_t lg, ModeHeld& h) {
    const TileBlock b = tile_block(e, o);
    const uint32_t pc = (b.ny / 2u) * b.nx + b.nx / 2u;
    mode_none(h);
    QOIMI_CROP_UNROLL
    for (uint32_t j = 0; j < kModeHold; ++j) {
        const uint32_t p = l + (j << lg);
        if (p < b.nx * b.ny) {
            const uint32_t pr = p / b.nx, pk = p - pr * b.nx;
            h.v[j] = tile_rect_pixel<SCH>(mem, e, base, b.x0 + pk, b.y0 + pr);
            h.n = j + 1u;
            if (p == pc) h.centre = j;
        }
    }
}

// The store of pixel o of the reduced rectangle into the output at the address q (4-aligned): a dword at och == 4, three bytes at och == 3.
template <class Mem>
QOIMI_CROP_HD void tile_put(const Mem& mem, const TileEntry& e, uint64_t q, uint32_t o, uint32_t px) {
    const uint32_t och = (e.cfg >> 20) & 15u;
    const uint64_t a = q + (uint64_t)tile_dest(e, o) * och;
    if (och == 4u) mem.store4(a, px);
    else { mem.store1(a, px & 255u); mem.store1(a + 1u, (px >> 8) & 255u); mem.store1(a + 2u, (px >> 16) & 255u); }
}

}  // namespace qoimi

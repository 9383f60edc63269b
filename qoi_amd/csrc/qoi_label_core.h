// qoi_label_core.h — label tensors as the source of qoimi_encode_tiles (QOIMI_TILE_LABELS): the item arithmetic of the kernel label_ingest,
// which a label call runs in tile_gather's place - which elements an item reads, how an element becomes a byte, how a byte becomes a pixel.
//
// The definition (normative; qoi_amd/tiles.py: labels_to_bytes states it in Python).  The image a tile names is ONE PLANE of w x h elements:
// u8, or little-endian two's-complement int32 / int64 (element size E = 1 / 4 / 8), tightly packed at an address that is a multiple of E;
// element (Y, X) stands at element index Y * w + X.  The byte b of the element v is 0 for v < 0, 255 for v > 255, else v: saturation of the
// full 32- / 64-bit value - the high dword of an i64 takes part, 2^32 is 255 and not 0 - and silent: nothing counts it, an ignore index of
// -100 becomes 0.  Pixel (Y, X) of the byte image B (h x w x 4) is (b, b, b, 255): the dword b * 0x010101 | 0xFF000000.  The tile then is
// the tile of B as a 4-channel byte image: qoi_tile_core.h's rectangle, flips, och (4 to 3 drops the 255) and - unlike a tensor source - its
// two label reductions, the centre pixel (QOIMI_TILE_NEAREST, f = 1..64) and the vote (QOIMI_TILE_MODE, f = 1..16).  All pixels of B are
// grey with alpha 255, so the whole-pixel vote is the vote on b: the largest count, among several winners the centre pixel if it is one,
// else the lowest b.  A label source is never averaged: the box modes take factor 1 only.
//
// 24-bit ids (QOIMI_TILE_LABELS_ID24; normative; qoi_amd/tiles.py: label_ids_to_bytes).  The same plane, dtype, alignment and extent; the id of
// the element v is 0 for v < 0, 2^24 - 1 for v > 2^24 - 1, else v - again of the full 32- / 64-bit value, 2^32 + 5 is 2^24 - 1 and not 5, and
// silent -, and pixel (Y, X) of B is (id & 255, (id >> 8) & 255, id >> 16, 255): the dword id | 0xFF000000, the COCO panoptic convention
// id = R + 256 * G + 256^2 * B.  A u8 plane gives (v, 0, 0, 255).  Everything behind B is as above; the pixels are no longer grey, so the
// vote is the whole-pixel vote as it stands: among winners without the centre pixel the lowest r << 24 | g << 16 | b << 8 | a - the order of
// the id's bytes from the low byte up, not the lowest id.  The functions below take the variant as the template parameter ID (0: bytes).
//
// f == 1: an ITEM is kIngestPixels = 4 consecutive pixels of the tile's OUTPUT in output order, stored as qoi_ingest_core.h's item stores
// them - one 16-byte store at och == 4, one 12-byte store at och == 3 (a last item of och == 3 stores only the dwords that hold one of the
// tile's bytes) -, 256 items to a tile of the walk.  Where its four pixels lie in one row the lane reads four consecutive elements: u8 the one
// or two aligned dwords that hold them; i32 one 16-byte load where the address is a multiple of 16, else four dwords; i64 two 16-byte loads
// where it is, else four 8-byte loads.  Otherwise element by element.
// f >= 2: the items of tile_select (qoi_tile_core.h: tile_select_cfg, tile_select_tiles).  NEAREST: a lane per output pixel loads the
// element at its block's centre.  MODE: L = 2^lg neighbouring lanes share an output pixel, tile_vote_hold says which pixels of the block a
// lane holds and qoi_mode_core.h votes; only the fetch is this file's: LabelImage presents B to those functions - its load4 of the byte
// address 4 * i gives pixel i of B -, so neither the block arithmetic nor the vote is stated again.
// Nothing is read but whole, naturally aligned elements of the plane - for u8 the aligned dwords that hold one of its bytes.
//
// The table entry is qoi_tile_core.h's TileEntry with kind kTileKindLabel; w, x, y, cw, ch, tw, th and f are a tile's.  cfg: label_cfg.
//
// Plain sequential code over a memory functor `Mem` (load4(aligned address) -> dword, load8 / load16(aligned address, dwords), store1 / store4 /
// store12 / store16(address, ...)), compiled for the device by hipcc (qoi_label.hip) and - by tests/host/label_host.cpp only - for the
// host, where the functor checks every address against the plane and the slot.
#pragma once
#include <stdint.h>

#include "qoi_ingest_core.h"
#include "qoi_tile_core.h"

namespace qoimi {

constexpr uint32_t kTileKindLabel = 4;

// qoimi_tile.flags: a label source and its dtype field (3 is not a dtype)
constexpr uint32_t kTileLabels = 2048, kTileLabelsDtypeShift = 12;
constexpr uint32_t kTileLabelsMask = kTileLabels | (3u << kTileLabelsDtypeShift);
constexpr uint32_t kLabelU8 = 0, kLabelI32 = 1, kLabelI64 = 2;
// ... and the 24-bit id variant: bit 15 of the flags, 4 in the dtype field of an entry's cfg (4 / 5 / 6)
constexpr uint32_t kTileLabelsId24 = 32768, kLabelId24 = 4, kLabelIdMax = 0xFFFFFFu;

QOIMI_CROP_HD uint32_t label_dtype(uint32_t flags) { return (flags >> kTileLabelsDtypeShift) & 3u; }
QOIMI_CROP_HD uint32_t label_elem(uint32_t dtype) { return dtype == kLabelU8 ? 1u : dtype == kLabelI32 ? 4u : 8u; }

// cfg of a label entry: the vote's split in bits 0..15 as tile_select_cfg gives it (lg = 0, c = 1 without a vote) | dtype << 16 (the
// place of sch: B has four channels, whatever the plane is made of; kLabelId24 is added for 24-bit ids) | och << 20 | (vote ? 1 : 0) << 24 | kTileKindLabel << 25 | flips << 28
QOIMI_CROP_HD uint32_t label_cfg(uint32_t flags, uint32_t f, bool vote, uint32_t och) {
    const uint32_t split = tile_select_cfg(vote && f != 1u ? kTileKindMode : kTileKindNearest, f, 0u, 0u, 0u) & 0xFFFFu;
    return split | ((label_dtype(flags) | ((flags & kTileLabelsId24) != 0u ? kLabelId24 : 0u)) << 16) | (och << 20) | ((vote && f != 1u ? 1u : 0u) << 24) | (kTileKindLabel << 25) |
           ((flags & (kCropFlipX | kCropFlipY)) << 28);
}

// Tiles of kTileThreads items of a label tile: f == 1 four output pixels an item, else tile_select's items.
QOIMI_CROP_HD uint64_t label_tiles(uint32_t cw, uint32_t ch, uint32_t f, bool vote, uint32_t och) {
    return f == 1u ? ingest_tiles(cw, ch) : tile_select_tiles(vote ? kTileKindMode : kTileKindNearest, cw, ch, f, och);
}

// The byte of an int32 element with the bits v, and of an int64 element with the bits hi : lo - the high dword decides, then the low.
QOIMI_CROP_HD uint32_t label_sat32(uint32_t v) {
    const int32_t s = (int32_t)v;
    return s < 0 ? 0u : s > 255 ? 255u : (uint32_t)s;
}
QOIMI_CROP_HD uint32_t label_sat64(uint32_t lo, uint32_t hi) {
    const int32_t h = (int32_t)hi;
    return h < 0 ? 0u : h > 0 ? 255u : lo > 255u ? 255u : lo;
}

// ... and their 24-bit ids: 0 below 0, 2^24 - 1 above it.
QOIMI_CROP_HD uint32_t label_id32(uint32_t v) {
    const int32_t s = (int32_t)v;
    return s < 0 ? 0u : v > kLabelIdMax ? kLabelIdMax : v;
}
QOIMI_CROP_HD uint32_t label_id64(uint32_t lo, uint32_t hi) {
    const int32_t h = (int32_t)hi;
    return h < 0 ? 0u : h > 0 ? kLabelIdMax : lo > kLabelIdMax ? kLabelIdMax : lo;
}

// The pixel (b, b, b, 255) as r | g << 8 | b << 16 | a << 24.
QOIMI_CROP_HD uint32_t label_pixel(uint32_t b) { return b * 0x010101u | 0xFF000000u; }
// The pixel (id & 255, (id >> 8) & 255, id >> 16, 255) of an id below 2^24.
QOIMI_CROP_HD uint32_t label_id_pixel(uint32_t id) { return id | 0xFF000000u; }

// What an element becomes - its byte (ID == 0) or its id - and the pixel of that.
template <uint32_t ID> QOIMI_CROP_HD uint32_t label_value32(uint32_t v) { return ID != 0u ? label_id32(v) : label_sat32(v); }
template <uint32_t ID> QOIMI_CROP_HD uint32_t label_value64(uint32_t lo, uint32_t hi) { return ID != 0u ? label_id64(lo, hi) : label_sat64(lo, hi); }
template <uint32_t ID> QOIMI_CROP_HD uint32_t label_value_pixel(uint32_t b) { return ID != 0u ? label_id_pixel(b) : label_pixel(b); }

// The byte (the id) of the one element at the address a (a multiple of E).
template <uint32_t DT, uint32_t ID = 0u, class Mem>
QOIMI_CROP_HD uint32_t label_load(const Mem& mem, uint64_t a) {
    if (DT == kLabelU8) return (mem.load4(a & ~(uint64_t)3u) >> (8u * ((uint32_t)a & 3u))) & 255u;      // (out of the aligned dword that holds it)
    if (DT == kLabelI32) return label_value32<ID>(mem.load4(a));
    uint32_t w[2];
    mem.load8(a, w);
    return label_value64<ID>(w[0], w[1]);
}

// The bytes (the ids) of four consecutive elements from the address a (a multiple of E).
template <uint32_t DT, uint32_t ID = 0u, class Mem>
QOIMI_CROP_HD void label_load_run(const Mem& mem, uint64_t a, uint32_t (&b)[4]) {
    if (DT == kLabelU8) {
        const uint32_t s = (uint32_t)a & 3u;
        const uint32_t lo = mem.load4(a - s), hi = s != 0u ? mem.load4(a - s + 4u) : 0u;
        const uint32_t w = crop_align(hi, lo, s);
        b[0] = w & 255u; b[1] = (w >> 8) & 255u; b[2] = (w >> 16) & 255u; b[3] = w >> 24;
    } else if (DT == kLabelI32) {
        uint32_t v[4];
        if ((a & 15u) == 0u) mem.load16(a, v);
        else { v[0] = mem.load4(a); v[1] = mem.load4(a + 4u); v[2] = mem.load4(a + 8u); v[3] = mem.load4(a + 12u); }
        QOIMI_CROP_UNROLL
        for (uint32_t j = 0; j < 4u; ++j) b[j] = label_value32<ID>(v[j]);
    } else {
        if ((a & 15u) == 0u) {
            uint32_t v[4], u[4];
            mem.load16(a, v); mem.load16(a + 16u, u);
            b[0] = label_value64<ID>(v[0], v[1]); b[1] = label_value64<ID>(v[2], v[3]); b[2] = label_value64<ID>(u[0], u[1]); b[3] = label_value64<ID>(u[2], u[3]);
        } else {
            QOIMI_CROP_UNROLL
            for (uint32_t j = 0; j < 4u; ++j) { uint32_t w[2]; mem.load8(a + 8u * j, w); b[j] = label_value64<ID>(w[0], w[1]); }
        }
    }
}

// f == 1: item k < ingest_items of the entry e, whose plane begins at the address `base` and whose output begins at the 256-aligned address q.
template <uint32_t DT, uint32_t ID = 0u, class Mem>
QOIMI_CROP_HD void label_item(const Mem& mem, const TileEntry& e, uint64_t base, uint64_t q, uint32_t k) {
    constexpr uint32_t E = DT == kLabelU8 ? 1u : DT == kLabelI32 ? 4u : 8u;
    const uint32_t och = (e.cfg >> 20) & 15u, flags = e.cfg >> 28;
    const bool fx = (flags & kCropFlipX) != 0u, fy = (flags & kCropFlipY) != 0u;
    const uint32_t P = e.cw * e.ch, p0 = kIngestPixels * k;                      // (an image holds fewer than 400 000 000 pixels)
    const uint32_t n = P - p0 < kIngestPixels ? P - p0 : kIngestPixels;
    uint32_t r = p0 / e.cw, c = p0 - r * e.cw;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    if (n == kIngestPixels && c + kIngestPixels <= e.cw) {                       // four pixels of one row: a run of four elements
        const uint64_t row = fy ? e.y + e.ch - 1u - r : e.y + r, col = fx ? e.x + e.cw - kIngestPixels - c : e.x + c;     // the lowest of the four
        uint32_t b[4];
        label_load_run<DT, ID>(mem, base + (row * e.w + col) * E, b);
        QOIMI_CROP_UNROLL
        for (uint32_t j = 0; j < 4u; ++j) px[j] = label_value_pixel<ID>(b[fx ? 3u - j : j]);
    } else {
        QOIMI_CROP_UNROLL
        for (uint32_t j = 0; j < 4u; ++j) {
            if (j < n) {
                const uint64_t row = fy ? e.y + e.ch - 1u - r : e.y + r, col = fx ? e.x + e.cw - 1u - c : e.x + c;
                px[j] = label_value_pixel<ID>(label_load<DT, ID>(mem, base + (row * e.w + col) * E));
                if (++c == e.cw) { c = 0u; ++r; }
            }
        }
    }
    if (och == 4u) { mem.store16(q + 16u * (uint64_t)k, px); return; }
    uint32_t W[3];                                                               // (three bytes a pixel, the 255 dropped; with ids r, g and b differ)
    const uint32_t a0 = px[0] & 0xFFFFFFu, a1 = px[1] & 0xFFFFFFu, a2 = px[2] & 0xFFFFFFu, a3 = px[3] & 0xFFFFFFu;
    W[0] = a0 | (a1 << 24); W[1] = (a1 >> 8) | (a2 << 16); W[2] = (a2 >> 16) | (a3 << 8);
    const uint64_t a = q + 12u * (uint64_t)k;
    if (n == kIngestPixels) { mem.store12(a, W); return; }
    const uint32_t nd = (3u * n + 3u) >> 2;                                      // the dwords that hold one of the tile's bytes
    QOIMI_CROP_UNROLL
    for (uint32_t d = 0; d < 3u; ++d)
        if (d < nd) mem.store4(a + 4u * d, W[d]);
}

// B as the memory qoi_tile_core.h's label reductions read: the dword at the byte address 4 * i is pixel i of B (tile_fetch<4> of an aligned
// address is one load4), fetched as one element of the plane at `base`.  The stores are the slot's.
template <uint32_t DT, class Mem, uint32_t ID = 0u>
struct LabelImage {
    const Mem& mem; uint64_t base;
    QOIMI_CROP_HD uint32_t load4(uint64_t A) const { return label_value_pixel<ID>(label_load<DT, ID>(mem, base + (A >> 2) * (DT == kLabelU8 ? 1u : DT == kLabelI32 ? 4u : 8u))); }
    QOIMI_CROP_HD void store1(uint64_t a, uint32_t v) const { mem.store1(a, v); }
    QOIMI_CROP_HD void store4(uint64_t a, uint32_t v) const { mem.store4(a, v); }
};

// f >= 2, NEAREST: output pixel o < tw * th of the entry - one element load, at the block's centre - stored where the flips put it.
template <uint32_t DT, uint32_t ID = 0u, class Mem>
QOIMI_CROP_HD void label_nearest_item(const Mem& mem, const TileEntry& e, uint64_t base, uint64_t q, uint32_t o) {
    const LabelImage<DT, Mem, ID> B = {mem, base};
    tile_put(B, e, q, o, tile_centre_pixel<4u>(B, e, 0u, o));
}

// f >= 2, MODE: what lane l of 2^lg holds of the block of output pixel o < tw * th (tile_vote_hold over B).
template <uint32_t DT, uint32_t ID = 0u, class Mem>
QOIMI_CROP_HD void label_vote_hold(const Mem& mem, const TileEntry& e, uint64_t base, uint32_t o, uint32_t l, uint32_t lg, ModeHeld& h) {
    const LabelImage<DT, Mem, ID> B = {mem, base};
    tile_vote_hold<4u>(B, e, 0u, o, l, lg, h);
}

}  // namespace qoimi

// tile_select_host.cpp — the item loop of qoimi_encode_tiles in QOIMI_TILE_NEAREST and QOIMI_TILE_MODE (qoi_amd/csrc/qoi_tile_core.h:
// tile_select_cfg, tile_select_tiles, tile_copy_item, tile_centre_pixel, tile_vote_hold, tile_put; the vote: qoi_mode_core.h) compiled for
// the host: the walk of tile_select over one table entry, tile by tile, with the 256 lanes of a tile walked in a loop - where the kernel
// moves pixels between lanes (__shfl of width L, __shfl_xor) this file reads the other lane's entry of an array of 256.  The image stands
// in real memory at any byte offset and every load is checked against its aligned dwords; the slot is the virtual array of host_mem.h
// (StoreMem), so every store is checked and counted.  tests/test_tile_select_core_host.py compares it with the Python model without a GPU.
// With -DTILE_SELECT_HOST_MAIN the same source is a stand-alone program that walks a grid of tiles against a plain counting loop (the test
// builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include <string.h>

#include "../../qoi_amd/csrc/qoi_tile_core.h"
#include "host_mem.h"

namespace {

// The kernel's memory: a 4-byte load must be aligned and hold at least one byte of the image, a 16-byte load must be aligned and lie
// inside the image; the stores are StoreMem's.
struct SelectMem : hostmem::StoreMem {
    uint64_t img_lo, img_hi;
    long long* loads;
    uint32_t load4(uint64_t a) const {
        ++*loads;
        if ((a & 3u) != 0u || a + 4u <= img_lo || a >= img_hi) { ++*bad; return 0u; }
        uint32_t v; memcpy(&v, (const void*)(uintptr_t)a, 4); return v;
    }
    void load16(uint64_t a, uint32_t (&W)[4]) const {
        ++*loads;
        if ((a & 15u) != 0u || a < img_lo || a + 16u > img_hi) { ++*bad; W[0] = W[1] = W[2] = W[3] = 0u; return; }
        memcpy(W, (const void*)(uintptr_t)a, 16);
    }
};

template <uint32_t SCH, uint32_t OCH>
void copy_tile(const SelectMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tile) {
    for (uint32_t t = 0; t < qoimi::kTileThreads; ++t) {
        const uint64_t k = tile * qoimi::kTileThreads + t;
        if (k < qoimi::tile_items(e.cw, e.ch, 1u, OCH)) qoimi::tile_copy_item<SCH, OCH>(mem, e, base, q, (uint32_t)k);
    }
}

template <uint32_t SCH>
void nearest_tile(const SelectMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tile) {
    for (uint32_t t = 0; t < qoimi::kTileThreads; ++t) {
        const uint64_t o = tile * qoimi::kTileThreads + t;
        if (o < (uint64_t)e.tw * e.th) qoimi::tile_put(mem, e, q, (uint32_t)o, qoimi::tile_centre_pixel<SCH>(mem, e, base, (uint32_t)o));
    }
}

// One tile as the kernel runs it: every one of the 256 lanes takes every step, whether its output pixel exists or not.
template <uint32_t SCH>
void vote_tile(const SelectMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tile) {
    using namespace qoimi;
    const uint32_t lg = e.cfg & 255u, L = 1u << lg;
    ModeHeld h[kTileThreads];
    uint32_t count[kTileThreads][kModeHold];
    uint64_t best[kTileThreads], next[kTileThreads], o[kTileThreads];
    bool valid[kTileThreads];
    for (uint32_t t = 0; t < kTileThreads; ++t) {
        const uint64_t item = tile * kTileThreads + t;
        o[t] = item >> lg;
        valid[t] = o[t] < (uint64_t)e.tw * e.th;
        if (valid[t]) tile_vote_hold<SCH>(mem, e, base, (uint32_t)o[t], (uint32_t)item & (L - 1u), lg, h[t]);
        else mode_none(h[t]);
        for (uint32_t j = 0; j < kModeHold; ++j) count[t][j] = 0u;
    }
    for (uint32_t s = 0; s < L; ++s)                                  // (s = 0: the lane's own pixels)
        for (uint32_t t = 0; t < kTileThreads; ++t) {
            const uint32_t other = (t & ~(L - 1u)) | ((t + s) & (L - 1u));   // __shfl(., l + s, L)
            mode_meet(h[t], h[other].v, h[other].n, count[t]);
        }
    for (uint32_t t = 0; t < kTileThreads; ++t) best[t] = mode_best(h[t], count[t]);
    for (uint32_t step = 1u; step < L; step <<= 1) {                  // __shfl_xor(., step)
        for (uint32_t t = 0; t < kTileThreads; ++t) next[t] = best[t ^ step] > best[t] ? best[t ^ step] : best[t];
        for (uint32_t t = 0; t < kTileThreads; ++t) best[t] = next[t];
    }
    for (uint32_t t = 0; t < kTileThreads; ++t)
        if (valid[t] && (t & (L - 1u)) == 0u) tile_put(mem, e, q, (uint32_t)o[t], mode_pick(best[t]));
}

}  // namespace

extern "C" {

// One table entry as tile_select walks it.  img: the image's first byte (rows of w pixels of sch bytes; 16 readable bytes in front of it
// and behind it); kind: 1 NEAREST, 2 MODE; the slot begins at out[q - base], q a multiple of 16; writes[i] counts the stores to out[i].
// Returns the tiles walked, or -1 - the number of bad accesses if there was one.
long long tile_select_host_run(const uint8_t* img, uint32_t w, uint32_t h, uint32_t sch, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t f,
                               uint32_t flags, uint32_t och, uint32_t kind, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len) {
    long long bad = 0, loads = 0;
    qoimi::TileEntry e;
    memset(&e, 0, sizeof e);
    e.w = w; e.x = x; e.y = y; e.cw = cw; e.ch = ch; e.f = f;
    e.tw = qoimi::thumb_extent(cw, f); e.th = qoimi::thumb_extent(ch, f);
    e.cfg = qoimi::tile_select_cfg(kind, f, sch, och, flags);
    const uint64_t at = (uint64_t)(uintptr_t)img;
    SelectMem mem = {{out, writes, out_len, base, &bad, nullptr}, at, at + (uint64_t)w * h * sch, &loads};
    const uint64_t tiles = qoimi::tile_select_tiles(kind, cw, ch, f, och);
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        if (f == 1u) {
            if (sch == 4u) { if (och == 4u) copy_tile<4u, 4u>(mem, e, at, q, tile); else copy_tile<4u, 3u>(mem, e, at, q, tile); }
            else { if (och == 4u) copy_tile<3u, 4u>(mem, e, at, q, tile); else copy_tile<3u, 3u>(mem, e, at, q, tile); }
        } else if (kind == qoimi::kTileKindNearest) {
            if (sch == 4u) nearest_tile<4u>(mem, e, at, q, tile); else nearest_tile<3u>(mem, e, at, q, tile);
        } else {
            if (sch == 4u) vote_tile<4u>(mem, e, at, q, tile); else vote_tile<3u>(mem, e, at, q, tile);
        }
    }
    return hostmem::checked(bad, (long long)tiles);
}

uint64_t tile_select_host_tiles(uint32_t kind, uint32_t cw, uint32_t ch, uint32_t f, uint32_t och) { return qoimi::tile_select_tiles(kind, cw, ch, f, och); }
uint32_t tile_select_host_cfg(uint32_t kind, uint32_t f, uint32_t sch, uint32_t och, uint32_t flags) { return qoimi::tile_select_cfg(kind, f, sch, och, flags); }
uint32_t tile_select_host_max_factor() { return qoimi::kTileModeMaxFactor; }

}

#ifdef TILE_SELECT_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

// Pixel (k, r) of the rectangle as r | g << 8 | b << 16 | a << 24, alpha 255 behind 3 bytes
static uint32_t pixel(const uint8_t* img, uint32_t w, uint32_t sch, uint32_t x, uint32_t y, uint32_t k, uint32_t r) {
    const uint8_t* p = img + ((size_t)(y + r) * w + x + k) * sch;
    return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (sch == 4u ? (uint32_t)p[3] : 255u) << 24;
}

// The definition as a plain counting loop (qoi_amd/tiles.py: select)
static uint32_t plain_pixel(const uint8_t* img, uint32_t w, uint32_t sch, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t f, uint32_t kind, uint32_t X, uint32_t Y) {
    const uint32_t nx = cw - X * f < f ? cw - X * f : f, ny = ch - Y * f < f ? ch - Y * f : f;
    const uint32_t centre = pixel(img, w, sch, x, y, X * f + nx / 2u, Y * f + ny / 2u);
    if (kind == 1u) return centre;
    std::vector<uint32_t> px;
    for (uint32_t r = 0; r < ny; ++r) for (uint32_t k = 0; k < nx; ++k) px.push_back(pixel(img, w, sch, x, y, X * f + k, Y * f + r));
    size_t top = 0;
    for (uint32_t a : px) { size_t n = 0; for (uint32_t b : px) n += a == b; if (n > top) top = n; }
    bool have = false, centre_wins = false; uint32_t low = 0; uint64_t low_key = 0;
    for (uint32_t a : px) {
        size_t n = 0; for (uint32_t b : px) n += a == b;
        if (n != top) continue;
        const uint64_t key = ((uint64_t)(a & 255u) << 24) | ((a >> 8 & 255u) << 16) | ((a >> 16 & 255u) << 8) | (a >> 24);
        if (a == centre) centre_wins = true;
        if (!have || key < low_key) { have = true; low = a; low_key = key; }
    }
    return centre_wins ? centre : low;
}

// Label maps of 2 to 5 classes - two of them differ in alpha alone at 4 bytes - so that votes, ties and lowest keys all happen; the image
// at every byte offset 0..3 from a 16-aligned address; rectangles at odd corners; both kinds, every factor with its own split, both och,
// all four flips.  The slot stands between two guard bands.
int main() {
    struct Src { uint32_t w, h, sch, off; };
    const Src srcs[] = {{1, 1, 3, 0}, {1, 1, 4, 2}, {1, 130, 3, 2}, {1, 130, 4, 1}, {37, 29, 3, 1}, {37, 29, 3, 3}, {70, 45, 4, 3}, {70, 45, 4, 2}, {64, 40, 4, 0}};
    const uint32_t factors[] = {1, 2, 3, 4, 5, 8, 13, 16, 33, 64};
    const uint32_t palette[5] = {0xFF000000u, 0xFF030201u, 0x80030201u, 0xFF000007u, 0x00FFFFFFu};
    const uint64_t base = 4096, guard = 48;
    uint32_t seed = 12345u;
    long long runs = 0;
    for (const Src& s : srcs) {
        const size_t bytes = (size_t)s.w * s.h * s.sch;
        uint8_t* raw = (uint8_t*)aligned_alloc(16, (bytes + 64u + 15u) & ~(size_t)15u);
        uint8_t* img = raw + 16 + s.off;
        const uint32_t classes = 2u + (s.w + s.h + s.off) % 4u;
        for (size_t i = 0; i < bytes + 48u; ++i) raw[i] = 0x5Au;
        for (size_t p = 0; p < (size_t)s.w * s.h; ++p) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t c = palette[(seed >> 24) % classes];
            for (uint32_t k = 0; k < s.sch; ++k) img[p * s.sch + k] = (uint8_t)(c >> (8u * k));
        }
        const uint32_t rects[][4] = {{0, 0, s.w, s.h}, {s.w > 8 ? 3u : 0u, s.h > 12 ? 5u : 0u, s.w > 8 ? s.w - 7 : s.w, s.h > 12 ? s.h - 9 : s.h},
                                     {s.w > 8 ? 4u : 0u, s.h > 12 ? 8u : 0u, s.w > 8 ? s.w - 4 : s.w, s.h > 12 ? s.h - 8 : s.h}};
        for (const auto& r : rects)
            for (uint32_t kind = 1; kind <= 2; ++kind)
                for (uint32_t f : factors)
                    for (uint32_t flags = 0; flags < 4; ++flags)
                        for (uint32_t och = 3; och <= 4; ++och) {
                            if (kind == 2u && f > tile_select_host_max_factor()) continue;
                            const uint32_t tw = (r[2] + f - 1) / f, th = (r[3] + f - 1) / f;
                            const size_t B = (size_t)tw * th * och, slot = (B + 255u) & ~(size_t)255u, stored = f == 1u ? (B + 15u) & ~(size_t)15u : B;
                            std::vector<uint8_t> out(guard + slot + guard, hostmem::kGuard), writes(out.size(), 0);
                            const long long rc = tile_select_host_run(img, s.w, s.h, s.sch, r[0], r[1], r[2], r[3], f, flags, och, kind, base + guard, base, out.data(),
                                                                      writes.data(), guard + slot);        // (a store behind the slot is a bad access)
                            if (rc < 0) { printf("%lld bad accesses: %ux%ux%u+%u rect %u,%u %ux%u kind %u f %u flags %u och %u\n", -1 - rc, s.w, s.h, s.sch, s.off, r[0], r[1], r[2], r[3], kind, f, flags, och); return 1; }
                            const long long off = hostmem::first_miswritten(out, writes, guard, stored);      // (f == 1 stores whole 16-byte words)
                            if (off >= 0) { printf("byte %lld written %u times: kind %u f %u och %u\n", off, writes[off], kind, f, och); return 1; }
                            for (uint32_t Y = 0; Y < th; ++Y)
                                for (uint32_t X = 0; X < tw; ++X) {
                                    const uint32_t px = plain_pixel(img, s.w, s.sch, r[0], r[1], r[2], r[3], f, kind, X, Y);
                                    const uint32_t dx = (flags & 1u) ? tw - 1 - X : X, dy = (flags & 2u) ? th - 1 - Y : Y;
                                    for (uint32_t c = 0; c < och; ++c)
                                        if (out[guard + ((size_t)dy * tw + dx) * och + c] != ((px >> (8u * c)) & 255u)) {
                                            printf("wrong byte: %ux%ux%u+%u rect %u,%u %ux%u kind %u f %u flags %u och %u at (%u, %u).%u\n", s.w, s.h, s.sch, s.off, r[0], r[1], r[2], r[3], kind, f,
                                                   flags, och, X, Y, c);
                                            return 1;
                                        }
                                }
                            ++runs;
                        }
        free(raw);
    }
    printf("tile_select_host: %lld tiles ok\n", runs);
    return 0;
}
#endif

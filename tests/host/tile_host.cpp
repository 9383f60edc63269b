// tile_host.cpp — the item arithmetic of qoimi_encode_tiles (qoi_amd/csrc/qoi_tile_core.h) compiled for the host, so that
// tests/test_tile_core_host.py can compare every item of every tile with the Python model without a GPU.  Not part of the library.
// With -DTILE_HOST_MAIN it is a stand-alone program (built with -fsanitize=address,undefined by the same test and run directly): the same
// cases against a plain double loop in this file.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../qoi_amd/csrc/qoi_tile_core.h"

namespace {

// The kernel's memory with every address checked: a 4-byte load must be aligned and hold at least one byte of the image, a 16-byte load
// must be aligned and lie inside the image, a store must be an aligned word of the slot.
struct HostMem {
    uint64_t img_lo, img_hi, out_lo, out_hi;
    mutable int bad = 0;
    uint32_t load4(uint64_t a) const {
        if ((a & 3u) != 0u || a + 4u <= img_lo || a >= img_hi) { bad |= 1; return 0u; }
        uint32_t v; memcpy(&v, (const void*)(uintptr_t)a, 4); return v;
    }
    void load16(uint64_t a, uint32_t (&W)[4]) const {
        if ((a & 15u) != 0u || a < img_lo || a + 16u > img_hi) { bad |= 2; W[0] = W[1] = W[2] = W[3] = 0u; return; }
        memcpy(W, (const void*)(uintptr_t)a, 16);
    }
    void store16(uint64_t a, const uint32_t (&W)[4]) const {
        if ((a & 15u) != 0u || a < out_lo || a + 16u > out_hi) { bad |= 4; return; }
        memcpy((void*)(uintptr_t)a, W, 16);
    }
};

template <uint32_t SCH, bool WEIGHTED>
void reduce_item(const HostMem& mem, const qoimi::TileEntry& e, uint64_t base, uint32_t item, std::vector<uint32_t>& acc, std::vector<uint32_t>& cnt) {
    const uint32_t lg = e.cfg & 255u, c = (e.cfg >> 8) & 255u;
    const qoimi::ThumbShare sh = qoimi::thumb_share(item, e.cw, e.ch, e.tw, e.th, e.f, lg, c);
    if (sh.o >= e.tw * e.th) return;
    uint32_t rb = 0, ga = 0, W[3] = {0, 0, 0};
    qoimi::tile_share_sums<SCH, WEIGHTED>(mem, e, base, sh, rb, ga, W);
    uint32_t* a = &acc[(size_t)sh.o * 7u];
    a[0] += rb & 0xFFFFu; a[1] += ga & 0xFFFFu; a[2] += rb >> 16; a[3] += ga >> 16;      // (the butterfly of the block's lanes)
    for (int k = 0; k < 3; ++k) a[4 + k] += W[k];
    if ((item & ((1u << lg) - 1u)) == 0u) cnt[sh.o] = sh.cnt;
}

}  // namespace

extern "C" {

// One tile, item by item and tile by tile as tile_gather numbers them.  img: the image's first byte (w pixels of sch bytes per row; 16
// readable bytes in front of it and behind it); out: 16-aligned, (tw * th * och rounded up to 256) bytes.  Returns the tiles walked, or
// -(bits) where an address was wrong (1: a dword load, 2: a 16-byte load, 4: a store).
long long tile_host_run(const uint8_t* img, uint32_t w, uint32_t h, uint32_t sch, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t f,
                        uint32_t flags, uint32_t och, int weighted, uint8_t* out) {
    qoimi::TileEntry e;
    memset(&e, 0, sizeof e);
    e.w = w; e.x = x; e.y = y; e.cw = cw; e.ch = ch; e.f = f;
    e.tw = qoimi::thumb_extent(cw, f); e.th = qoimi::thumb_extent(ch, f);
    e.cfg = qoimi::tile_cfg(f, sch, och, weighted != 0 && sch == 4u, flags);
    const uint64_t base = (uint64_t)(uintptr_t)img, q = (uint64_t)(uintptr_t)out;
    const size_t slot = ((size_t)e.tw * e.th * och + 255u) & ~(size_t)255u;
    HostMem mem = {base, base + (uint64_t)w * h * sch, q, q + slot};
    const uint64_t items = qoimi::tile_items(cw, ch, f, och), tiles = qoimi::tile_tiles(cw, ch, f, och);
    std::vector<uint32_t> acc((size_t)e.tw * e.th * 7u, 0u), cnt((size_t)e.tw * e.th, 0u);
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint32_t lane = 0; lane < qoimi::kTileThreads; ++lane) {
            const uint64_t k = t * qoimi::kTileThreads + lane;
            if (f == 1u) {
                if (k >= items) continue;
                if (sch == 4u) { if (och == 4u) qoimi::tile_copy_item<4u, 4u>(mem, e, base, q, (uint32_t)k); else qoimi::tile_copy_item<4u, 3u>(mem, e, base, q, (uint32_t)k); }
                else { if (och == 4u) qoimi::tile_copy_item<3u, 4u>(mem, e, base, q, (uint32_t)k); else qoimi::tile_copy_item<3u, 3u>(mem, e, base, q, (uint32_t)k); }
            } else {
                if (sch == 3u) reduce_item<3u, false>(mem, e, base, (uint32_t)k, acc, cnt);
                else if (e.cfg & (1u << 24)) reduce_item<4u, true>(mem, e, base, (uint32_t)k, acc, cnt);
                else reduce_item<4u, false>(mem, e, base, (uint32_t)k, acc, cnt);
            }
        }
    if (f != 1u)
        for (uint32_t o = 0; o < e.tw * e.th; ++o) {
            const uint32_t px = qoimi::thumb_pixel(&acc[(size_t)o * 7u], &acc[(size_t)o * 7u + 4u], cnt[o], (e.cfg & (1u << 24)) != 0u);
            uint8_t* p = out + (size_t)qoimi::tile_dest(e, o) * och;
            p[0] = (uint8_t)px; p[1] = (uint8_t)(px >> 8); p[2] = (uint8_t)(px >> 16);
            if (och == 4u) p[3] = (uint8_t)(px >> 24);
        }
    return mem.bad ? -(long long)mem.bad : (long long)tiles;
}

uint64_t tile_host_tiles(uint32_t cw, uint32_t ch, uint32_t f, uint32_t och) { return qoimi::tile_tiles(cw, ch, f, och); }

}

#ifdef TILE_HOST_MAIN
// The definition as a double loop (qoi_amd/tiles.py: tile), 64-bit sums.
static void model(const uint8_t* img, uint32_t w, uint32_t sch, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t f, uint32_t flags,
                  uint32_t och, bool weighted, std::vector<uint8_t>& out) {
    const uint32_t tw = (cw + f - 1) / f, th = (ch + f - 1) / f;
    out.assign((size_t)tw * th * och, 0);
    for (uint32_t Y = 0; Y < th; ++Y)
        for (uint32_t X = 0; X < tw; ++X) {
            uint64_t S[4] = {0, 0, 0, 0}, Wt[3] = {0, 0, 0}, cnt = 0;
            for (uint32_t yy = Y * f; yy < Y * f + f && yy < ch; ++yy)
                for (uint32_t xx = X * f; xx < X * f + f && xx < cw; ++xx) {
                    const uint8_t* p = img + ((size_t)(y + yy) * w + x + xx) * sch;
                    const uint64_t a = sch == 4u ? p[3] : 255u;
                    for (int k = 0; k < 3; ++k) { S[k] += p[k]; Wt[k] += p[k] * a; }
                    S[3] += a; ++cnt;
                }
            uint8_t px[4];
            for (int k = 0; k < 4; ++k) px[k] = (uint8_t)((S[k] + cnt / 2) / cnt);
            if (weighted && sch == 4u && S[3] > 0) for (int k = 0; k < 3; ++k) px[k] = (uint8_t)((Wt[k] + S[3] / 2) / S[3]);
            const uint32_t dx = (flags & 1u) ? tw - 1 - X : X, dy = (flags & 2u) ? th - 1 - Y : Y;
            memcpy(&out[((size_t)dy * tw + dx) * och], px, och);
        }
}

int main() {
    struct Src { uint32_t w, h, sch, off; };
    const Src srcs[] = {{1, 1, 3, 0}, {1, 1, 4, 2}, {1, 130, 3, 2}, {1, 130, 4, 0}, {37, 29, 3, 1}, {70, 45, 4, 3}, {64, 40, 4, 0}};
    const uint32_t factors[] = {1, 2, 3, 4, 5, 8, 13, 16, 33, 64};
    uint32_t seed = 12345u;
    long long runs = 0;
    for (const Src& s : srcs) {
        const size_t bytes = (size_t)s.w * s.h * s.sch;
        uint8_t* raw = (uint8_t*)aligned_alloc(16, (bytes + 64u + 15u) & ~(size_t)15u);
        uint8_t* img = raw + 16 + s.off;
        for (size_t i = 0; i < bytes + 48u; ++i) { seed = seed * 1664525u + 1013904223u; raw[i] = (uint8_t)(seed >> 24); }
        for (size_t i = 0; i < bytes; i += 7) if (s.sch == 4u && (i & 3u) == 3u) img[i] = (i & 8u) ? 0 : 255;
        const uint32_t rects[][4] = {{0, 0, s.w, s.h}, {s.w > 8 ? 3u : 0u, s.h > 12 ? 5u : 0u, s.w > 8 ? s.w - 7 : s.w, s.h > 12 ? s.h - 9 : s.h},
                                     {s.w > 8 ? 4u : 0u, s.h > 12 ? 8u : 0u, s.w > 8 ? s.w - 4 : s.w, s.h > 12 ? s.h - 8 : s.h}};
        for (const auto& r : rects)
            for (uint32_t f : factors)
                for (uint32_t flags = 0; flags < 4; ++flags)
                    for (uint32_t och = 3; och <= 4; ++och)
                        for (int weighted = 0; weighted < 2; ++weighted) {
                            const uint32_t tw = (r[2] + f - 1) / f, th = (r[3] + f - 1) / f;
                            const size_t slot = ((size_t)tw * th * och + 255u) & ~(size_t)255u;
                            uint8_t* out = (uint8_t*)aligned_alloc(256, slot);
                            memset(out, 0xEE, slot);
                            const long long rc = tile_host_run(img, s.w, s.h, s.sch, r[0], r[1], r[2], r[3], f, flags, och, weighted, out);
                            std::vector<uint8_t> want;
                            model(img, s.w, s.sch, r[0], r[1], r[2], r[3], f, flags, och, weighted != 0, want);
                            if (rc < 0 || memcmp(out, want.data(), want.size()) != 0) {
                                fprintf(stderr, "FAIL %ux%ux%u+%u rect %u,%u %ux%u f %u flags %u och %u weighted %d rc %lld\n", s.w, s.h, s.sch, s.off, r[0], r[1], r[2], r[3],
                                        f, flags, och, weighted, rc);
                                return 1;
                            }
                            free(out);
                            ++runs;
                        }
        free(raw);
    }
    printf("tile_host: %lld tiles ok\n", runs);
    return 0;
}
#endif

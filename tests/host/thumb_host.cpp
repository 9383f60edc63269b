// thumb_host.cpp — the block arithmetic of qoimi_decode_thumbnails (qoi_amd/csrc/qoi_thumb_core.h) compiled for the host, so that
// tests/test_thumb_core_host.py can compare it with the Python model without a GPU.  Not part of the library.
#include <stddef.h>
#include <stdint.h>

#include "../../qoi_amd/csrc/qoi_thumb_core.h"

extern "C" {

// n blocks: sums[i * 7 + 0..3] = S_r, S_g, S_b, S_a, sums[i * 7 + 4..6] = the alpha-weighted sums of r, g, b; cnt[i] pixels; out[i] = r | g << 8 | b << 16 | a << 24
void thumb_host_pixels(const uint32_t* sums, const uint32_t* cnt, size_t n, int weighted, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = qoimi::thumb_pixel(sums + i * 7, sums + i * 7 + 4, cnt[i], weighted != 0);
}

void thumb_host_div_round(const uint32_t* s, const uint32_t* d, size_t n, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = qoimi::thumb_div_round(s[i], d[i]);
}

// The items of a w x h image at factor f, tile by tile as thumb_reduce numbers them: reads[y * w + x] counts the lanes that read source pixel
// (x, y), share[o] adds up the pixels the lanes of output pixel o read, cnt[o] is the divisor its first lane holds.  Returns the tiles walked,
// or -1 if a share leaves the image, is wider than 4 columns, or the lanes of a block do not agree on cnt.
long long thumb_host_cover(uint32_t w, uint32_t h, uint32_t f, uint8_t* reads, uint32_t* share, uint32_t* cnt) {
    uint32_t lg, c;
    qoimi::thumb_split(f, lg, c);
    const uint32_t tw = qoimi::thumb_extent(w, f), th = qoimi::thumb_extent(h, f);
    const uint64_t tiles = qoimi::thumb_tiles(w, h, f);
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint32_t lane = 0; lane < qoimi::kThumbThreads; ++lane) {
            const uint32_t item = (uint32_t)t * qoimi::kThumbThreads + lane;
            const qoimi::ThumbShare s = qoimi::thumb_share(item, w, h, tw, th, f, lg, c);
            if (s.o >= tw * th) continue;
            if (s.n > 4u || (s.n != 0u && s.x0 + s.n > w) || s.y1 > h || s.y0 >= s.y1) return -1;   // (n == 0: the lane reads nothing)
            if ((item & ((1u << lg) - 1u)) == 0u) cnt[s.o] = s.cnt;
            else if (cnt[s.o] != s.cnt) return -1;
            for (uint32_t y = s.y0; y < s.y1; ++y)
                for (uint32_t x = s.x0; x < s.x0 + s.n; ++x) ++reads[(size_t)y * w + x];
            share[s.o] += s.n * (s.y1 - s.y0);
        }
    return (long long)tiles;
}

void thumb_host_split(uint32_t f, uint32_t* lg, uint32_t* c) { qoimi::thumb_split(f, *lg, *c); }

uint32_t thumb_host_extent(uint32_t n, uint32_t f) { return qoimi::thumb_extent(n, f); }

}

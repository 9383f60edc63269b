// resize_host.cpp — the arithmetic of qoimi_decode_resized (qoi_amd/csrc/qoi_resize_core.h) compiled for the host: the walk of resize_filter over
// an item, tile by tile and lane by lane, over a synthetic staging array and the checking memory functor of host_mem.h (StagedMem), so that
// tests/test_resize_core_host.py can compare it with the Python model without a GPU.  The sums of a pixel's lanes are added here where the
// kernel takes its butterfly steps.  With -DRESIZE_HOST_MAIN the same source is a stand-alone program that walks a grid of items against a
// plain loop over all taps (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_resize_core.h"
#include "host_mem.h"

extern "C" {

// One item as resize_filter walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base].
// writes[i] counts the stores to out[i].  Returns the loads made, or -1 - the number of bad accesses if there was one; *tiles_walked
// reports the tiles.
long long resize_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                          uint32_t flags, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len,
                          unsigned long long* tiles_walked) {
    long long bad = 0, loads = 0;
    const hostmem::StagedMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, &loads};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, flags};
    uint32_t lg, c;
    qoimi::resize_split(cw, ow, lg, c);
    const uint64_t tiles = qoimi::resize_tiles(cw, ow, oh), pixels = (uint64_t)ow * oh;
    const bool wgt = weighted != 0 && och == 4u;
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint32_t lane = 0; lane < qoimi::kResizeThreads; lane += 1u << lg) {       // the lanes of one output pixel
            const uint64_t o = (t * qoimi::kResizeThreads + lane) >> lg;
            if (o >= pixels) continue;
            const uint32_t Y = (uint32_t)qoimi::resize_div(o, ow), X = (uint32_t)(o - (uint64_t)Y * ow);
            qoimi::ResizeSums sum = {{0, 0, 0, 0}, {0, 0, 0}};
            for (uint32_t l = 0; l < (1u << lg); ++l) {
                qoimi::ResizeSums s;
                if (wgt) qoimi::resize_lane<true>(mem, g, X, Y, l, c, s);
                else qoimi::resize_lane<false>(mem, g, X, Y, l, c, s);
                for (int k = 0; k < 4; ++k) sum.S[k] += s.S[k];
                for (int k = 0; k < 3; ++k) sum.W[k] += s.W[k];
            }
            qoimi::resize_finish(mem, g, q, och, wgt, X, Y, sum);
        }
    if (tiles_walked) *tiles_walked = tiles;
    return hostmem::checked(bad, loads);
}

void resize_host_split(uint32_t cw, uint32_t ow, uint32_t* lg, uint32_t* c) { qoimi::resize_split(cw, ow, *lg, *c); }
uint32_t resize_host_taps(uint32_t cw, uint32_t ow) { return qoimi::resize_taps(cw, ow); }
unsigned long long resize_host_tiles(uint32_t cw, uint32_t ow, uint32_t oh) { return qoimi::resize_tiles(cw, ow, oh); }
uint32_t resize_host_div_round(uint64_t n, uint64_t d) { return qoimi::resize_div_round(n, d); }

}

#ifdef RESIZE_HOST_MAIN
#include <stdio.h>

static uint64_t overlap(uint64_t X, uint64_t n_src, uint64_t k, uint64_t n_out) {
    const uint64_t lo = X * n_src > k * n_out ? X * n_src : k * n_out, hi = (X + 1) * n_src < (k + 1) * n_out ? (X + 1) * n_src : (k + 1) * n_out;
    return hi > lo ? hi - lo : 0;
}

// Every och, mode and flag value, a set of alignments and of size pairs (identity, whole multiples, fractions, upscales, the cap with 65 taps,
// more than one tile), in arrays of exactly the size the walk may touch: the staging ends with the item's last row, the output with its guard band.
int main() {
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {11, 9, 3, 2}, {11, 9, 13, 11}, {11, 9, 11, 9}, {12, 8, 3, 2}, {5, 3, 13, 7}, {1, 1, 4, 3}, {127, 3, 2, 3},
                                 {128, 64, 2, 1}, {9, 130, 20, 3}, {40, 40, 37, 23}};
    const uint64_t base = 4096, guard = 32;
    long long items = 0;
    for (uint32_t och = 3; och <= 4; ++och)
        for (int weighted = 0; weighted < 2; ++weighted)
            for (uint32_t a : {0u, 1u, 2u, 3u, 7u, 15u})
                for (uint32_t flags = 0; flags < 4; ++flags)
                    for (const auto& sz : sizes) {
                        const uint32_t cw = sz[0], rh = sz[1], ow = sz[2], oh = sz[3], x = 3, y = 2, w = cw + 5;
                        std::vector<uint32_t> stage((size_t)w * (y + rh));
                        for (size_t i = 0; i < stage.size(); ++i) {
                            stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                            if (i % 5u == 0u) stage[i] &= 0x00FFFFFFu;                       // some transparent pixels
                        }
                        const uint64_t B = (uint64_t)ow * oh * och, T = (uint64_t)cw * rh;
                        std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                        const uint64_t q = base + guard + a;
                        unsigned long long tiles = 0;
                        const long long rc = resize_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, och, weighted, q, base, out.data(),
                                                             writes.data(), out.size(), &tiles);
                        if (rc < 0) { printf("bad access: och %u a %u flags %u %ux%u -> %ux%u: %lld\n", och, a, flags, cw, rh, ow, oh, rc); return 1; }
                        const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                        if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                        for (uint32_t Y = 0; Y < oh; ++Y)
                            for (uint32_t X = 0; X < ow; ++X) {
                                uint64_t N[4] = {0, 0, 0, 0}, M[3] = {0, 0, 0};
                                for (uint32_t r = 0; r < rh; ++r)
                                    for (uint32_t k = 0; k < cw; ++k) {
                                        const uint64_t wt = overlap(Y, rh, r, oh) * overlap(X, cw, k, ow);
                                        const uint32_t px = stage[(size_t)(y + r) * w + x + k];
                                        for (int ch = 0; ch < 4; ++ch) N[ch] += wt * ((px >> (8 * ch)) & 255u);
                                        for (int ch = 0; ch < 3; ++ch) M[ch] += wt * ((px >> (8 * ch)) & 255u) * (px >> 24);
                                    }
                                for (uint32_t ch = 0; ch < och; ++ch) {
                                    uint64_t v = (N[ch] + T / 2) / T;
                                    if (weighted && och == 4u && ch < 3u && N[3] > 0) v = (M[ch] + N[3] / 2) / N[3];
                                    if (out[guard + a + hostmem::element_index(false, flags, ow, oh, och, X, Y, ch)] != (uint8_t)v) {
                                        printf("wrong byte: och %u mode %d a %u flags %u %ux%u -> %ux%u at (%u, %u).%u\n", och, weighted, a, flags, cw, rh, ow, oh, X, Y, ch);
                                        return 1;
                                    }
                                }
                            }
                        ++items;
                    }
    printf("resize_host: %lld items ok\n", items);
    return 0;
}
#endif

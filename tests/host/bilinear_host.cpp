// bilinear_host.cpp — the arithmetic of qoimi_decode_bilinear (qoi_amd/csrc/qoi_bilinear_core.h) compiled for the host: the walk of
// bilinear_filter over an item, tile by tile and lane by lane, over a synthetic staging array and the checking memory functors of host_mem.h
// (StagedMem, SynthMem), so that tests/test_bilinear_core_host.py can compare it with the Python model without a GPU.  The sums of a pixel's lanes are added
// here where the kernel takes its butterfly steps.  bilinear_host_pixel computes single output pixels of geometries no array can hold: its
// functor makes a staged pixel from its index.  With -DBILINEAR_HOST_MAIN the same source is a stand-alone program that walks a grid of items
// against a plain loop over all taps (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_bilinear_core.h"
#include "host_mem.h"

namespace {

template <class Mem>
void pixel_sums(const Mem& mem, const qoimi::ResizeGeom& g, uint32_t X, uint32_t Y, bool wgt, qoimi::BilinearSums& sum) {
    uint32_t lg, c;
    qoimi::bilinear_split(g.cw, g.ow, lg, c);
    sum = qoimi::BilinearSums{{{0, 0, 0, 0}, {0, 0, 0}}, 0, 0};
    for (uint32_t l = 0; l < (1u << lg); ++l) {
        qoimi::BilinearSums s;
        if (wgt) qoimi::bilinear_lane<true>(mem, g, X, Y, l, c, s);
        else qoimi::bilinear_lane<false>(mem, g, X, Y, l, c, s);
        for (int k = 0; k < 4; ++k) sum.v.S[k] += s.v.S[k];
        for (int k = 0; k < 3; ++k) sum.v.W[k] += s.v.W[k];
        sum.wx += s.wx;                                                 // (the butterfly adds wx; wy stays lane 0's)
        if (l == 0u) sum.wy = s.wy;
    }
}

}  // namespace

extern "C" {

// One item as bilinear_filter walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base].
// writes[i] counts the stores to out[i].  Returns the loads made, or -1 - the number of bad accesses if there was one; *tiles_walked
// reports the tiles.
long long bilinear_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                            uint32_t flags, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len,
                            unsigned long long* tiles_walked) {
    long long bad = 0, loads = 0;
    const hostmem::StagedMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, &loads};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, flags};
    uint32_t lg, c;
    qoimi::bilinear_split(cw, ow, lg, c);
    const uint64_t tiles = qoimi::bilinear_tiles(cw, ow, oh), pixels = (uint64_t)ow * oh;
    const bool wgt = weighted != 0 && och == 4u;
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint32_t lane = 0; lane < qoimi::kResizeThreads; lane += 1u << lg) {       // the lanes of one output pixel
            const uint64_t o = (t * qoimi::kResizeThreads + lane) >> lg;
            if (o >= pixels) continue;
            const uint32_t Y = (uint32_t)qoimi::resize_div(o, ow), X = (uint32_t)(o - (uint64_t)Y * ow);
            qoimi::BilinearSums sum;
            pixel_sums(mem, g, X, Y, wgt, sum);
            qoimi::bilinear_finish(mem, g, q, och, wgt, X, Y, sum);
        }
    if (tiles_walked) *tiles_walked = tiles;
    return hostmem::checked(bad, loads);
}

// Output pixel (X, Y) of the unflipped result of an item over synthetic staged pixels (rows of w, stage_px of them), 4 channels, written as
// one dword to *px; sums[0..6] receive N_r, N_g, N_b, N_a, M_r, M_g, M_b, sums[7] Wx, sums[8] Wy.  Returns the loads, or -1 - bad accesses.
long long bilinear_host_pixel(uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, int weighted,
                              uint32_t X, uint32_t Y, uint32_t* px, uint64_t* sums) {
    long long bad = 0, loads = 0, stores = 0;
    const hostmem::SynthMem mem = {stage_px, px, &bad, &loads, &stores};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, 0u};
    qoimi::BilinearSums sum;
    pixel_sums(mem, g, X, Y, weighted != 0, sum);
    qoimi::bilinear_finish(mem, g, 0u, 4u, weighted != 0, X, Y, sum);
    for (int k = 0; k < 4; ++k) sums[k] = sum.v.S[k];
    for (int k = 0; k < 3; ++k) sums[4 + k] = sum.v.W[k];
    sums[7] = sum.wx; sums[8] = sum.wy;
    if (stores != 1) ++bad;
    return hostmem::checked(bad, loads);
}

uint32_t bilinear_host_synth(uint64_t i) { return hostmem::SynthMem::synth(i); }

void bilinear_host_split(uint32_t cw, uint32_t ow, uint32_t* lg, uint32_t* c) { qoimi::bilinear_split(cw, ow, *lg, *c); }
uint32_t bilinear_host_taps(uint32_t cw, uint32_t ow) { return qoimi::bilinear_taps(cw, ow); }
uint32_t bilinear_host_first(uint32_t Z, uint32_t n_src, uint32_t n_out) { return qoimi::bilinear_first(Z, n_src, n_out); }
uint32_t bilinear_host_tent(uint32_t Z, uint32_t k, uint32_t n_src, uint32_t n_out) {
    return qoimi::bilinear_tent((2ull * Z + 1u) * n_src, k, n_out, qoimi::bilinear_rad(n_src, n_out));
}
unsigned long long bilinear_host_tiles(uint32_t cw, uint32_t ow, uint32_t oh) { return qoimi::bilinear_tiles(cw, ow, oh); }

}

#ifdef BILINEAR_HOST_MAIN
#include <stdio.h>

static uint64_t tent(uint64_t Z, uint64_t k, uint64_t n_src, uint64_t n_out) {
    const uint64_t rad = 2 * (n_src > n_out ? n_src : n_out), o = (2 * Z + 1) * n_src, c = (2 * k + 1) * n_out, d = o > c ? o - c : c - o;
    return d < rad ? rad - d : 0;
}

// Every och, mode and flag value, a set of alignments and of size pairs (identity, reductions up to the cap with 64 taps, enlargements, mixed
// axes, more than one tile), in arrays of exactly the size the walk may touch: the staging ends with the item's last row, the output with its
// guard band.
int main() {
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {11, 9, 3, 2}, {11, 9, 13, 11}, {11, 9, 11, 9}, {12, 8, 3, 2}, {5, 3, 13, 7}, {1, 1, 4, 3}, {63, 3, 2, 3},
                                 {128, 64, 4, 2}, {9, 130, 20, 5}, {40, 40, 37, 23}, {3, 1, 2, 1}};
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
                        const uint64_t B = (uint64_t)ow * oh * och;
                        std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                        const uint64_t q = base + guard + a;
                        unsigned long long tiles = 0;
                        const long long rc = bilinear_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, och, weighted, q, base, out.data(),
                                                               writes.data(), out.size(), &tiles);
                        if (rc < 0) { printf("bad access: och %u a %u flags %u %ux%u -> %ux%u: %lld\n", och, a, flags, cw, rh, ow, oh, rc); return 1; }
                        const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                        if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                        for (uint32_t Y = 0; Y < oh; ++Y)
                            for (uint32_t X = 0; X < ow; ++X) {
                                uint64_t N[4] = {0, 0, 0, 0}, M[3] = {0, 0, 0}, Wx = 0, Wy = 0;
                                for (uint32_t k = 0; k < cw; ++k) Wx += tent(X, k, cw, ow);
                                for (uint32_t r = 0; r < rh; ++r) Wy += tent(Y, r, rh, oh);
                                for (uint32_t r = 0; r < rh; ++r)
                                    for (uint32_t k = 0; k < cw; ++k) {
                                        const uint64_t wt = tent(Y, r, rh, oh) * tent(X, k, cw, ow);
                                        const uint32_t px = stage[(size_t)(y + r) * w + x + k];
                                        for (int ch = 0; ch < 4; ++ch) N[ch] += wt * ((px >> (8 * ch)) & 255u);
                                        for (int ch = 0; ch < 3; ++ch) M[ch] += wt * ((px >> (8 * ch)) & 255u) * (px >> 24);
                                    }
                                const uint64_t D = Wx * Wy;
                                for (uint32_t ch = 0; ch < och; ++ch) {
                                    uint64_t v = (N[ch] + D / 2) / D;
                                    if (weighted && och == 4u && ch < 3u && N[3] > 0) v = (M[ch] + N[3] / 2) / N[3];
                                    if (out[guard + a + hostmem::element_index(false, flags, ow, oh, och, X, Y, ch)] != (uint8_t)v) {
                                        printf("wrong byte: och %u mode %d a %u flags %u %ux%u -> %ux%u at (%u, %u).%u\n", och, weighted, a, flags, cw, rh, ow, oh, X, Y, ch);
                                        return 1;
                                    }
                                }
                            }
                        ++items;
                    }
    printf("bilinear_host: %lld items ok\n", items);
    return 0;
}
#endif

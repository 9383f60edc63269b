// warp_bicubic_host.cpp — qoimi_decode_warped with QOIMI_WARP_BICUBIC (qoi_amd/csrc/qoi_warp_cubic_core.h: warp_cubic_work, warp_cubic_pixel)
// compiled for the host: the walk of warp_bicubic_bytes over an item, tile by tile and work item by work item, over a synthetic staging array
// and the checking memory functor of host_mem.h (RectMem), so that tests/test_warp_bicubic_core_host.py can compare it with the Python model without a GPU.  With
// -DWARP_BICUBIC_HOST_MAIN the same source is a stand-alone program that walks a grid of items against a plain loop over the sixteen samples
// with weights made by division (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_warp_cubic_core.h"
#include "host_mem.h"

extern "C" {

// One item as warp_bicubic_bytes walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base];
// m holds a, b, c, d, e, f; flags as the item's (kWarpBicubic among them, or not).  writes[i] counts the stores to out[i].  Returns the loads
// made, or -1 - the number of bad accesses if there was one.
long long warp_bicubic_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                                uint32_t flags, const long long* m, uint32_t fill, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out,
                                uint8_t* writes, uint64_t out_len) {
    long long bad = 0, loads = 0;
    const hostmem::RectMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, w, x, y, cw, rh, &loads};
    const qoimi::WarpGeom g = {w, x, y, cw, rh, ow, oh, flags, (int32_t)m[0], (int32_t)m[1], (int32_t)m[3], (int32_t)m[4], fill, m[2], m[5]};
    const uint64_t tiles = qoimi::warp_tiles(ow, oh);
    const bool wgt = weighted != 0 && och == 4u;
    const qoimi::WarpByteSink sink;
    for (uint64_t tile = 0; tile < tiles; ++tile)
        for (uint32_t t = 0; t < qoimi::kWarpThreads; ++t) {
            if (wgt) qoimi::warp_cubic_work<true>(mem, g, q, och, (uint32_t)tile, t, sink);
            else qoimi::warp_cubic_work<false>(mem, g, q, och, (uint32_t)tile, t, sink);
        }
    return hostmem::checked(bad, loads);
}

unsigned warp_bicubic_host_flag() { return qoimi::kWarpBicubic; }

// The four weights of the fraction fr
void warp_bicubic_host_weights(uint32_t fr, int32_t* q) { qoimi::warp_cubic_weights(fr, q); }

}

#ifdef WARP_BICUBIC_HOST_MAIN
#include <stdio.h>

// floor(p / 2^17) and the remainder without shifting a negative number
static void split17(long long P, long long& k0, long long& fr) {
    const long long p = P - 65536;
    k0 = p >= 0 ? p / 131072 : -((-p + 131071) / 131072);
    fr = p - k0 * 131072;
}

static long long floor_div(long long n, long long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }

// The weights of a fraction from the expanded polynomial and a flooring division
static void weights(long long fr, long long q[4]) {
    const long long u = 131072, d[4] = {u + fr, fr, u - fr, 2 * u - fr};
    long long c[4], sum = 0, best = 0;
    int jbest = 0;
    for (int j = 0; j < 4; ++j) {
        const long long t = d[j];
        c[j] = t >= 2 * u ? 0 : (t <= u ? 3 * t * t * t - 5 * u * t * t + 2 * u * u * u : -t * t * t + 5 * u * t * t - 8 * u * u * t + 4 * u * u * u);
        if (c[j] > best) { best = c[j]; jbest = j; }
        q[j] = floor_div(c[j] + (1ll << 36), 1ll << 37);                  // (c * 2^15 + W/2) / W with W = 2^52, reduced by 2^15
        sum += q[j];
    }
    q[jbest] += 32768 - sum;
}

static uint8_t clamp8(long long v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// Every och, mode and border, a set of alignments, outputs of one pixel, of one row and one column past a tile and of several tiles,
// rectangles of one pixel and of 2 x 2, maps that turn, shear, reduce, enlarge, reach past the top-left corner, leave the rectangle altogether
// and stand at the limits, in arrays of exactly the size the walk may touch: the staging ends with the item's last row, the output with its
// guard band.
int main() {
    const uint32_t sizes[][4] = {{11, 9, 1, 1}, {11, 9, 17, 1}, {11, 9, 1, 17}, {11, 9, 33, 18}, {1, 1, 5, 4}, {2, 2, 7, 5}, {40, 30, 16, 16}};
    const long long S = 65536;
    const uint64_t base = 4096, guard = 32;
    long long items = 0, taken = 0, spared = 0;
    for (uint32_t fr = 0; fr < 131072u; fr += 7u) {                  // the weights alone, a sweep of fractions
        int32_t got[4];
        long long want[4];
        qoimi::warp_cubic_weights(fr, got);
        weights(fr, want);
        for (int j = 0; j < 4; ++j) if (got[j] != want[j]) { printf("weight %d of fraction %u\n", j, fr); return 1; }
    }
    for (uint32_t och = 3; och <= 4; ++och)
        for (int weighted = 0; weighted < 2; ++weighted)
            for (uint32_t a : {0u, 1u, 2u, 3u, 7u, 12u})
                for (uint32_t replicate = 0; replicate < 2; ++replicate)
                    for (const auto& sz : sizes)
                        for (int map = 0; map < 8; ++map) {
                            const uint32_t cw = sz[0], rh = sz[1], ow = sz[2], oh = sz[3], x = 3, y = 2, w = cw + 5, fill = 0x80C04020u, flags = replicate | 16u;
                            const long long maps[8][6] = {{S, 0, 0, 0, S, 0},                                                    // identity (cut or padded)
                                                          {0, -S, 2 * S * cw, S, 0, 0},                                          // a quarter turn
                                                          {56756, -32768, S * cw - 56756ll * ow + 32768ll * oh, 32768, 56756, S * rh - 32768ll * ow - 56756ll * oh},
                                                          {S, 23000, -40000, -9000, S + 700, 12345},                             // a shear
                                                          {177124, 0, -3 * S, 0, 21140, 5},                                      // down in x, up in y
                                                          {S, 0, -5 * S - 1, 0, S, -3 * S - 1},                                  // past the top-left corner: negative positions
                                                          {S, 0, 40 * S * cw, 0, S, -37 * S * rh},                               // everything outside
                                                          {-2147483647ll - 1, 2147483647, (1ll << 56) - 1, 3, -5, 1 - (1ll << 56)}};  // the limits
                            const long long* m = maps[map];
                            std::vector<uint32_t> stage((size_t)w * (y + rh));
                            for (size_t i = 0; i < stage.size(); ++i) {
                                stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                                if (i % 3u != 0u) stage[i] &= 0x00FFFFFFu;                       // mostly transparent pixels: A <= 0 arises
                            }
                            const uint64_t B = (uint64_t)ow * oh * och;
                            std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                            const uint64_t q = base + guard + a;
                            const long long rc = warp_bicubic_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, m, fill, och, weighted, q, base,
                                                                       out.data(), writes.data(), out.size());
                            if (rc < 0) { printf("bad access: och %u a %u flags %u map %d %ux%u -> %ux%u: %lld\n", och, a, flags, map, cw, rh, ow, oh, rc); return 1; }
                            const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                            if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                            long long want_loads = 0;
                            for (uint32_t Y = 0; Y < oh; ++Y)
                                for (uint32_t X = 0; X < ow; ++X) {
                                    const long long U = 2ll * X + 1, V = 2ll * Y + 1;
                                    long long kx, fx, ky, fy, qx[4], qy[4];
                                    split17(m[0] * U + m[1] * V + m[2], kx, fx);
                                    split17(m[3] * U + m[4] * V + m[5], ky, fy);
                                    weights(fx, qx);
                                    weights(fy, qy);
                                    long long N[4] = {0, 0, 0, 0}, M[3] = {0, 0, 0};
                                    for (int r = 0; r < 4; ++r)
                                        for (int k = 0; k < 4; ++k) {
                                            const long long wt = qy[r] * qx[k];
                                            if (wt == 0) { ++spared; continue; }
                                            long long rr = ky - 1 + r, kk = kx - 1 + k;
                                            if (replicate) {
                                                rr = rr < 0 ? 0 : (rr >= (long long)rh ? (long long)rh - 1 : rr);
                                                kk = kk < 0 ? 0 : (kk >= (long long)cw ? (long long)cw - 1 : kk);
                                            }
                                            const bool in = rr >= 0 && rr < (long long)rh && kk >= 0 && kk < (long long)cw;
                                            const uint32_t px = in ? stage[(size_t)(y + rr) * w + x + kk] : fill;
                                            want_loads += in ? 1 : 0;
                                            for (int ch = 0; ch < 4; ++ch) N[ch] += wt * (long long)((px >> (8 * ch)) & 255u);
                                            for (int ch = 0; ch < 3; ++ch) M[ch] += wt * (long long)(((px >> (8 * ch)) & 255u) * (px >> 24));
                                        }
                                    for (uint32_t ch = 0; ch < och; ++ch) {
                                        uint8_t v = clamp8(floor_div(N[ch] + (1ll << 29), 1ll << 30));
                                        if (weighted && och == 4u && ch < 3u && N[3] > 0) v = clamp8(floor_div(M[ch] + N[3] / 2, N[3]));
                                        if (out[guard + a + ((size_t)Y * ow + X) * och + ch] != v) {
                                            printf("wrong byte: och %u mode %d a %u flags %u map %d %ux%u -> %ux%u at (%u, %u).%u\n", och, weighted, a, flags, map, cw, rh, ow, oh, X, Y, ch);
                                            return 1;
                                        }
                                    }
                                }
                            if (rc != want_loads) { printf("%lld loads, %lld samples with a weight inside: map %d flags %u\n", rc, want_loads, map, flags); return 1; }
                            taken += want_loads;
                            ++items;
                        }
    if (taken == 0 || spared == 0) { printf("no sample taken or none spared\n"); return 1; }
    printf("warp_bicubic_host: %lld items ok\n", items);
    return 0;
}
#endif

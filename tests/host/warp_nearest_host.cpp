// warp_nearest_host.cpp — qoimi_decode_warped with QOIMI_WARP_NEAREST (qoi_amd/csrc/qoi_warp_core.h: warp_work, warp_nearest) compiled for the
// host: the walk of warp_gather over an item whose flags hold kWarpNearest, tile by tile and work item by work item, over a synthetic staging
// array and the checking memory functor of host_mem.h (RectMem), so that tests/test_nearest_core_host.py can compare it with the Python model without a GPU.  With -DWARP_NEAREST_HOST_MAIN
// the same source is a stand-alone program that walks a grid of items against a plain loop that floors by division (the test builds it with
// -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_warp_core.h"
#include "host_mem.h"

extern "C" {

// One item as warp_gather walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base]; m holds
// a, b, c, d, e, f; flags as the item's (kWarpNearest among them, or not).  writes[i] counts the stores to out[i].  Returns the loads made, or
// -1 - the number of bad accesses if there was one.
long long warp_nearest_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                                uint32_t flags, const long long* m, uint32_t fill, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out,
                                uint8_t* writes, uint64_t out_len) {
    long long bad = 0, loads = 0;
    const hostmem::RectMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, w, x, y, cw, rh, &loads};
    const qoimi::WarpGeom g = {w, x, y, cw, rh, ow, oh, flags, (int32_t)m[0], (int32_t)m[1], (int32_t)m[3], (int32_t)m[4], fill, m[2], m[5]};
    const uint64_t tiles = qoimi::warp_tiles(ow, oh);
    const bool wgt = weighted != 0 && och == 4u;
    for (uint64_t tile = 0; tile < tiles; ++tile)
        for (uint32_t t = 0; t < qoimi::kWarpThreads; ++t) {
            if (wgt) qoimi::warp_work<true>(mem, g, q, och, (uint32_t)tile, t);
            else qoimi::warp_work<false>(mem, g, q, och, (uint32_t)tile, t);
        }
    return hostmem::checked(bad, loads);
}

unsigned warp_nearest_host_flag() { return qoimi::kWarpNearest; }

}

#ifdef WARP_NEAREST_HOST_MAIN
#include <stdio.h>

// floor(P / 2^17) without shifting a negative number
static long long floor17(long long P) { return P >= 0 ? P / 131072 : -((-P + 131071) / 131072); }

// Every och, mode and border, a set of alignments, outputs of one pixel, of one row and one column past a tile and of several tiles, a
// rectangle of one pixel, maps that turn, shear, reduce, enlarge, reach past the top-left corner and leave the rectangle altogether, in
// arrays of exactly the size the walk may touch: the staging ends with the item's last row, the output with its guard band.
int main() {
    const uint32_t sizes[][4] = {{11, 9, 1, 1}, {11, 9, 17, 1}, {11, 9, 1, 17}, {11, 9, 33, 18}, {1, 1, 5, 4}, {40, 30, 16, 16}};
    const long long S = 65536;
    const uint64_t base = 4096, guard = 32;
    long long items = 0, filled = 0, taken = 0;
    for (uint32_t och = 3; och <= 4; ++och)
        for (int weighted = 0; weighted < 2; ++weighted)
            for (uint32_t a : {0u, 1u, 2u, 3u, 7u, 12u})
                for (uint32_t replicate = 0; replicate < 2; ++replicate)
                    for (const auto& sz : sizes)
                        for (int map = 0; map < 8; ++map) {
                            const uint32_t cw = sz[0], rh = sz[1], ow = sz[2], oh = sz[3], x = 3, y = 2, w = cw + 5, fill = 0x80C04020u, flags = replicate | 4u;
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
                            for (size_t i = 0; i < stage.size(); ++i) stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                            const uint64_t B = (uint64_t)ow * oh * och;
                            std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                            const uint64_t q = base + guard + a;
                            const long long rc = warp_nearest_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, m, fill, och, weighted, q, base,
                                                                       out.data(), writes.data(), out.size());
                            if (rc < 0) { printf("bad access: och %u a %u flags %u map %d %ux%u -> %ux%u: %lld\n", och, a, flags, map, cw, rh, ow, oh, rc); return 1; }
                            const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                            if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                            long long want_loads = 0;
                            for (uint32_t Y = 0; Y < oh; ++Y)
                                for (uint32_t X = 0; X < ow; ++X) {
                                    const long long U = 2ll * X + 1, V = 2ll * Y + 1;
                                    long long kk = floor17(m[0] * U + m[1] * V + m[2]), rr = floor17(m[3] * U + m[4] * V + m[5]);
                                    if (replicate) {
                                        rr = rr < 0 ? 0 : (rr >= (long long)rh ? (long long)rh - 1 : rr);
                                        kk = kk < 0 ? 0 : (kk >= (long long)cw ? (long long)cw - 1 : kk);
                                    }
                                    const bool in = rr >= 0 && rr < (long long)rh && kk >= 0 && kk < (long long)cw;
                                    const uint32_t px = in ? stage[(size_t)(y + rr) * w + x + kk] : fill;
                                    want_loads += in ? 1 : 0;
                                    for (uint32_t ch = 0; ch < och; ++ch)
                                        if (out[guard + a + ((size_t)Y * ow + X) * och + ch] != (uint8_t)(px >> (8 * ch))) {
                                            printf("wrong byte: och %u mode %d a %u flags %u map %d %ux%u -> %ux%u at (%u, %u).%u\n", och, weighted, a, flags, map, cw, rh, ow, oh, X, Y, ch);
                                            return 1;
                                        }
                                }
                            if (rc != want_loads) { printf("%lld loads, %lld samples inside\n", rc, want_loads); return 1; }
                            taken += want_loads; filled += (long long)ow * oh - want_loads;
                            ++items;
                        }
    if (taken == 0 || filled == 0) { printf("no sample taken or none filled\n"); return 1; }
    printf("warp_nearest_host: %lld items ok\n", items);
    return 0;
}
#endif

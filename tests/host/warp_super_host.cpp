// warp_super_host.cpp — qoimi_decode_warped with QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4 (qoi_amd/csrc/qoi_warp_super_core.h: warp_super_work,
// warp_super_pixel, warp_super_position) compiled for the host: the walk of warp_super_bytes over an item, tile by tile and work item by work
// item, over a synthetic staging array and the checking memory functor of host_mem.h (RectMem: a load beside the rectangle is bad), so that
// tests/test_warp_super_core_host.py can compare it with the Python model without a GPU.  With -DWARP_SUPER_HOST_MAIN the same source is a
// stand-alone program that walks a grid of items against a plain loop over the sub-samples and their taps written with flooring divisions
// (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_warp_super_core.h"
#include "host_mem.h"

extern "C" {

// One item as warp_super_bytes walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base];
// m holds a, b, c, d, e, f; flags as the item's (a SUPER flag among them, or not).  writes[i] counts the stores to out[i].  Returns the loads
// made, or -1 - the number of bad accesses if there was one.
long long warp_super_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
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
            if (wgt) qoimi::warp_super_work<true>(mem, g, q, och, (uint32_t)tile, t, sink);
            else qoimi::warp_super_work<false>(mem, g, q, och, (uint32_t)tile, t, sink);
        }
    return hostmem::checked(bad, loads);
}

// kWarpSuper2, kWarpSuper4
void warp_super_host_flags(unsigned* out) { out[0] = qoimi::kWarpSuper2; out[1] = qoimi::kWarpSuper4; }

// The position of sub-sample (i, j) of output pixel (X, Y) on the axis with the coefficients (m, n, o)
long long warp_super_host_position(int m, int n, long long o, uint32_t X, uint32_t Y, uint32_t i, uint32_t j, uint32_t L) {
    return qoimi::warp_super_position(m, n, o, X, Y, i, j, L);
}

}

#ifdef WARP_SUPER_HOST_MAIN
#include <stdio.h>

static long long floor_div(long long n, long long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }
static long long floor_mod(long long n, long long d) { return n - floor_div(n, d) * d; }

// A tap index under the border: the index inside [0, n), or -1 where the tap takes the fill
static long long index_ref(long long k, long long n, uint32_t border) {
    if (border == 0u) return k >= 0 && k < n ? k : -1;
    if (border == 1u) return k < 0 ? 0 : (k < n ? k : n - 1);
    if (border == 256u) return floor_mod(k, n);
    if (border == 64u) { const long long m = floor_mod(k, 2 * n); return m < n ? m : 2 * n - 1 - m; }
    if (n == 1) return 0;
    const long long m = floor_mod(k, 2 * n - 2);
    return m < n ? m : 2 * n - 2 - m;
}

// Both SUPER flags, every border and the fill, och and mode, odd output addresses, rectangles of 1 x 1, 1 x 7, 2 x 2 and 17 x 9 into an
// output of partial and whole tiles, maps that are the box, turn and reduce, shear, lie hundreds of periods away, stand next to the offset
// limits and have a negative a with the largest U - in arrays of exactly the size the walk may touch: the staging ends with the item's last
// row, the output with its guard band.
int main() {
    const uint32_t rects[][2] = {{1, 1}, {1, 7}, {2, 2}, {17, 9}};
    const long long S = 65536;
    const uint64_t base = 4096, guard = 32;
    long long items = 0, taken = 0, spared = 0, filled = 0, negative = 0;
    for (uint32_t L = 1; L <= 2; ++L)
        for (uint32_t border : {0u, 1u, 64u, 128u, 256u})
            for (uint32_t och = 3; och <= 4; ++och)
                for (int weighted = 0; weighted < 2; ++weighted)
                    for (uint32_t a : {0u, 3u})
                        for (const auto& rc : rects)
                            for (int map = 0; map < 7; ++map) {
                                const long long s = 1ll << L;
                                const uint32_t cw = rc[0], rh = rc[1], ow = 19, oh = 18, x = 3, y = 2, w = cw + 5, fill = 0x80C04020u;
                                const uint32_t flags = border | (L == 1u ? 1024u : 2048u);
                                const long long maps[7][6] = {{s * S, 0, 0, 0, s * S, 0},                                       // the box: every sub-sample a pixel centre
                                                              {56756 * 2, -32768 * 2, S * cw - 2 * (56756ll * ow - 32768ll * oh), 32768 * 2, 56756 * 2, S * rh - 2 * (32768ll * ow + 56756ll * oh)},
                                                              {S, 23000, -40000, -9000, S + 700, 12345},                         // a shear
                                                              {3 * S, 0, 2 * S * cw * 300 + 777, 0, 3 * S, -2 * S * rh * 500 - 999},   // hundreds of periods away
                                                              {S, 31, (1ll << 56) - 1, -17, S, 1 - (1ll << 56)},                 // next to +2^56 and -2^56
                                                              {-2147483647ll - 1, 2147483647, 1 - (1ll << 56), 3, -5, (1ll << 56) - 1},  // the limits: a negative sum under the shift
                                                              {-3 * S - 1, 1, 2 * S * cw + 5, -1, -2 * S - 3, 2 * S * rh + 1}};   // a half turn that reduces, odd sums
                                const long long* m = maps[map];
                                std::vector<uint32_t> stage((size_t)w * (y + rh));
                                for (size_t i = 0; i < stage.size(); ++i) {
                                    stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                                    if (i % 3u != 0u) stage[i] &= 0x00FFFFFFu;                   // mostly transparent pixels: A == 0 arises
                                }
                                const uint64_t B = (uint64_t)ow * oh * och;
                                std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                                const uint64_t q = base + guard + a;
                                const long long rc2 = warp_super_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, m, fill, och, weighted, q, base,
                                                                          out.data(), writes.data(), out.size());
                                if (rc2 < 0) { printf("bad access: och %u a %u flags %u map %d %ux%u: %lld\n", och, a, flags, map, cw, rh, rc2); return 1; }
                                const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                                if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                                long long want_loads = 0;
                                for (uint32_t Y = 0; Y < oh; ++Y)
                                    for (uint32_t X = 0; X < ow; ++X) {
                                        long long N[4] = {0, 0, 0, 0}, M[3] = {0, 0, 0};
                                        for (long long j = 0; j < s; ++j)
                                            for (long long i = 0; i < s; ++i) {
                                                const long long Us = s * (2ll * X + 1) + 2 * i + 1 - s, Vs = s * (2ll * Y + 1) + 2 * j + 1 - s;
                                                const long long ex = m[0] * Us + m[1] * Vs, ey = m[3] * Us + m[4] * Vs;
                                                if (ex < 0 && floor_mod(ex, s) != 0) ++negative;
                                                const long long px = floor_div(ex, s) + m[2] - 65536, py = floor_div(ey, s) + m[5] - 65536;
                                                const long long kx = floor_div(px, 131072), fx = px - kx * 131072, ky = floor_div(py, 131072), fy = py - ky * 131072;
                                                const long long wx[2] = {131072 - fx, fx}, wy[2] = {131072 - fy, fy};
                                                for (int r = 0; r < 2; ++r)
                                                    for (int k = 0; k < 2; ++k) {
                                                        const long long wt = wy[r] * wx[k];
                                                        if (wt == 0) { ++spared; continue; }
                                                        const long long ir = index_ref(ky + r, rh, border), ik = index_ref(kx + k, cw, border);
                                                        uint32_t v = fill;
                                                        if (ir >= 0 && ik >= 0) { v = stage[(size_t)(y + ir) * w + x + ik]; ++want_loads; } else ++filled;
                                                        for (int ch = 0; ch < 4; ++ch) N[ch] += wt * (long long)((v >> (8 * ch)) & 255u);
                                                        for (int ch = 0; ch < 3; ++ch) M[ch] += wt * (long long)(((v >> (8 * ch)) & 255u) * (v >> 24));
                                                    }
                                            }
                                        const long long total = (1ll << 34) * s * s;
                                        for (uint32_t ch = 0; ch < och; ++ch) {
                                            long long v = floor_div(N[ch] + total / 2, total);
                                            if (weighted && och == 4u && ch < 3u && N[3] > 0) v = floor_div(M[ch] + N[3] / 2, N[3]);
                                            if (v < 0 || v > 255 || out[guard + a + ((size_t)Y * ow + X) * och + ch] != (uint8_t)v) {
                                                printf("wrong byte: och %u mode %d a %u flags %u map %d %ux%u at (%u, %u).%u\n", och, weighted, a, flags, map, cw, rh, X, Y, ch);
                                                return 1;
                                            }
                                        }
                                    }
                                if (rc2 != want_loads) { printf("%lld loads, %lld taps with a weight inside: map %d flags %u\n", rc2, want_loads, map, flags); return 1; }
                                taken += want_loads;
                                ++items;
                            }
    if (taken == 0 || spared == 0 || filled == 0 || negative == 0) { printf("no sample taken, none spared, none filled or no negative sum floored\n"); return 1; }
    printf("warp_super_host: %lld items ok\n", items);
    return 0;
}
#endif

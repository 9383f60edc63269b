// warp_border_host.cpp — qoimi_decode_warped with QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 or QOIMI_WARP_WRAP (qoi_amd/csrc/qoi_warp_border_core.h:
// warp_border_work, warp_border_pixel, warp_fold) compiled for the host: the walk of warp_border_bytes over an item, tile by tile and work
// item by work item, over a synthetic staging array and the checking memory functor of host_mem.h (RectMem: a load beside the rectangle is
// bad), so that tests/test_warp_border_core_host.py can compare it with the Python model without a GPU.  With -DWARP_BORDER_HOST_MAIN the same
// source is a stand-alone program that sweeps the fold against the integer remainder and walks a grid of items against a plain loop over the
// taps with every index folded by that remainder (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_warp_border_core.h"
#include "host_mem.h"

extern "C" {

// One item as warp_border_bytes walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base];
// m holds a, b, c, d, e, f; flags as the item's (a border among them, or not).  writes[i] counts the stores to out[i].  Returns the loads
// made, or -1 - the number of bad accesses if there was one.
long long warp_border_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
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
            if (wgt) qoimi::warp_border_work<true>(mem, g, q, och, (uint32_t)tile, t, sink);
            else qoimi::warp_border_work<false>(mem, g, q, och, (uint32_t)tile, t, sink);
        }
    return hostmem::checked(bad, loads);
}

// kWarpReflect, kWarpReflect101, kWarpWrap
void warp_border_host_flags(unsigned* out) { out[0] = qoimi::kWarpReflect; out[1] = qoimi::kWarpReflect101; out[2] = qoimi::kWarpWrap; }

// The index k of an axis of n samples under the border
unsigned warp_border_host_fold(long long k, uint32_t n, uint32_t border) { return qoimi::warp_fold(k, n, border); }

}

#ifdef WARP_BORDER_HOST_MAIN
#include <stdio.h>

static long long floor_div(long long n, long long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }
static long long floor_mod(long long n, long long d) { return n - floor_div(n, d) * d; }

// The definition with the integer remainder
static long long fold_ref(long long k, long long n, uint32_t border) {
    if (border == 256u) return floor_mod(k, n);
    if (border == 64u) { const long long m = floor_mod(k, 2 * n); return m < n ? m : 2 * n - 1 - m; }
    if (n == 1) return 0;
    const long long m = floor_mod(k, 2 * n - 2);
    return m < n ? m : 2 * n - 2 - m;
}

// floor(p / 2^17) and the remainder without shifting a negative number
static void split17(long long p, long long& k0, long long& fr) {
    k0 = floor_div(p, 131072);
    fr = p - k0 * 131072;
}

// The bicubic weights of a fraction from the expanded polynomial and a flooring division
static void cubic_weights_ref(long long fr, long long q[4]) {
    const long long u = 131072, d[4] = {u + fr, fr, u - fr, 2 * u - fr};
    long long c[4], sum = 0, best = 0;
    int jbest = 0;
    for (int j = 0; j < 4; ++j) {
        const long long t = d[j];
        c[j] = t >= 2 * u ? 0 : (t <= u ? 3 * t * t * t - 5 * u * t * t + 2 * u * u * u : -t * t * t + 5 * u * t * t - 8 * u * u * t + 4 * u * u * u);
        if (c[j] > best) { best = c[j]; jbest = j; }
        q[j] = floor_div(c[j] + (1ll << 36), 1ll << 37);
        sum += q[j];
    }
    q[jbest] += 32768 - sum;
}

// The taps of one axis by the sampling: their count, first index and weights (nearest: one tap of weight 1)
static int taps_ref(long long P, uint32_t sampling, long long& first, long long wgt[4]) {
    long long k0, fr;
    if (sampling == 4u) { split17(P, first, fr); wgt[0] = 1; return 1; }
    split17(P - 65536, k0, fr);
    if (sampling == 16u) { first = k0 - 1; cubic_weights_ref(fr, wgt); return 4; }
    first = k0; wgt[0] = 131072 - fr; wgt[1] = fr;
    return 2;
}

static uint8_t clamp8(long long v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// The fold alone: small axes over a window of indices, and every axis at the indices where a quotient estimate could be off by one - the
// multiples of the period and their neighbours, up to the largest accepted index.
static bool sweep_fold() {
    const uint32_t ns[] = {1, 2, 3, 7, 1000, 65536, 65537, 399999999, 1u << 29};
    long long checked = 0;
    for (uint32_t border : {64u, 128u, 256u})
        for (uint32_t n : ns) {
            const long long P = border == 256u ? n : (border == 64u ? 2ll * n : (n > 1u ? 2ll * n - 2 : 1));
            const long long top = (1ll << 40) - 1;
            std::vector<long long> ks = {0, 1, -1, top, -top, top - 1, 1 - top, P - 1, P, P + 1, -P, -P - 1, -P + 1, 2 * P - 1, 2 * P, 2 * P + 1, -2 * P, -2 * P - 1};
            if (n <= 1000u) for (long long k = -3 * P - 5; k <= 3 * P + 5; ++k) ks.push_back(k);
            for (long long qv : {3ll, 1000ll, 65535ll, top / P - 1, top / P, top / (2 * P)})
                for (long long dlt : {-2ll, -1ll, 0ll, 1ll, 2ll, (long long)n - 1, (long long)n, (long long)n + 1})
                    for (long long sign : {1ll, -1ll}) ks.push_back(sign * (qv * P + dlt));
            for (long long k : ks) {
                if (k > top || k < -top) continue;
                if ((long long)qoimi::warp_fold(k, n, border) != fold_ref(k, n, border)) { printf("fold %lld of %u under %u\n", k, n, border); return false; }
                ++checked;
            }
        }
    return checked > 10000;
}

// Every border, sampling, och and mode, odd output addresses, rectangles of 1 x 1, 1 x 7, 7 x 1, 5 x 3 and 17 x 9 into an output of partial
// and whole tiles, maps that pad, turn, shear, lie hundreds of periods away and stand at the limits - the ordinary path of the fold and the
// quotient estimate both -, in arrays of exactly the size the walk may touch: the staging ends with the item's last row, the output with its
// guard band.
int main() {
    if (!sweep_fold()) return 1;
    const uint32_t rects[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 3}, {17, 9}};
    const long long S = 65536;
    const uint64_t base = 4096, guard = 32;
    long long items = 0, taken = 0, spared = 0, far = 0;
    for (uint32_t border : {64u, 128u, 256u})
        for (uint32_t sampling : {0u, 4u, 16u})
            for (uint32_t och = 3; och <= 4; ++och)
                for (int weighted = 0; weighted < 2; ++weighted)
                    for (uint32_t a : {0u, 1u, 3u})
                        for (const auto& rc : rects)
                            for (int map = 0; map < 7; ++map) {
                                const uint32_t cw = rc[0], rh = rc[1], ow = 19, oh = 18, x = 3, y = 2, w = cw + 5, fill = 0x80C04020u, flags = border | sampling;
                                const long long maps[7][6] = {{S, 0, -2 * S * 6, 0, S, -2 * S * 4},                              // the rectangle padded: pixel centres
                                                              {0, -S, 2 * S * cw, S, 0, 0},                                      // a quarter turn
                                                              {56756, -32768, S * cw - 56756ll * ow + 32768ll * oh, 32768, 56756, S * rh - 32768ll * ow - 56756ll * oh},
                                                              {S, 23000, -40000, -9000, S + 700, 12345},                         // a shear
                                                              {S, 0, 2 * S * cw * 300 + 777, 0, S, -2 * S * rh * 500 - 999},     // hundreds of periods away
                                                              {S, 0, (1ll << 56) - 1, 0, S, 1 - (1ll << 56)},                    // near +2^56 and -2^56
                                                              {-2147483647ll - 1, 2147483647, 1 - (1ll << 56), 3, -5, (1ll << 56) - 1}};  // the limits
                                const long long* m = maps[map];
                                std::vector<uint32_t> stage((size_t)w * (y + rh));
                                for (size_t i = 0; i < stage.size(); ++i) {
                                    stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                                    if (i % 3u != 0u) stage[i] &= 0x00FFFFFFu;                   // mostly transparent pixels: A <= 0 arises
                                }
                                const uint64_t B = (uint64_t)ow * oh * och;
                                std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                                const uint64_t q = base + guard + a;
                                const long long rc2 = warp_border_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, m, fill, och, weighted, q, base,
                                                                           out.data(), writes.data(), out.size());
                                if (rc2 < 0) { printf("bad access: och %u a %u flags %u map %d %ux%u: %lld\n", och, a, flags, map, cw, rh, rc2); return 1; }
                                const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                                if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                                long long want_loads = 0;
                                for (uint32_t Y = 0; Y < oh; ++Y)
                                    for (uint32_t X = 0; X < ow; ++X) {
                                        const long long U = 2ll * X + 1, V = 2ll * Y + 1;
                                        long long kx, ky, wx[4], wy[4];
                                        const int nx = taps_ref(m[0] * U + m[1] * V + m[2], sampling, kx, wx), ny = taps_ref(m[3] * U + m[4] * V + m[5], sampling, ky, wy);
                                        if (kx < -2ll * cw || kx >= 4ll * cw) ++far;
                                        long long N[4] = {0, 0, 0, 0}, M[3] = {0, 0, 0};
                                        for (int r = 0; r < ny; ++r)
                                            for (int k = 0; k < nx; ++k) {
                                                const long long wt = wy[r] * wx[k];
                                                if (wt == 0) { ++spared; continue; }
                                                const uint32_t px = stage[(size_t)(y + fold_ref(ky + r, rh, border)) * w + x + fold_ref(kx + k, cw, border)];
                                                ++want_loads;
                                                for (int ch = 0; ch < 4; ++ch) N[ch] += wt * (long long)((px >> (8 * ch)) & 255u);
                                                for (int ch = 0; ch < 3; ++ch) M[ch] += wt * (long long)(((px >> (8 * ch)) & 255u) * (px >> 24));
                                            }
                                        const long long half = sampling == 4u ? 0 : (sampling == 16u ? 1ll << 29 : 1ll << 33), total = 2 * half > 0 ? 2 * half : 1;
                                        for (uint32_t ch = 0; ch < och; ++ch) {
                                            uint8_t v = clamp8(floor_div(N[ch] + half, total));
                                            if (sampling != 4u && weighted && och == 4u && ch < 3u && N[3] > 0) v = clamp8(floor_div(M[ch] + N[3] / 2, N[3]));
                                            if (out[guard + a + ((size_t)Y * ow + X) * och + ch] != v) {
                                                printf("wrong byte: och %u mode %d a %u flags %u map %d %ux%u at (%u, %u).%u\n", och, weighted, a, flags, map, cw, rh, X, Y, ch);
                                                return 1;
                                            }
                                        }
                                    }
                                if (rc2 != want_loads) { printf("%lld loads, %lld taps with a weight: map %d flags %u\n", rc2, want_loads, map, flags); return 1; }
                                taken += want_loads;
                                ++items;
                            }
    if (taken == 0 || spared == 0 || far == 0) { printf("no sample taken, none spared or none far away\n"); return 1; }
    printf("warp_border_host: %lld items ok\n", items);
    return 0;
}
#endif

// warp_proj_host.cpp — qoimi_decode_warped with QOIMI_WARP_PROJECTIVE (qoi_amd/csrc/qoi_warp_proj_core.h: warp_proj_work,
// warp_proj_position, warp_proj_denominator, warp_proj_bits, warp_proj_least) compiled for the host: the walk of warp_proj_bytes over an
// item, tile by tile and work item by work item, over a synthetic staging array and the checking memory functor of host_mem.h (RectMem: a
// load beside the rectangle is bad), so that tests/test_warp_proj_core_host.py can compare it with the Python model without a GPU.  With
// -DWARP_PROJ_HOST_MAIN the same source is a stand-alone program that walks the quotient against a 128-bit division at its extremes and a
// grid of items against an independent restatement - the positions by 128-bit division, the nearest sample and the bilinear blend as plain
// loops with flooring divisions - (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_warp_proj_core.h"
#include "host_mem.h"

extern "C" {

// One item as warp_proj_bytes walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base];
// m holds a, b, c, d, e, f; flags and reserved as the item's (kWarpProjective among the flags, or not).  writes[i] counts the stores to
// out[i].  Returns the loads made, or -1 - the number of bad accesses if there was one.
long long warp_proj_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                             uint32_t flags, const long long* m, uint32_t reserved, uint32_t fill, uint32_t och, int weighted, uint64_t q, uint64_t base,
                             uint8_t* out, uint8_t* writes, uint64_t out_len) {
    long long bad = 0, loads = 0;
    const hostmem::RectMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, w, x, y, cw, rh, &loads};
    const qoimi::WarpGeom g = {w, x, y, cw, rh, ow, oh, flags, (int32_t)m[0], (int32_t)m[1], (int32_t)m[3], (int32_t)m[4], fill, m[2], m[5]};
    const qoimi::WarpProj pj = qoimi::warp_proj_of((flags & qoimi::kWarpProjective) != 0u ? reserved : 0u);
    const uint64_t tiles = qoimi::warp_tiles(ow, oh);
    const bool wgt = weighted != 0 && och == 4u;
    const qoimi::WarpByteSink sink;
    for (uint64_t tile = 0; tile < tiles; ++tile)
        for (uint32_t t = 0; t < qoimi::kWarpThreads; ++t) {
            if (wgt) qoimi::warp_proj_work<true>(mem, g, pj, q, och, (uint32_t)tile, t, sink);
            else qoimi::warp_proj_work<false>(mem, g, pj, q, och, (uint32_t)tile, t, sink);
        }
    return hostmem::checked(bad, loads);
}

// floor(N * 2^F / W) as the core computes it
long long warp_proj_host_position(long long N, long long W, uint32_t F) { return qoimi::warp_proj_position(N, W, F); }

// Both positions of output pixel (X, Y) of an ow x oh item as the work item forms them; W is returned
long long warp_proj_host_pixel(uint32_t ow, uint32_t oh, const long long* m, uint32_t reserved, uint32_t X, uint32_t Y, long long* P) {
    const qoimi::WarpProj pj = qoimi::warp_proj_of(reserved);
    const uint32_t F = qoimi::warp_proj_bits(ow, oh);
    const int64_t W = qoimi::warp_proj_denominator(pj, F, ow, oh, X, Y);
    P[0] = qoimi::warp_proj_position(qoimi::warp_position((int32_t)m[0], (int32_t)m[1], m[2], X, Y), W, F);
    P[1] = qoimi::warp_proj_position(qoimi::warp_position((int32_t)m[3], (int32_t)m[4], m[5], X, Y), W, F);
    return W;
}

uint32_t warp_proj_host_bits(uint32_t ow, uint32_t oh) { return qoimi::warp_proj_bits(ow, oh); }

long long warp_proj_host_least(uint32_t reserved, uint32_t ow, uint32_t oh) {
    return qoimi::warp_proj_least(qoimi::warp_proj_of(reserved), qoimi::warp_proj_bits(ow, oh), ow, oh);
}

// kWarpProjective, kWarpProjBase, kWarpProjChunk, log2 of kWarpProjMaxOffset
void warp_proj_host_consts(unsigned* out) {
    out[0] = qoimi::kWarpProjective; out[1] = qoimi::kWarpProjBase; out[2] = qoimi::kWarpProjChunk;
    out[3] = 0u;
    while ((1ll << out[3]) < qoimi::kWarpProjMaxOffset) ++out[3];
}

}

#ifdef WARP_PROJ_HOST_MAIN
#include <stdio.h>

typedef __int128 wide;

static wide floor_div(wide n, wide d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }
static long long floor_mod(long long n, long long d) { return (long long)(n - floor_div(n, d) * d); }

// A sample index under the border: the index inside [0, n), or -1 where the sample takes the fill
static long long index_ref(long long k, long long n, uint32_t border) {
    if (border == 0u) return k >= 0 && k < n ? k : -1;
    if (border == 1u) return k < 0 ? 0 : (k < n ? k : n - 1);
    if (border == 256u) return floor_mod(k, n);
    if (border == 64u) { const long long m = floor_mod(k, 2 * n); return m < n ? m : 2 * n - 1 - m; }
    if (n == 1) return 0;
    const long long m = floor_mod(k, 2 * n - 2);
    return m < n ? m : 2 * n - 2 - m;
}

static long long position_ref(long long N, long long W, uint32_t F) { return (long long)floor_div((wide)N * ((wide)1 << F), (wide)W); }

// The quotient at its extremes: N within 1 of +-2^54, W at 2^(F-3) and next to 5 * 2^F, F = 14, 17, 18, 31 and 34, negative N that floor,
// exact multiples, and a pseudo-random sweep.
static long long walk_quotients() {
    long long n = 0;
    uint64_t z = 0x9E3779B97F4A7C15ull;
    for (uint32_t F : {14u, 15u, 17u, 18u, 25u, 31u, 33u, 34u}) {
        const long long one = 1ll << F;
        const long long Ws[] = {one >> 3, (one >> 3) + 1, one - 1, one, one + 1, 2 * one - 1, 5 * one - 1, 5 * one - 2, 3 * one + 12345 % one, one - one / 3};
        const long long Ns[] = {(1ll << 54) - 1, (1ll << 54) - 2, 1 - (1ll << 54), 2 - (1ll << 54), 0, 1, -1, 65536, -65536, (1ll << 53) + 1, -(1ll << 53) - 1, 131071, -131073};
        for (long long W : Ws) {
            for (long long N : Ns) {
                if (qoimi::warp_proj_position(N, W, F) != position_ref(N, W, F)) { printf("quotient: N %lld W %lld F %u\n", N, W, F); return -1; }
                ++n;
            }
            for (long long k : {-7ll, -1ll, 1ll, 3ll, 1000003ll}) {                  // exact multiples and their neighbours: the floor at a boundary
                for (long long dlt = -1; dlt <= 1; ++dlt) {
                    const long long N = k * W + dlt;
                    if (qoimi::warp_proj_position(N, W, F) != position_ref(N, W, F)) { printf("quotient at a multiple: N %lld W %lld F %u\n", N, W, F); return -1; }
                    ++n;
                }
            }
            for (int it = 0; it < 2000; ++it) {
                z ^= z << 13; z ^= z >> 7; z ^= z << 17;
                const long long N = (long long)(z >> 9) - (1ll << 54);               // [-2^54, 2^54)
                if (N <= -(1ll << 54)) continue;
                if (qoimi::warp_proj_position(N, W, F) != position_ref(N, W, F)) { printf("quotient: N %lld W %lld F %u\n", N, W, F); return -1; }
                ++n;
            }
        }
    }
    return n;
}

// The flag with the three samplings, every border and the fill, och and mode, odd output addresses, rectangles of 1 x 1, 1 x 7, 2 x 2 and
// 17 x 9 into an output of partial and whole tiles, maps that turn, shear, lie hundreds of periods away and stand next to the offset limit
// of 2^53, with denominators that are 1 (g = h = 0), tilt either way and come next to the limit of 1/8 - in arrays of exactly the size the
// walk may touch.  Nearest and bilinear items are compared with plain loops; a bicubic item is compared with warp_cubic_pixel_at /
// warp_border_pixel_at at the independently divided positions (the cubic blend has its own harness).
int main() {
    const long long quotients = walk_quotients();
    if (quotients < 0) return 1;
    const uint32_t rects[][2] = {{1, 1}, {1, 7}, {2, 2}, {17, 9}};
    const long long S = 65536;
    const uint64_t base = 4096, guard = 32;
    long long items = 0, taken = 0, filled = 0;
    for (uint32_t sampling : {0u, 4u, 16u})
        for (uint32_t border : {0u, 1u, 64u, 128u, 256u})
            for (uint32_t och = 3; och <= 4; ++och)
                for (int weighted = 0; weighted < 2; ++weighted)
                    for (const auto& rc : rects)
                        for (int map = 0; map < 5; ++map)
                            for (int tilt = 0; tilt < 4; ++tilt) {
                                const uint32_t cw = rc[0], rh = rc[1], ow = 19, oh = 18, x = 3, y = 2, w = cw + 5, fill = 0x80FF4007u, a = (uint32_t)(map % 4);
                                const uint32_t flags = border | sampling | qoimi::kWarpProjective;
                                const uint32_t F = 14 + 5;                                   // 2^5 >= 19
                                const int ghs[4][2] = {{0, 0}, {9000, -7000}, {-25486, 0}, {12743, 13492}};   // the last two: 7/8 * 2^19 = 458752 = 25486 * 18 + 4 = 12743 * 18 + 13492 * 17 + 14
                                const int gg = ghs[tilt][0], hh = ghs[tilt][1];
                                const uint32_t reserved = ((uint32_t)gg & 0xFFFFu) | (((uint32_t)hh & 0xFFFFu) << 16);
                                const long long maps[5][6] = {{56756, -32768, S * cw - (56756ll * ow - 32768ll * oh), 32768, 56756, S * rh - (32768ll * ow + 56756ll * oh)},
                                                              {S, 23000, -40000, -9000, S + 700, 12345},                         // a shear
                                                              {3 * S, 0, 2 * S * cw * 300 + 777, 0, 3 * S, -2 * S * rh * 500 - 999},   // hundreds of periods away
                                                              {S, 31, (1ll << 53) - 1, -17, S, 1 - (1ll << 53)},                 // next to +2^53 and -2^53
                                                              {-2147483647ll - 1, 2147483647, 1 - (1ll << 53), 3, -5, (1ll << 53) - 1}};   // the limits
                                const long long* m = maps[map];
                                if (qoimi::warp_proj_bits(ow, oh) != F) { printf("F\n"); return 1; }
                                const long long least = qoimi::warp_proj_least(qoimi::warp_proj_of(reserved), F, ow, oh);
                                if (least != (1ll << F) - (gg < 0 ? -gg : gg) * 18ll - (hh < 0 ? -hh : hh) * 17ll || least < (1ll << (F - 3))) { printf("least W\n"); return 1; }
                                std::vector<uint32_t> stage((size_t)w * (y + rh));
                                for (size_t i = 0; i < stage.size(); ++i) stage[i] = hostmem::SynthMem::synth(i) | (i % 3u == 0u ? 0u : 0xFF000000u);
                                const uint64_t B = (uint64_t)ow * oh * och;
                                std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                                const uint64_t q = base + guard + a;
                                const long long rc2 = warp_proj_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, m, reserved, fill, och, weighted, q, base,
                                                                         out.data(), writes.data(), out.size());
                                if (rc2 < 0) { printf("bad access: och %u flags %u map %d tilt %d %ux%u: %lld\n", och, flags, map, tilt, cw, rh, rc2); return 1; }
                                const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                                if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                                const bool wgt = weighted != 0 && och == 4u;
                                long long want_loads = 0;
                                long long bad2 = 0, loads2 = 0;
                                const hostmem::RectMem mem = {{nullptr, nullptr, 0, 0, &bad2}, stage.data(), stage.size(), w, x, y, cw, rh, &loads2};
                                const qoimi::WarpGeom geom = {w, x, y, cw, rh, ow, oh, flags, (int32_t)m[0], (int32_t)m[1], (int32_t)m[3], (int32_t)m[4], fill, m[2], m[5]};
                                for (uint32_t Y = 0; Y < oh; ++Y)
                                    for (uint32_t X = 0; X < ow; ++X) {
                                        const long long U = 2ll * X + 1, V = 2ll * Y + 1;
                                        const long long W = (1ll << F) + gg * (U - ow) + hh * (V - oh);
                                        if (W < least) { printf("W below its least\n"); return 1; }
                                        const long long Px = position_ref(m[0] * U + m[1] * V + m[2], W, F), Py = position_ref(m[3] * U + m[4] * V + m[5], W, F);
                                        uint32_t want;
                                        if (sampling == 4u) {
                                            const long long ik = index_ref((long long)floor_div(Px, 131072), cw, border), ir = index_ref((long long)floor_div(Py, 131072), rh, border);
                                            if (ik >= 0 && ir >= 0) { want = stage[(size_t)(y + ir) * w + x + ik]; ++want_loads; }
                                            else { want = fill; ++filled; }
                                        } else if (sampling == 16u) {
                                            const long long before = loads2;
                                            if (border > 1u) want = wgt ? qoimi::warp_border_pixel_at<true>(mem, geom, Px, Py) : qoimi::warp_border_pixel_at<false>(mem, geom, Px, Py);
                                            else want = wgt ? qoimi::warp_cubic_pixel_at<true>(mem, geom, Px, Py) : qoimi::warp_cubic_pixel_at<false>(mem, geom, Px, Py);
                                            want_loads += loads2 - before;
                                        } else {
                                            const long long kx = (long long)floor_div(Px - 65536, 131072), ky = (long long)floor_div(Py - 65536, 131072);
                                            const long long fx = Px - 65536 - kx * 131072, fy = Py - 65536 - ky * 131072;
                                            const long long wx[2] = {131072 - fx, fx}, wy[2] = {131072 - fy, fy};
                                            unsigned long long Nc[4] = {0, 0, 0, 0}, Mc[3] = {0, 0, 0};
                                            for (int r = 0; r < 2; ++r)
                                                for (int k = 0; k < 2; ++k) {
                                                    if (wx[k] == 0 || wy[r] == 0) continue;         // a tap without a weight is not taken
                                                    const long long ik = index_ref(kx + k, cw, border), ir = index_ref(ky + r, rh, border);
                                                    uint32_t v = fill;
                                                    if (ik >= 0 && ir >= 0) { v = stage[(size_t)(y + ir) * w + x + ik]; ++want_loads; } else ++filled;
                                                    const unsigned long long wgt2 = (unsigned long long)(wx[k] * wy[r]);
                                                    for (int ch = 0; ch < 4; ++ch) Nc[ch] += wgt2 * ((v >> (8 * ch)) & 255u);
                                                    for (int ch = 0; ch < 3; ++ch) Mc[ch] += wgt2 * ((v >> (8 * ch)) & 255u) * (v >> 24);
                                                }
                                            want = 0;
                                            for (int ch = 0; ch < 4; ++ch) {
                                                unsigned long long val = (Nc[ch] + (1ull << 33)) >> 34;
                                                if (wgt && ch < 3 && Nc[3] > 0) val = (Mc[ch] + Nc[3] / 2) / Nc[3];
                                                want |= (uint32_t)val << (8 * ch);
                                            }
                                        }
                                        for (uint32_t ch = 0; ch < och; ++ch)
                                            if (out[guard + a + ((size_t)Y * ow + X) * och + ch] != (uint8_t)(want >> (8 * ch))) {
                                                printf("wrong byte: och %u mode %d flags %u map %d tilt %d %ux%u at (%u, %u).%u\n", och, weighted, flags, map, tilt, cw, rh, X, Y, ch);
                                                return 1;
                                            }
                                    }
                                if (bad2 != 0) { printf("the reference read beside the rectangle\n"); return 1; }
                                if (rc2 != want_loads) { printf("%lld loads, %lld samples inside: map %d flags %u\n", rc2, want_loads, map, flags); return 1; }
                                taken += want_loads;
                                ++items;
                            }
    if (taken == 0 || filled == 0) { printf("no sample taken or none filled\n"); return 1; }
    printf("warp_proj_host: %lld quotients, %lld items ok\n", quotients, items);
    return 0;
}
#endif

// warp_vote_host.cpp — qoimi_decode_warped with QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4 (qoi_amd/csrc/qoi_warp_vote_core.h: warp_vote_work,
// warp_vote_pixel, warp_vote_value) compiled for the host: the walk of warp_vote_bytes over an item, tile by tile and work item by work
// item, over a synthetic staging array and the checking memory functor of host_mem.h (RectMem: a load beside the rectangle is bad), so that
// tests/test_warp_vote_core_host.py can compare it with the Python model without a GPU.  With -DWARP_VOTE_HOST_MAIN the same source is a
// stand-alone program that walks a grid of items against a plain loop over the sub-samples written with flooring divisions and a table of
// counts (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_warp_vote_core.h"
#include "host_mem.h"

extern "C" {

// One item as warp_vote_bytes walks it: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins at out[q - base];
// m holds a, b, c, d, e, f; flags as the item's (a VOTE flag among them, or not).  writes[i] counts the stores to out[i].  Returns the loads
// made, or -1 - the number of bad accesses if there was one.
long long warp_vote_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
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
            if (wgt) qoimi::warp_vote_work<true>(mem, g, q, och, (uint32_t)tile, t, sink);
            else qoimi::warp_vote_work<false>(mem, g, q, och, (uint32_t)tile, t, sink);
        }
    return hostmem::checked(bad, loads);
}

// kWarpVote2, kWarpVote4, kWarpVotes
void warp_vote_host_flags(unsigned* out) { out[0] = qoimi::kWarpVote2; out[1] = qoimi::kWarpVote4; out[2] = qoimi::kWarpVotes; }

}

#ifdef WARP_VOTE_HOST_MAIN
#include <stdio.h>

static long long floor_div(long long n, long long d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }
static long long floor_mod(long long n, long long d) { return n - floor_div(n, d) * d; }

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

static uint32_t key_ref(uint32_t v) { return ((v & 255u) << 24) | (((v >> 8) & 255u) << 16) | (((v >> 16) & 255u) << 8) | (v >> 24); }

// Both VOTE flags, every border and the fill, och and mode, odd output addresses, rectangles of 1 x 1, 1 x 7, 2 x 2 and 17 x 9 into an
// output of partial and whole tiles, maps that are the whole-factor reduction, turn and reduce, shear, lie hundreds of periods away, stand
// next to the offset limits and have a negative a with the largest U - in arrays of exactly the size the walk may touch: the staging ends
// with the item's last row, the output with its guard band.  The staging holds few values, so that ties arise.
int main() {
    const uint32_t rects[][2] = {{1, 1}, {1, 7}, {2, 2}, {17, 9}};
    const uint32_t values[5] = {0xFF000000u, 0xFF030201u, 0x80030201u, 0xFF000007u, 0x00FFFFFFu};
    const long long S = 65536;
    const uint64_t base = 4096, guard = 32;
    long long items = 0, taken = 0, filled = 0, unique = 0, by_centre = 0, by_key = 0;
    for (uint32_t L = 1; L <= 2; ++L)
        for (uint32_t border : {0u, 1u, 64u, 128u, 256u})
            for (uint32_t och = 3; och <= 4; ++och)
                for (int weighted = 0; weighted < 2; ++weighted)
                    for (uint32_t a : {0u, 3u})
                        for (const auto& rc : rects)
                            for (int map = 0; map < 7; ++map) {
                                const long long s = 1ll << L;
                                const uint32_t cw = rc[0], rh = rc[1], ow = 19, oh = 18, x = 3, y = 2, w = cw + 5, fill = 0xFF000007u;   // (the fill is one of the values)
                                const uint32_t flags = border | (L == 1u ? 8192u : 16384u);
                                const long long maps[7][6] = {{s * S, 0, 0, 0, s * S, 0},                                       // the whole-factor reduction: every sub-sample a pixel centre
                                                              {56756 * 2, -32768 * 2, S * cw - 2 * (56756ll * ow - 32768ll * oh), 32768 * 2, 56756 * 2, S * rh - 2 * (32768ll * ow + 56756ll * oh)},
                                                              {S, 23000, -40000, -9000, S + 700, 12345},                         // a shear
                                                              {3 * S, 0, 2 * S * cw * 300 + 777, 0, 3 * S, -2 * S * rh * 500 - 999},   // hundreds of periods away
                                                              {S, 31, (1ll << 56) - 1, -17, S, 1 - (1ll << 56)},                 // next to +2^56 and -2^56
                                                              {-2147483647ll - 1, 2147483647, 1 - (1ll << 56), 3, -5, (1ll << 56) - 1},  // the limits: a negative sum under the shift
                                                              {-3 * S - 1, 1, 2 * S * cw + 5, -1, -2 * S - 3, 2 * S * rh + 1}};   // a half turn that reduces, odd sums
                                const long long* m = maps[map];
                                std::vector<uint32_t> stage((size_t)w * (y + rh));
                                for (size_t i = 0; i < stage.size(); ++i) stage[i] = values[((uint32_t)(i * 2654435761u + 12345u) >> 13) % 5u];
                                const uint64_t B = (uint64_t)ow * oh * och;
                                std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                                const uint64_t q = base + guard + a;
                                const long long rc2 = warp_vote_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, m, fill, och, weighted, q, base,
                                                                         out.data(), writes.data(), out.size());
                                if (rc2 < 0) { printf("bad access: och %u a %u flags %u map %d %ux%u: %lld\n", och, a, flags, map, cw, rh, rc2); return 1; }
                                const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                                if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                                long long want_loads = 0;
                                for (uint32_t Y = 0; Y < oh; ++Y)
                                    for (uint32_t X = 0; X < ow; ++X) {
                                        uint32_t v[17];                                  // the s * s sub-samples, then the centre
                                        long long n = 0;
                                        for (long long j = 0; j <= s; ++j)
                                            for (long long i = 0; i < s; ++i) {
                                                if (j == s && i > 0) break;
                                                const long long U = 2ll * X + 1, V = 2ll * Y + 1;
                                                const long long Us = s * U + 2 * i + 1 - s, Vs = s * V + 2 * j + 1 - s;
                                                const long long px = j == s ? m[0] * U + m[1] * V + m[2] : floor_div(m[0] * Us + m[1] * Vs, s) + m[2];
                                                const long long py = j == s ? m[3] * U + m[4] * V + m[5] : floor_div(m[3] * Us + m[4] * Vs, s) + m[5];
                                                const long long ik = index_ref(floor_div(px, 131072), cw, border), ir = index_ref(floor_div(py, 131072), rh, border);
                                                if (ir >= 0 && ik >= 0) { v[n++] = stage[(size_t)(y + ir) * w + x + ik]; ++want_loads; }
                                                else { v[n++] = fill; ++filled; }
                                            }
                                        const long long subs = s * s;
                                        const uint32_t centre = v[subs];
                                        long long top = 0, winners = 0;
                                        uint32_t low = 0;
                                        bool centre_wins = false;
                                        for (long long p = 0; p < subs; ++p) {
                                            long long count = 0;
                                            for (long long o = 0; o < subs; ++o) count += v[o] == v[p];
                                            if (count > top) top = count;
                                        }
                                        for (long long p = 0; p < subs; ++p) {
                                            long long count = 0, earlier = 0;
                                            for (long long o = 0; o < subs; ++o) { count += v[o] == v[p]; earlier += o < p && v[o] == v[p]; }
                                            if (count != top || earlier != 0) continue;     // (every winning value once)
                                            if (winners == 0 || key_ref(v[p]) < key_ref(low)) low = v[p];
                                            if (v[p] == centre) centre_wins = true;
                                            ++winners;
                                        }
                                        const uint32_t win = winners > 1 && centre_wins ? centre : low;
                                        if (winners == 1) ++unique; else if (centre_wins) ++by_centre; else ++by_key;
                                        for (uint32_t ch = 0; ch < och; ++ch)
                                            if (out[guard + a + ((size_t)Y * ow + X) * och + ch] != (uint8_t)(win >> (8 * ch))) {
                                                printf("wrong byte: och %u mode %d a %u flags %u map %d %ux%u at (%u, %u).%u\n", och, weighted, a, flags, map, cw, rh, X, Y, ch);
                                                return 1;
                                            }
                                    }
                                if (rc2 != want_loads) { printf("%lld loads, %lld samples inside: map %d flags %u\n", rc2, want_loads, map, flags); return 1; }
                                taken += want_loads;
                                ++items;
                            }
    if (taken == 0 || filled == 0 || unique == 0 || by_centre == 0 || by_key == 0) { printf("no sample taken, none filled, or a kind of decision that never arose\n"); return 1; }
    printf("warp_vote_host: %lld items ok\n", items);
    return 0;
}
#endif

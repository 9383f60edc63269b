// stats_host.cpp — the tile arithmetic of qoimi_pixel_stats (qoi_amd/csrc/qoi_stats_core.h) compiled for the host: the tile loop of stats_reduce,
// tile by tile and lane by lane, over a synthetic staging array and a memory functor that checks every load, so that
// tests/test_stats_core_host.py can compare it with the Python model without a GPU.  The lanes of a "workgroup" keep their shares over a range of
// tiles, as the kernel's lanes do between two flushes, and are then folded into 64-bit totals.  With -DSTATS_HOST_MAIN the same source is a
// stand-alone program that walks a grid of regions against a plain per-pixel loop (the test builds it with -fsanitize=address,undefined and
// runs it).  Not part of the library.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../qoi_amd/csrc/qoi_stats_core.h"

namespace {

struct HostMem {
    const uint32_t* stage; uint64_t stage_px;
    qoimi::StatsRect g;
    uint32_t* hist;                      // [4][256] or NULL
    long long* bad;                      // loads outside the array or outside the region
    uint32_t load(uint64_t i) const {
        const uint64_t r = i / g.w, c = i % g.w;
        if (i >= stage_px || r < g.y || r >= (uint64_t)g.y + g.ch || c < g.x || c >= (uint64_t)g.x + g.cw) { ++*bad; return 0u; }
        return stage[i];
    }
    void count(uint32_t px, bool on) const {
        if (on) for (uint32_t c = 0; c < 4u; ++c) ++hist[c * 256u + ((px >> (8u * c)) & 255u)];
    }
};

}  // namespace

extern "C" {

// One region as stats_reduce walks it when `per_wg` tiles go to a workgroup: the lanes keep their shares over that many tiles, then they are
// folded into *out (64-bit adds, minima, maxima), which the caller has set with stats_host_init.  hist: NULL or uint32[4][256], zeroed by the
// caller.  Returns the pixels walked, or -1 - the number of bad loads if there was one.  lane_sq_max: the largest square sum a lane held.
long long stats_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t flags,
                         uint32_t per_wg, qoimi::StatsAcc* out, uint32_t* hist, uint64_t* lane_sq_max) {
    long long bad = 0, walked = 0;
    const qoimi::StatsRect g = {w, x, y, cw, ch, flags};
    const HostMem mem = {stage, stage_px, g, hist, &bad};
    const uint64_t tiles = qoimi::stats_tiles(cw, ch), npx = (uint64_t)cw * ch;
    uint64_t sq_max = 0;
    static qoimi::StatsLane lanes[qoimi::kStatsThreads];
    for (uint64_t t0 = 0; t0 < tiles; t0 += per_wg) {
        for (uint32_t lane = 0; lane < qoimi::kStatsThreads; ++lane) qoimi::stats_clear(lanes[lane]);
        for (uint64_t t = t0; t < t0 + per_wg && t < tiles; ++t)
            for (uint32_t lane = 0; lane < qoimi::kStatsThreads; ++lane) {
                if (hist) qoimi::stats_tile<true>(mem, g, (uint32_t)t, lane, lanes[lane]);
                else qoimi::stats_tile<false>(mem, g, (uint32_t)t, lane, lanes[lane]);
                const uint64_t p0 = t * qoimi::kStatsTilePx + (uint64_t)lane * qoimi::kStatsLanePx;
                if (p0 < npx) walked += (long long)(npx - p0 < qoimi::kStatsLanePx ? npx - p0 : qoimi::kStatsLanePx);
            }
        for (uint32_t lane = 0; lane < qoimi::kStatsThreads; ++lane) {
            for (uint32_t k = 0; k < 4u; ++k) if (lanes[lane].sq[k] > sq_max) sq_max = lanes[lane].sq[k];
            qoimi::stats_fold(*out, lanes[lane]);
        }
    }
    out->first = mem.load(qoimi::stats_first_at(g));
    if (lane_sq_max) *lane_sq_max = sq_max;
    return bad ? -1 - bad : walked;
}

void stats_host_init(qoimi::StatsAcc* out) { qoimi::stats_init(*out); }
unsigned stats_host_flags(const qoimi::StatsAcc* a, uint64_t pixels) { return qoimi::stats_flags(*a, pixels); }
unsigned long long stats_host_tiles(uint32_t cw, uint32_t ch) { return qoimi::stats_tiles(cw, ch); }
unsigned stats_host_tile_px(void) { return qoimi::kStatsTilePx; }

}

#ifdef STATS_HOST_MAIN
#include <stdio.h>
#include <vector>

// Small widths and heights, regions around one tile, an interior rectangle and an all-white run through one workgroup, in a staging array of
// exactly the size the walk may touch: it ends with the region's last pixel.
int main() {
    struct Case { uint32_t w, x, y, cw, ch, per_wg; bool white; };
    const uint32_t T = qoimi::kStatsTilePx;
    const Case cases[] = {{1, 0, 0, 1, 1, 1, false}, {9, 3, 2, 5, 1, 1, false}, {9, 3, 2, 1, 7, 1, false}, {40, 1, 3, 37, 31, 1, false},
                          {T + 4, 2, 1, T - 1, 1, 1, false}, {T + 4, 2, 1, T, 1, 2, false}, {T + 4, 2, 1, T + 1, 1, 1, false},
                          {135, 1, 3, 129, 67, 3, false}, {300, 0, 0, 300, 260, 1000, true}};
    long long regions = 0;
    for (const Case& k : cases)
        for (uint32_t flags = 0; flags < 4; ++flags)
            for (int with_hist = 0; with_hist < 2; ++with_hist) {
                std::vector<uint32_t> stage((size_t)k.w * (k.y + k.ch - 1u) + k.x + k.cw);
                for (size_t i = 0; i < stage.size(); ++i) stage[i] = k.white ? 0xFFFFFFFFu : (uint32_t)(i * 2654435761u + 12345u);
                std::vector<uint32_t> hist(1024, 0u);
                qoimi::StatsAcc got;
                stats_host_init(&got);
                uint64_t sq_max = 0;
                const long long rc = stats_host_run(stage.data(), stage.size(), k.w, k.x, k.y, k.cw, k.ch, flags, k.per_wg, &got, with_hist ? hist.data() : nullptr, &sq_max);
                if (rc != (long long)k.cw * k.ch) { printf("bad load: %u x %u flags %u: %lld\n", k.cw, k.ch, flags, rc); return 1; }
                qoimi::StatsAcc want;
                stats_host_init(&want);
                std::vector<uint32_t> want_hist(1024, 0u);
                for (uint32_t r = 0; r < k.ch; ++r)
                    for (uint32_t c = 0; c < k.cw; ++c) {
                        const uint32_t px = stage[(size_t)(k.y + r) * k.w + k.x + c];
                        for (uint32_t q = 0; q < 4u; ++q) {
                            const uint32_t v = (px >> (8u * q)) & 255u;
                            want.sum[q] += v; want.sum_sq[q] += (uint64_t)v * v; ++want_hist[q * 256u + v];
                            if (v < want.mn[q]) want.mn[q] = v;
                            if (v > want.mx[q]) want.mx[q] = v;
                        }
                        want.opaque += (px >> 24) == 255u; want.transparent += (px >> 24) == 0u;
                        want.grey += (px & 255u) == ((px >> 8) & 255u) && ((px >> 8) & 255u) == ((px >> 16) & 255u);
                    }
                want.first = stage[(size_t)((flags & 2u) ? k.y + k.ch - 1u : k.y) * k.w + ((flags & 1u) ? k.x + k.cw - 1u : k.x)];
                if (memcmp(&got, &want, sizeof(got)) != 0) { printf("wrong result: %u x %u flags %u\n", k.cw, k.ch, flags); return 1; }
                if (with_hist && hist != want_hist) { printf("wrong histogram: %u x %u\n", k.cw, k.ch); return 1; }
                // 78 000 white pixels through ONE workgroup: its total passes 2^32 (at 66 052 pixels), no lane does
                if (k.white && (got.sum_sq[0] != 65025ull * k.cw * k.ch || got.sum_sq[0] <= 0xFFFFFFFFull || sq_max > 0xFFFFFFFFull ||
                                stats_host_flags(&got, (uint64_t)k.cw * k.ch) != (qoimi::kStatsConstant | qoimi::kStatsOpaque | qoimi::kStatsGrey))) {
                    printf("the white run: square sum %llu\n", (unsigned long long)got.sum_sq[0]);
                    return 1;
                }
                ++regions;
            }
    printf("stats_host: %lld regions ok\n", regions);
    return 0;
}
#endif

// qoi_stats.hip — qoimi_pixel_stats: per-region pixel statistics of a sub-batch of decoded images (stats_reduce).  gfx950, wave64.
// The host side: qoi_host_staged.hip (qoi_kernels.h holds the table and declares the launcher).
//
// The result (normative; qoi_amd/pixelstats.py: stats states it in Python, qoi_stats_core.h holds the arithmetic and the bounds): image i stands
// in the staging arena as w x rows pixels of 4 bytes; a region is a rectangle of it; per region: the sum and the sum of squares of every
// channel, minimum and maximum, how many pixels are opaque, transparent, grey, and - in the instantiation with a histogram - how often every
// value of every channel occurs.
//
//   stats_reduce  Work is cut over the REGION's pixels in row-major order: a TILE is kStatsTilePx consecutive pixels of ONE region, laid over the
//                 region table the host builds (an entry holds its region's first tile); a workgroup takes a contiguous range of tiles
//                 (qoi_dev.h: walk_tiles), so one launch serves every region of a sub-batch.  A lane takes four consecutive pixels: one
//                 division by the region's width, then it steps on; it reads them as aligned dwords - plain loads: regions may share pixels -
//                 and nothing outside the region.  A lane keeps four sums, four 64-bit sums of squares, minimum and maximum per channel and
//                 three counters (qoi_stats_core.h says why 32 bits hold the sums).  When the workgroup leaves a region (as cmp_flush
//                 of qoi_compare.hip does) the sums are added across the wavefront in 64 bits and the minima / maxima minimised / maximised with
//                 cross-lane operations, the four wavefronts meet in 19 x 4 words of LDS, and 19 lanes send one atomic each to the region's
//                 result: 64-bit adds (none for a zero), 32-bit minima and maxima.  All integer: the result is the same whatever order the
//                 workgroups finish in.  The lane that holds pixel 0 of tile 0 also stores `first`, the pixel the flipped region begins with.
//                 <true> keeps ONE histogram of 4 x 256 counters (4 KiB) per workgroup in LDS, updated with LDS atomics: a step at which
//                 all pixels of a wavefront are equal (flat content: 64 lanes on one counter) sends one add of the lane count per channel
//                 instead; on leaving a region the non-zero counters go to the region's device histogram with atomic adds and the LDS copy is
//                 cleared.  <false> holds the reduction words and no other LDS.
#include "qoi_dev.h"
#include "qoi_stats_core.h"

namespace qoimi {

constexpr uint32_t kStatsWords = kStatsSums + 8u;      // per wavefront: 11 sums, 4 minima, 4 maxima
constexpr uint32_t kStatsNone = 0xFFFFFFFFu;

template <bool HIST>
struct StatsMem {
    const uint32_t* src;
    uint32_t* bins;                                    // the workgroup's histogram in LDS (HIST)
    __device__ __forceinline__ uint32_t load(u64 i) const { return src[i]; }
    // every lane of the wavefront comes here together
    __device__ __forceinline__ void count(uint32_t px, bool on) const {
        const u64 mask = lanes_where(on);
        if (mask == 0ull) return;
        const uint32_t lead = read_lane_dyn(px, (uint32_t)__builtin_ctzll(mask));
        if (lanes_where(on && px != lead) == 0ull) {   // one value in the whole wavefront: one add per channel
            if (on && count_below(mask) == 0u) {
                const uint32_t k = (uint32_t)__builtin_popcountll(mask);
#pragma unroll
                for (uint32_t c = 0; c < 4u; ++c) atomicAdd(&bins[c * 256u + ((px >> (8u * c)) & 255u)], k);
            }
        } else if (on) {
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) atomicAdd(&bins[c * 256u + ((px >> (8u * c)) & 255u)], 1u);
        }
    }
};

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((unsigned long long)v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o); v = t > v ? t : v; }
    return v;
}

// The workgroup leaves a region (every thread calls): what its lanes hold goes to the region's result, the workgroup's histogram to the
// region's.
template <bool HIST>
__device__ __forceinline__ void stats_flush(const StatsLane& a, StatsAcc* res, unsigned* hist, u64 (*s_part)[kStatsWords], uint32_t* s_bins) {
    const uint32_t wave = threadIdx.x >> 6;
    u64 v[kStatsWords];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        v[k] = wave_sum_u64(a.sum[k]); v[4u + k] = wave_sum_u64(a.sq[k]);
        v[kStatsSums + k] = wave_min_u32(a.mn[k]); v[kStatsSums + 4u + k] = wave_max_u32(a.mx[k]);
    }
    v[8] = wave_sum_u64(a.opaque); v[9] = wave_sum_u64(a.transparent); v[10] = wave_sum_u64(a.grey);
    if (lane_id() == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < kStatsWords; ++k) s_part[wave][k] = v[k];
    }
    __syncthreads();                                              // (also: every LDS atomic of the histogram has landed)
    const uint32_t k = threadIdx.x;
    if (k < kStatsSums) {
        u64 total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kStatsThreads / 64u; ++w) total += s_part[w][k];
        if (total != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(res) + k, (unsigned long long)total);
    } else if (k < kStatsSums + 4u) {
        uint32_t lowest = 255u;
#pragma unroll
        for (uint32_t w = 0; w < kStatsThreads / 64u; ++w) lowest = (uint32_t)s_part[w][k] < lowest ? (uint32_t)s_part[w][k] : lowest;
        atomicMin(&res->mn[k - kStatsSums], lowest);
    } else if (k < kStatsWords) {
        uint32_t highest = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kStatsThreads / 64u; ++w) highest = (uint32_t)s_part[w][k] > highest ? (uint32_t)s_part[w][k] : highest;
        atomicMax(&res->mx[k - kStatsSums - 4u], highest);
    }
    if (HIST) {
#pragma unroll
        for (uint32_t b = threadIdx.x; b < kStatsBins; b += kStatsThreads) {
            const uint32_t n = s_bins[b];
            if (n != 0u) { atomicAdd(&hist[b], n); s_bins[b] = 0u; }
        }
    }
    __syncthreads();                                              // the words are rewritten at the next region
}

template <bool HIST>
__global__ __launch_bounds__(kStatsThreads) void stats_reduce(const uint8_t* __restrict__ stage, const StatsEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               StatsAcc* res, unsigned* hist) {
    __shared__ u64 s_part[kStatsThreads / 64u][kStatsWords];
    __shared__ uint32_t s_bins[HIST ? kStatsBins : 1u];
    if (HIST) {
#pragma unroll
        for (uint32_t b = threadIdx.x; b < kStatsBins; b += kStatsThreads) s_bins[b] = 0u;
        __syncthreads();
    }
    StatsLane a;
    stats_clear(a);
    uint32_t cur = kStatsNone;                                    // the region the lanes hold pixels of (the same in every thread)
    walk_tiles(tab, m, tiles, [&](const StatsEntry& e, uint32_t tile) {
        if (cur != kStatsNone && cur != e.index) {
            stats_flush<HIST>(a, &res[cur], HIST ? hist + (u64)cur * kStatsBins : nullptr, s_part, s_bins);
            stats_clear(a);
        }
        cur = e.index;
        const StatsRect g = {e.w, e.x, e.y, e.cw, e.ch, e.cfg};
        const StatsMem<HIST> mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off), s_bins};
        stats_tile<HIST>(mem, g, tile, threadIdx.x, a);
        if (tile == 0u && threadIdx.x == 0u) res[e.index].first = mem.load(stats_first_at(g));
    });
    if (cur != kStatsNone) stats_flush<HIST>(a, &res[cur], HIST ? hist + (u64)cur * kStatsBins : nullptr, s_part, s_bins);
}

void launch_stats(const uint8_t* stage, const StatsEntry* tab, uint32_t m, uint32_t tiles, StatsAcc* res, unsigned* hist, uint32_t grid, hipStream_t st) {
    if (hist) hipLaunchKernelGGL(stats_reduce<true>, dim3(grid), dim3(kStatsThreads), 0, st, stage, tab, m, tiles, res, hist);
    else hipLaunchKernelGGL(stats_reduce<false>, dim3(grid), dim3(kStatsThreads), 0, st, stage, tab, m, tiles, res, hist);
}

}  // namespace qoimi

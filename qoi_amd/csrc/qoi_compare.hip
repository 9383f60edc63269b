// qoi_compare.hip — qoimi_compare_images / qoimi_verify_images: are two sets of device images equal, pixel by pixel (cmp_pixels), and what
// stands at the first difference (cmp_first).  gfx950, wave64.  The host side: qoi_host_staged.hip (qoi_kernels.h holds the tables and declares the launcher).
//
// The comparison (normative; qoi_amd/imagediff.py: diff states it in Python): image i has npx pixels of ca bytes at a + a_off and of cb bytes at
// b + b_off, both tightly packed at any byte offset; two pixels are equal when their first min(ca, cb) bytes are.  Per image: how many pixels
// differ, and the lowest index of one that does.
//
//   cmp_pixels   Work is cut into TILES of kCmpTilePx pixels of ONE image over the image table the host builds (an entry holds its image's
//                first tile); a workgroup takes a contiguous range of tiles - one binary search, then it steps on from image to image - so one
//                launch serves every image of a call, a 4K frame and a 1 x 1 image alike.  A lane compares GROUPS of four pixels: 16 bytes of
//                a 4-channel side, 12 of a 3-channel one, consecutive lanes consecutive groups (a wavefront's load is one contiguous KiB or
//                768 bytes).  A group's bytes - at any alignment - are the aligned dwords that hold them, turned with v_alignbyte: four (three)
//                dwords, one more only where the side is not dword aligned - the dword that holds the group's last byte, never the one behind
//                it.  Only whole groups are loaded that way; the up to three pixels behind an image's last whole group go byte by byte, so no
//                load reaches beyond the aligned dwords that hold the image's first and last byte.  All four channel pairings take this path:
//                the pixels of a group are cut out of its dwords as 32-bit values (24 bits of a 3-channel side) and compared under a mask.
//                A lane keeps a count and its first differing index (its pixels ascend) per image; when the workgroup leaves an image the
//                counts are summed and the indices minimised over the wavefronts (cross-lane, then four words of LDS), and - only if something
//                differed - one 64-bit add and one 64-bit min go to the image's result.  Loads are non-temporal: every byte is read once.
//   cmp_first    a thread per image, behind cmp_pixels: reads pixel `first` of both sides and fills want / got / flags, which makes the
//                result a function of the inputs alone, whatever order the workgroups finished in.
#include "qoi_dev.h"

namespace qoimi {

// (kCmpThreads, kCmpSteps, kCmpGroupPx, kCmpTilePx and the table structs CmpImage / CmpDiff: qoi_kernels.h)
constexpr uint32_t kCmpNone = 0xFFFFFFFFu;

// A group of four CH-byte pixels at p (sh = address & 3) as CH dwords: the aligned dwords that hold its bytes and no other.
template <uint32_t CH>
__device__ __forceinline__ void cmp_load(const uint8_t* p, uint32_t sh, uint32_t (&w)[5]) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
#pragma unroll
    for (uint32_t k = 0; k < CH; ++k) w[k] = __builtin_nontemporal_load(&q[k]);
    w[CH] = sh ? __builtin_nontemporal_load(&q[CH]) : 0u;
}

// pixel j of a group whose bytes stand in d[0 .. CH): all 32 bits of a 4-byte pixel, the low 24 of a 3-byte one
template <uint32_t CH>
__device__ __forceinline__ uint32_t cmp_px(const uint32_t (&d)[4], uint32_t j) {
    if (CH == 4u) return d[j];
    return j == 0u ? d[0] & 0xFFFFFFu : j == 1u ? ((d[0] >> 24) | (d[1] << 8)) & 0xFFFFFFu : j == 2u ? ((d[1] >> 16) | (d[2] << 16)) & 0xFFFFFFu : d[2] >> 8;
}

// One tile of an image: pixels [px_base, px_base + kCmpTilePx) as far as the image has them.
template <uint32_t CA, uint32_t CB>
__device__ __forceinline__ void cmp_tile(const uint8_t* __restrict__ pa, const uint8_t* __restrict__ pb, uint32_t npx, uint32_t px_base,
                                         uint32_t& cnt, uint32_t& first) {
    constexpr uint32_t kMask = (CA == 4u && CB == 4u) ? 0xFFFFFFFFu : 0xFFFFFFu, kMin = CA < CB ? CA : CB;
    const uint32_t sa = (uint32_t)reinterpret_cast<uintptr_t>(pa) & 3u, sb = (uint32_t)reinterpret_cast<uintptr_t>(pb) & 3u;   // (a group begins a multiple of 4 bytes behind its image)
    uint32_t wa[kCmpSteps][5], wb[kCmpSteps][5];
#pragma unroll
    for (uint32_t s = 0; s < kCmpSteps; ++s) {
        const uint32_t px0 = px_base + (s * kCmpThreads + threadIdx.x) * kCmpGroupPx;
        if (px0 + kCmpGroupPx <= npx) {
            cmp_load<CA>(pa + (u64)px0 * CA, sa, wa[s]);
            cmp_load<CB>(pb + (u64)px0 * CB, sb, wb[s]);
        }
    }
#pragma unroll
    for (uint32_t s = 0; s < kCmpSteps; ++s) {
        const uint32_t px0 = px_base + (s * kCmpThreads + threadIdx.x) * kCmpGroupPx;
        if (px0 + kCmpGroupPx <= npx) {
            uint32_t da[4], db[4];
#pragma unroll
            for (uint32_t k = 0; k < CA; ++k) da[k] = __builtin_amdgcn_alignbyte(wa[s][k + 1u], wa[s][k], sa);
#pragma unroll
            for (uint32_t k = 0; k < CB; ++k) db[k] = __builtin_amdgcn_alignbyte(wb[s][k + 1u], wb[s][k], sb);
#pragma unroll
            for (uint32_t j = 0; j < kCmpGroupPx; ++j) {
                const bool differ = ((cmp_px<CA>(da, j) ^ cmp_px<CB>(db, j)) & kMask) != 0u;
                cnt += differ ? 1u : 0u;
                if (differ && first == kCmpNone) first = px0 + j;
            }
        } else if (px0 < npx) {                                   // the image's last pixels, fewer than a group: byte by byte
            for (uint32_t q = px0; q < npx; ++q) {
                bool differ = false;
#pragma unroll
                for (uint32_t ch = 0; ch < kMin; ++ch) differ |= pa[(u64)q * CA + ch] != pb[(u64)q * CB + ch];
                cnt += differ ? 1u : 0u;
                if (differ && first == kCmpNone) first = q;
            }
        }
    }
}

// The workgroup leaves an image (every thread calls): what its lanes found goes to the image's result - nothing, if nothing differed.
__device__ __forceinline__ void cmp_flush(uint32_t cnt, uint32_t first, CmpDiff* res, uint32_t* s_cnt, uint32_t* s_first) {
    const uint32_t wave = threadIdx.x >> 6;
    const bool any = lanes_where(cnt != 0u) != 0ull;
    const uint32_t c = any ? wave_sum(cnt) : 0u, f = any ? wave_min_u32(first) : kCmpNone;
    if (lane_id() == 0u) { s_cnt[wave] = c; s_first[wave] = f; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        u64 total = 0; uint32_t lowest = kCmpNone;
#pragma unroll
        for (uint32_t k = 0; k < kCmpThreads / 64u; ++k) { total += s_cnt[k]; lowest = s_first[k] < lowest ? s_first[k] : lowest; }
        if (total != 0ull) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&res->mismatched), (unsigned long long)total);
            atomicMin(reinterpret_cast<unsigned long long*>(&res->first), (unsigned long long)lowest);
        }
    }
    __syncthreads();                                              // the words are rewritten at the next image
}

__global__ __launch_bounds__(kCmpThreads) void cmp_pixels(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const CmpImage* __restrict__ tab,
                                                           uint32_t m, uint32_t tiles, CmpDiff* diffs) {
    __shared__ uint32_t s_cnt[kCmpThreads / 64u], s_first[kCmpThreads / 64u];
    const u64 per_wg = ((u64)tiles + gridDim.x - 1u) / gridDim.x;
    const u64 lo64 = (u64)blockIdx.x * per_wg, hi64 = lo64 + per_wg < (u64)tiles ? lo64 + per_wg : (u64)tiles;
    if (lo64 >= hi64) return;
    const uint32_t t_lo = (uint32_t)lo64, t_hi = (uint32_t)hi64;
    uint32_t i = 0;                                               // the image of tile t_lo: the last one whose first tile is not behind it
    for (uint32_t hi = m - 1u; i < hi;) {
        const uint32_t mid = i + (hi - i + 1u) / 2u;
        if (tab[mid].first_tile <= t_lo) i = mid; else hi = mid - 1u;
    }
    uint32_t cnt = 0, first = kCmpNone;
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        if (i + 1u < m && tab[i + 1u].first_tile <= t) {          // (every image has a tile: one step at most)
            cmp_flush(cnt, first, &diffs[tab[i].index], s_cnt, s_first);
            cnt = 0; first = kCmpNone; ++i;
        }
        const CmpImage im = tab[i];
        const uint32_t px_base = (t - im.first_tile) * kCmpTilePx, ca = im.chan & 255u, cb = (im.chan >> 8) & 255u;
        const uint8_t* pa = a + im.a_off;
        const uint8_t* pb = b + im.b_off;
        if (ca == 4u && cb == 4u) cmp_tile<4, 4>(pa, pb, im.npx, px_base, cnt, first);
        else if (ca == 3u && cb == 3u) cmp_tile<3, 3>(pa, pb, im.npx, px_base, cnt, first);
        else if (ca == 4u) cmp_tile<4, 3>(pa, pb, im.npx, px_base, cnt, first);
        else cmp_tile<3, 4>(pa, pb, im.npx, px_base, cnt, first);
    }
    cmp_flush(cnt, first, &diffs[tab[i].index], s_cnt, s_first);
}

// the pixel at p as r | g << 8 | b << 16 | a << 24; alpha reads 0xFF where the buffer does not hold it or the report leaves it out
__device__ __forceinline__ uint32_t cmp_read_pixel(const uint8_t* p, uint32_t ch, uint32_t reported) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((ch == 4u && reported == 4u ? (uint32_t)p[3] : 0xFFu) << 24);
}

__global__ __launch_bounds__(256) void cmp_first(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const CmpImage* __restrict__ tab, uint32_t m,
                                                  CmpDiff* diffs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const CmpImage im = tab[i];
    CmpDiff* d = &diffs[im.index];
    uint32_t want = 0, got = 0, flags = 0;
    if (d->mismatched != 0ull) {
        const u64 f = d->first;
        const uint32_t ca = im.chan & 255u, cb = (im.chan >> 8) & 255u;
        want = cmp_read_pixel(a + im.a_off + f * ca, ca, (im.chan >> 16) & 255u);
        got = cmp_read_pixel(b + im.b_off + f * cb, cb, im.chan >> 24);
        flags = 1u;                                               // QOIMI_DIFF_PIXELS
    }
    d->want = want; d->got = got; d->flags = flags; d->reserved = 0u;
}

void launch_compare(const uint8_t* a, const uint8_t* b, const CmpImage* tab, uint32_t m, uint32_t tiles, CmpDiff* diffs, uint32_t grid,
                    hipStream_t st, KernelTimer* tm) {
    tm->mark(kT_begin, st);
    hipLaunchKernelGGL(cmp_pixels, dim3(grid), dim3(kCmpThreads), 0, st, a, b, tab, m, tiles, diffs);
    tm->mark(kT_cmp_pixels, st);
    hipLaunchKernelGGL(cmp_first, dim3((m + 255u) / 256u), dim3(256), 0, st, a, b, tab, m, diffs);
    tm->mark(kT_cmp_first, st);
}

}  // namespace qoimi

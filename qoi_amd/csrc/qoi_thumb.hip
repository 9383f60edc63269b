// qoi_thumb.hip — qoimi_decode_thumbnails: the exact integer box reduction of a sub-batch of decoded images (thumb_reduce).  gfx950, wave64.
// The host side: qoi_host_staged.hip (qoi_kernels.h holds the table and declares the launcher).
//
// The reduction (normative; qoi_amd/thumbs.py: thumbnail states it in Python, qoi_thumb_core.h holds the arithmetic): image i stands in the
// staging arena as w x h pixels of 4 bytes (the decoder's output at 4 channels: a 256-aligned slot, every pixel an aligned dword); output
// pixel (X, Y) of its tw x th thumbnail is the rounded mean of the source block x in [X*f, min(w, X*f+f)), y in [Y*f, min(h, Y*f+f)) - plain, or
// with the colours weighted by alpha.  The thumbnail is written tightly packed, och = 3 or 4 bytes per pixel, at any byte offset.
//
//   thumb_reduce  Work is cut over the OUTPUT.  A block of f x f source pixels belongs to L = 1, 2, 4, 8 or 16 neighbouring lanes (L = 1 up to
//                 f = 4, then the power of two that leaves a lane at most four pixels of a block's row: 2 up to f = 8, 4 up to 16, 8 up to 32,
//                 16 up to 64); lane l of them takes columns [l*c, l*c + c) of the block, c = ceil(f / L) <= 4, in every row of the block.  An
//                 ITEM is one lane's share; item = (output pixel, row-major) * L + l, so consecutive lanes read consecutive addresses of a
//                 source row: 16 bytes each for f = 4, 8, 16, 32, 64 (one wavefront: one contiguous KiB per row), 8 for f = 2, c dwords for
//                 the others.  TILES of kThumbThreads items of ONE image are laid over the image table the host builds (an entry holds its
//                 image's first tile); a workgroup takes a contiguous range of tiles (qoi_dev.h: walk_tiles), so one launch serves every
//                 image of a sub-batch, a 4K frame and a 1 x 1 image alike.
//                 A lane walks down its columns row by row: one 16-byte load per row where the row pitch and the column are multiples of
//                 four pixels (then every row of the 256-aligned slot is 16-byte aligned there), 8-byte loads where both are even, dwords
//                 otherwise.  Loads are non-temporal: every staged byte is read once, by exactly one lane.  A lane sees at most 4 x 64 =
//                 256 pixels, so its channel sums are kept as two packed pairs of 16-bit fields (256 * 255 < 2^16); the alpha-weighted
//                 sums are 32-bit.  The L lanes of a block add their sums with log2(L) butterfly steps (L divides 64 and items are
//                 numbered so that a block's lanes are neighbours in one wavefront), the first of them divides (qoi_thumb_core.h) and
//                 stores the pixel: one dword where the thumbnail holds 4 bytes per pixel and the address is aligned, else 3 or 4 bytes.
//                 No LDS, no barrier, no atomics; not one byte outside a thumbnail is written.
#include "qoi_dev.h"
#include "qoi_thumb_core.h"

namespace qoimi {

typedef uint32_t thumb_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t thumb_u32x4 __attribute__((ext_vector_type(4)));

template <bool WEIGHTED>
__device__ __forceinline__ void thumb_acc(uint32_t px, uint32_t& rb, uint32_t& ga, uint32_t (&W)[3]) {
    rb += px & 0x00FF00FFu;
    ga += (px >> 8) & 0x00FF00FFu;
    if (WEIGHTED) {
        const uint32_t a = px >> 24;
        W[0] += (px & 255u) * a; W[1] += ((px >> 8) & 255u) * a; W[2] += ((px >> 16) & 255u) * a;
    }
}

// One tile of an image: items [item_base, item_base + kThumbThreads) as far as the image has them.
template <bool WEIGHTED>
__device__ __forceinline__ void thumb_tile(const uint32_t* __restrict__ src, uint8_t* __restrict__ dst, const ThumbImage& im, uint32_t item_base) {
    const uint32_t lg = im.cfg & 255u, c = (im.cfg >> 8) & 255u, och = (im.cfg >> 16) & 255u;
    const ThumbShare sh = thumb_share(item_base + threadIdx.x, im.w, im.h, im.tw, im.th, im.f, lg, c);
    const uint32_t o = sh.o, l = (item_base + threadIdx.x) & ((1u << lg) - 1u), cnt = sh.cnt;
    const bool valid = o < im.tw * im.th;                          // (a block's lanes are valid or not together)
    uint32_t rb = 0, ga = 0, W[3] = {0, 0, 0};
    if (valid) {
        const uint32_t w = im.w, x0 = sh.x0, n = sh.n, rows = sh.y1 - sh.y0;   // n <= 4 columns of this lane, rows <= 64
        const uint32_t* p = src + ((u64)sh.y0 * w + x0);
        if (n == 4u && ((w | x0) & 3u) == 0u) {                   // 16-byte aligned in every row
#pragma unroll 4
            for (uint32_t r = 0; r < rows; ++r, p += w) {
                const thumb_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const thumb_u32x4*>(p));
                thumb_acc<WEIGHTED>(v.x, rb, ga, W); thumb_acc<WEIGHTED>(v.y, rb, ga, W);
                thumb_acc<WEIGHTED>(v.z, rb, ga, W); thumb_acc<WEIGHTED>(v.w, rb, ga, W);
            }
        } else if ((n == 2u || n == 4u) && ((w | x0) & 1u) == 0u) {   // 8-byte aligned in every row
#pragma unroll 2
            for (uint32_t r = 0; r < rows; ++r, p += w) {
                const thumb_u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const thumb_u32x2*>(p));
                thumb_acc<WEIGHTED>(v.x, rb, ga, W); thumb_acc<WEIGHTED>(v.y, rb, ga, W);
                if (n == 4u) {
                    const thumb_u32x2 u = __builtin_nontemporal_load(reinterpret_cast<const thumb_u32x2*>(p + 2));
                    thumb_acc<WEIGHTED>(u.x, rb, ga, W); thumb_acc<WEIGHTED>(u.y, rb, ga, W);
                }
            }
        } else {
#pragma unroll 2
            for (uint32_t r = 0; r < rows; ++r, p += w) {
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k)
                    if (k < n) thumb_acc<WEIGHTED>(__builtin_nontemporal_load(&p[k]), rb, ga, W);
            }
        }
    }
    uint32_t S[4] = {rb & 0xFFFFu, ga & 0xFFFFu, rb >> 16, ga >> 16};
    for (uint32_t s = 1u; s < (1u << lg); s <<= 1) {              // (lg is the image's: the whole workgroup takes the same steps)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) S[k] += (uint32_t)__shfl_xor((int)S[k], (int)s);
        if (WEIGHTED) {
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) W[k] += (uint32_t)__shfl_xor((int)W[k], (int)s);
        }
    }
    if (valid && l == 0u) {
        const uint32_t px = thumb_pixel(S, W, cnt, WEIGHTED);
        uint8_t* q = dst + (u64)o * och;
        if (och == 4u && ((uint32_t)reinterpret_cast<uintptr_t>(q) & 3u) == 0u) *reinterpret_cast<uint32_t*>(q) = px;
        else {
            q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16);
            if (och == 4u) q[3] = (uint8_t)(px >> 24);
        }
    }
}

__global__ __launch_bounds__(kThumbThreads) void thumb_reduce(const uint8_t* __restrict__ stage, const ThumbImage* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               uint8_t* __restrict__ out) {
    walk_tiles(tab, m, tiles, [&](const ThumbImage& im, uint32_t tile) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(stage + im.src_off);
        const uint32_t item_base = tile * kThumbThreads;
        if (im.cfg >> 24) thumb_tile<true>(src, out + im.dst_off, im, item_base);
        else thumb_tile<false>(src, out + im.dst_off, im, item_base);
    });
}

void launch_thumb(const uint8_t* stage, const ThumbImage* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(thumb_reduce, dim3(grid), dim3(kThumbThreads), 0, st, stage, tab, m, tiles, out);
}

}  // namespace qoimi

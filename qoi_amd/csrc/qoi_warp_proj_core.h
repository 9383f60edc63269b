// qoi_warp_proj_core.h — the arithmetic of qoimi_decode_warped with QOIMI_WARP_PROJECTIVE: the scale of an item's denominator, the
// denominator of an output pixel, the exact quotient floor(N * 2^F / W) that is the pixel's position in the source rectangle, and the work
// item of the tile that serves items with and without the flag alike.  Everything behind the position - the taps of an axis, their weights,
// the clamp, the fold, the blends, the one sample of kWarpNearest, the rounding and the stores - is that of qoi_warp_core.h,
// qoi_warp_cubic_core.h and qoi_warp_border_core.h through their position-taking forms (warp_pixel_at, warp_nearest_at, warp_cubic_pixel_at,
// warp_border_pixel_at): shared, not restated.  Only the POSITION of an output pixel is new: P = N / W instead of P = N.
//
// The definition (normative; qoi_amd/warp.py states it in Python: positions).  kWarpProjective = 1 << 17 is a flag of the item; it goes with
// the fill or any one of the four borders and with the bilinear sampling, kWarpNearest or kWarpBicubic, never with kWarpSuper2, kWarpSuper4,
// kWarpVote2 or kWarpVote4.  With it the item's `reserved` holds g = (int16)(reserved & 0xFFFF) and h = (int16)(reserved >> 16), two's
// complement.  All arithmetic is integer, every division and shift floors.
//   L = the smallest integer >= 0 with 2^L >= max(ow, oh);  F = 14 + L          (14 .. 34)
//   U = 2X + 1, V = 2Y + 1;  Uc = U - ow, Vc = V - oh                           (doubled offsets from the output's centre: |Uc| < ow, |Vc| < oh)
//   Nx = a * U + b * V + c,  Ny = d * U + e * V + f                             (the positions of the affine warp)
//   W  = 2^F + g * Uc + h * Vc                                                  (the denominator: 1.0 at the centre of the output)
//   Px = floor(Nx * 2^F / W),  Py = floor(Ny * 2^F / W)
// From Px and Py on nothing changes.  The scale is sized by the item because W > 0 everywhere needs |gamma| * ow < 1 for the real
// coefficient gamma = g / 2^F per doubled pixel: the useful range of g is 1 / ow, and with F = 14 + L the 16 bits cover that range at every
// size.  With g = h = 0, W = 2^F and Px = Nx exactly: the item has the bytes of the same item without the flag.
// Limits (the host checks them per item behind all older checks, in this order): the flag with a SUPER or VOTE flag; |c| or |f| of 2^53 or
// more; 2^F - |g| * (ow - 1) - |h| * (oh - 1) < 2^(F - 3) - W is linear in (X, Y), so that is its exact minimum over the pixel grid
// (|Uc| <= ow - 1), and the limit keeps the denominator at or above 1/8 inside the output.
// Bounds.  |a * U|, |b * V| <= 2^31 * 2^21 = 2^52 and |c| < 2^53: |Nx| < 2^52 + 2^52 + 2^53 = 2^54.  |g| <= 2^15 and |Uc| < ow <= 2^L:
// |g * Uc| < 2^(15 + L) = 2 * 2^F, likewise h: 2^(F-3) <= W < 5 * 2^F < 2^37.  |Px| <= |Nx| * 2^F / 2^(F-3) = 8 * |Nx| < 2^57: the bound every
// path behind the position, the fold's quotient estimate included (|Px >> 17| < 2^40), already assumes.
//
// How the quotient is computed.  N * 2^F has up to 88 bits; a 128-bit division does not link on the device, and no 64-bit integer division
// is compiled either.  The quotient is brought down in stages with the scheme of warp_fold_position (qoi_warp_border_core.h): the head
// q0 = floor(N / W), r = N - q0 * W, then the F fractional bits in chunks of s <= 17 bits: t = r << s (r < W < 2^37, so t < 2^54),
// q = floor(t / W), r = t - q * W, P = (P << s) + q.  That is long division in base 2^s and exact: 0 <= r < W holds after every stage.  Each
// stage's floor(n / W) (warp_proj_divide) takes an ESTIMATE in double precision, q' = floor((double)n * (1.0 / (double)W)): the conversion
// of n (|n| < 2^54), the reciprocal (W is an exact double) and the product each round once, a relative error below 2^-51 of a quotient below
// 2^54 / 2^(F-3) <= 2^43 - less than 2^-8 before the floor, so q' is the true quotient or one beside it and n - q' * W lies in [-W, 2W); one
// conditional add or subtract finishes it.  |q' * W| < 2^54 + 2^37 fits 64 bits.  The result is exact for every accepted item: the double
// only chooses which multiple of W the 64-bit integer subtraction takes.  The reciprocal is one per output pixel, shared by both positions
// and all their stages (three stages a position at most: F <= 34 is two chunks).  F is the item's: uniform over a tile.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_warp_proj.hip) and - by tests/host/warp_proj_host.cpp only - for the host, where the functor checks and counts every
// access.
#pragma once
#include <stdint.h>

#include "qoi_warp_vote_core.h"

namespace qoimi {

constexpr uint32_t kWarpProjective = 1u << 17;                  // (32768 and 65536 are not flags)
constexpr int64_t kWarpProjMaxOffset = 1ll << 53;               // |c|, |f| of an item with the flag stay below it
constexpr uint32_t kWarpProjBase = 14, kWarpProjChunk = 17;     // F = kWarpProjBase + L; the fractional bits come down kWarpProjChunk at a time

// The perspective coefficients of an item: the two halves of qoimi_warp::reserved
struct WarpProj { int32_t g, h; };

QOIMI_RESIZE_HD WarpProj warp_proj_of(uint32_t reserved) { return {(int32_t)(int16_t)(reserved & 0xFFFFu), (int32_t)(int16_t)(reserved >> 16)}; }

// F of an ow x oh output (both at least 1 and below 2^20)
QOIMI_RESIZE_HD uint32_t warp_proj_bits(uint32_t ow, uint32_t oh) {
    const uint32_t m = ow > oh ? ow : oh;
    return kWarpProjBase + (m > 1u ? 32u - (uint32_t)__builtin_clz(m - 1u) : 0u);
}

// W of output pixel (X, Y)
QOIMI_RESIZE_HD int64_t warp_proj_denominator(const WarpProj& pj, uint32_t F, uint32_t ow, uint32_t oh, uint32_t X, uint32_t Y) {
    const int64_t Uc = (int64_t)(2ull * X + 1u) - (int64_t)ow, Vc = (int64_t)(2ull * Y + 1u) - (int64_t)oh;
    return ((int64_t)1 << F) + (int64_t)pj.g * Uc + (int64_t)pj.h * Vc;
}

// The least W over the pixels of the output: 2^F - |g| * (ow - 1) - |h| * (oh - 1)
QOIMI_RESIZE_HD int64_t warp_proj_least(const WarpProj& pj, uint32_t F, uint32_t ow, uint32_t oh) {
    const int64_t ag = pj.g < 0 ? -(int64_t)pj.g : (int64_t)pj.g, ah = pj.h < 0 ? -(int64_t)pj.h : (int64_t)pj.h;
    return ((int64_t)1 << F) - ag * (int64_t)(ow - 1u) - ah * (int64_t)(oh - 1u);
}

// floor(n / W), and n becomes n - floor(n / W) * W, for |n| < 2^54, 0 < W < 2^37, |n / W| <= 2^43; rw = 1.0 / (double)W
QOIMI_RESIZE_HD int64_t warp_proj_divide(int64_t& n, int64_t W, double rw) {
    int64_t q = (int64_t)__builtin_floor((double)n * rw);        // (the estimate: the quotient or one beside it)
    int64_t r = n - q * W;
    if (r < 0) { r += W; --q; }
    else if (r >= W) { r -= W; ++q; }
    n = r;
    return q;
}

// floor(N * 2^F / W) for |N| < 2^54, 2^(F-3) <= W < 2^37, F <= 34; rw = 1.0 / (double)W
QOIMI_RESIZE_HD int64_t warp_proj_position(int64_t N, int64_t W, uint32_t F, double rw) {
    int64_t r = N, P = warp_proj_divide(r, W, rw);
    for (uint32_t left = F; left != 0u;) {
        const uint32_t s = left < kWarpProjChunk ? left : kWarpProjChunk;
        r <<= s;                                                   // (0 <= r < W < 2^37: below 2^54)
        P = P * ((int64_t)1 << s) + warp_proj_divide(r, W, rw);    // (a product, not a shift: P may be negative)
        left -= s;
    }
    return P;
}

// ... with the reciprocal made here (the tests walk it; the work item makes one for both positions)
QOIMI_RESIZE_HD int64_t warp_proj_position(int64_t N, int64_t W, uint32_t F) { return warp_proj_position(N, W, F, 1.0 / (double)W); }

// Work item t of tile `tile` of the item: for an item with kWarpProjective both positions through warp_proj_position and the pixel by the
// item's border and sampling through the position-taking forms, warp_vote_work as it is - the whole older chain - for any other (the flags
// are the item's, so the branch is the tile's), handed to the sink, or nothing beyond an edge.
template <bool WEIGHTED, class Mem, class Sink>
QOIMI_RESIZE_HD void warp_proj_work(const Mem& mem, const WarpGeom& g, const WarpProj& pj, uint64_t q, uint32_t och, uint32_t tile, uint32_t t, const Sink& sink) {
    if ((g.flags & kWarpProjective) == 0u) { warp_vote_work<WEIGHTED>(mem, g, q, och, tile, t, sink); return; }
    uint32_t X, Y;
    if (!warp_place(tile, t, g.ow, g.oh, X, Y)) return;
    const uint32_t F = warp_proj_bits(g.ow, g.oh);
    const int64_t W = warp_proj_denominator(pj, F, g.ow, g.oh, X, Y);
    const double rw = 1.0 / (double)W;
    const int64_t Px = warp_proj_position(warp_position(g.a, g.b, g.c, X, Y), W, F, rw), Py = warp_proj_position(warp_position(g.d, g.e, g.f, X, Y), W, F, rw);
    uint32_t px;
    if ((g.flags & kWarpBorders) != 0u) px = warp_border_pixel_at<WEIGHTED>(mem, g, Px, Py);
    else if ((g.flags & kWarpBicubic) != 0u) px = warp_cubic_pixel_at<WEIGHTED>(mem, g, Px, Py);
    else px = (g.flags & kWarpNearest) != 0u ? warp_nearest_at(mem, g, Px, Py) : warp_pixel_at<WEIGHTED>(mem, g, Px, Py);
    sink(mem, g, q, och, X, Y, px);
}

}  // namespace qoimi

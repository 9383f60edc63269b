// qoi_warp_vote_core.h — the arithmetic of qoimi_decode_warped with QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4: the value of a nearest sub-sample,
// the majority vote over the s x s sub-samples of an output pixel, and the work item of the tile that serves items with and without such a
// flag alike.  The position of a sub-sample is that of qoi_warp_super_core.h (warp_super_position), the fold that of qoi_warp_border_core.h
// (warp_fold_of, warp_fold), the key and the word whose maximum wins those of qoi_mode_core.h (mode_key, mode_word, mode_pick), the place
// and the sinks those of qoi_warp_core.h and qoi_tensor_core.h: shared, not restated.  A majority vote, not an average and not a selection:
// for label maps (segmentation masks, instance ids, palette indices) under a REDUCING map, where kWarpNearest looks at one source pixel.
//
// The definition (normative; qoi_amd/warp.py states it in Python).  kWarpVote2: s = 2, L = 1; kWarpVote4: s = 4, L = 2; at most one of the
// two, a sampling of its own: never with kWarpNearest, kWarpBicubic, kWarpSuper2 or kWarpSuper4; with the fill or any one of the four borders.
// Output pixel (X, Y), U = 2X + 1, V = 2Y + 1.  For 0 <= i, j < s the sub-sample's position is that of the SUPER flags:
//   Us = s * U + 2i + 1 - s,   Vs = s * V + 2j + 1 - s
//   Px = ((a * Us + b * Vs) >> L) + c,   Py = ((d * Us + e * Vs) >> L) + f     (arithmetic shift: it floors; |Px|, |Py| < 2^57)
// Its value is that of kWarpNearest at (Px, Py): column k = Px >> 17, row r = Py >> 17, the 64-bit index tested before it is narrowed;
// inside the rectangle R[r][k], all four bytes as staged; outside it each index is clamped under kWarpReplicate, folded on its own under
// kWarpReflect / kWarpReflect101 / kWarpWrap, and without a border flag the value is the dword `fill` as given and nothing is read.
// Nothing outside the rectangle is ever read.
// A value votes as a whole dword.  The count of a value is the number of the s^2 sub-samples equal to it, the winners are the values with
// the largest count.  One winner is the output; of several the centre value if it is a winner, else the winner with the lowest key
// r << 24 | g << 16 | b << 8 | a.  The centre value is what kWarpNearest gives this output pixel with the same border or fill, from
// Px = a * U + b * V + c, Py = d * U + e * V + f; it does not vote.  There are no modes: PLAIN and ALPHA_WEIGHTED give the same bytes; the
// drop of alpha for och 3 is the sink's, after the vote.
// There is no adaptivity: s^2 + 1 samples are taken whether or not the map reduces.
//
// How it is computed.  A lane holds its s^2 sub-sample dwords and the centre value in registers: warp_vote_pixel is instantiated per L and
// its loops have constant trip counts, so that the held values are never indexed dynamically.  Sub-sample p counts the sub-samples equal
// to it by comparison (itself included: a count is at least 1) and forms mode_word(count, value == centre value, value); the largest word
// is the winner - the largest count, then the centre value, then the lowest key -, and equal words stand for equal values.
//
// Plain sequential code over a memory functor `Mem` (load(pixel index) -> dword, store1 / store4(address, value)), compiled for the device
// by hipcc (qoi_warp_vote.hip) and - by tests/host/warp_vote_host.cpp only - for the host, where the functor checks and counts every
// access.
#pragma once
#include <stdint.h>

#include "qoi_mode_core.h"
#include "qoi_warp_super_core.h"

namespace qoimi {

constexpr uint32_t kWarpVote2 = 8192, kWarpVote4 = 16384;      // (4096 is not a flag)
constexpr uint32_t kWarpVotes = kWarpVote2 | kWarpVote4;       // an item with one of them takes the paths of this file

// The walk of both axes under the item's border (looked at under a folding border only)
struct WarpVoteFolds { WarpFold x, y; };

// The value of the position (Px, Py): the one sample of kWarpNearest there with the item's border - one load, none where it takes the fill.
template <class Mem>
QOIMI_RESIZE_HD uint32_t warp_vote_value(const Mem& mem, const WarpGeom& g, const WarpVoteFolds& fo, int64_t Px, int64_t Py) {
    int64_t k = Px >> 17, r = Py >> 17;                           // (64-bit: the border test comes before the narrowing)
    if ((g.flags & kWarpBorders) != 0u) {
        k = (int64_t)warp_fold_index(warp_fold_position(k, fo.x.P), fo.x);
        r = (int64_t)warp_fold_index(warp_fold_position(r, fo.y.P), fo.y);
    } else if ((g.flags & kWarpReplicate) != 0u) {
        k = k < 0 ? 0 : (k < (int64_t)g.cw ? k : (int64_t)g.cw - 1);
        r = r < 0 ? 0 : (r < (int64_t)g.rh ? r : (int64_t)g.rh - 1);
    } else if (k < 0 || k >= (int64_t)g.cw || r < 0 || r >= (int64_t)g.rh) return g.fill;
    return mem.load((uint64_t)(g.y + (uint32_t)r) * g.w + g.x + (uint32_t)k);
}

// Output pixel (X, Y) of an item with the VOTE flag of s = 1 << L: its s x s sub-sample values and the centre value, the vote, the winner.
template <uint32_t L, class Mem>
QOIMI_RESIZE_HD uint32_t warp_vote_pixel(const Mem& mem, const WarpGeom& g, uint32_t X, uint32_t Y) {
    constexpr uint32_t s = 1u << L, n = s * s;
    const uint32_t border = g.flags & kWarpBorders;
    const WarpVoteFolds fo = {warp_fold_of(border, g.cw), warp_fold_of(border, g.rh)};
    uint32_t v[n];
    QOIMI_RESIZE_UNROLL
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t i = p & (s - 1u), j = p >> L;
        v[p] = warp_vote_value(mem, g, fo, warp_super_position(g.a, g.b, g.c, X, Y, i, j, L), warp_super_position(g.d, g.e, g.f, X, Y, i, j, L));
    }
    const uint32_t centre = warp_vote_value(mem, g, fo, warp_position(g.a, g.b, g.c, X, Y), warp_position(g.d, g.e, g.f, X, Y));
    uint64_t best = 0u;                                           // (below every real word: a count is at least 1)
    QOIMI_RESIZE_UNROLL
    for (uint32_t p = 0; p < n; ++p) {
        uint32_t count = 0u;
        QOIMI_RESIZE_UNROLL
        for (uint32_t o = 0; o < n; ++o) count += v[o] == v[p] ? 1u : 0u;
        const uint64_t wd = mode_word(count, v[p] == centre, v[p]);
        if (wd > best) best = wd;
    }
    return mode_pick(best);
}

// Work item t of tile `tile` of the item: warp_vote_pixel for an item with a VOTE flag, warp_super_work as it is for any other (the flags
// are the item's, so the branch is the tile's), handed to the sink, or nothing beyond an edge.
template <bool WEIGHTED, class Mem, class Sink>
QOIMI_RESIZE_HD void warp_vote_work(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t tile, uint32_t t, const Sink& sink) {
    if ((g.flags & kWarpVotes) == 0u) { warp_super_work<WEIGHTED>(mem, g, q, och, tile, t, sink); return; }
    uint32_t X, Y;
    if (!warp_place(tile, t, g.ow, g.oh, X, Y)) return;
    sink(mem, g, q, och, X, Y, (g.flags & kWarpVote4) != 0u ? warp_vote_pixel<2>(mem, g, X, Y) : warp_vote_pixel<1>(mem, g, X, Y));
}

}  // namespace qoimi

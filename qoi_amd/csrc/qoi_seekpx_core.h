// qoi_seekpx_core.h — the pixel fetch of both builds of the seek index (seekpx_last, seekpx_carry): which aligned dwords a lane reads for its
// pixels of a pixel buffer - the caller's (qoimi_seek_index_from_pixels), or the staging arena at 4 bytes per pixel (qoimi_build_seek_index:
// the ch == 4, 256-byte-aligned case) -, how they unpack, and which of a lane's pixels leave their position in the tile's table.
//
// The definition (normative; qoi_amd/seekindex.py: points_from_pixels).  An image of `ch` = 3 or 4 bytes per pixel stands tightly packed at ANY
// byte address; pixel i is the bytes [base + i * ch, + ch) as r | g << 8 | b << 16 | a << 24, a = 255 where ch == 3.  A lane of seekpx_last takes
// kSeekPxLane = 4 consecutive pixels, n <= 4 of them inside its interval: n * ch <= 16 bytes at the address addr, read as the 1 to 5 aligned
// dwords that hold one of those bytes - never a dword that holds none, so never one that holds no byte of the image - and turned with
// v_alignbyte (crop_align) by addr & 3 as BandMem::tail16 turns a tail's bytes.  seekpx_carry reads single pixels the same way (n = 1: one dword
// or two).  A pixel that equals its right neighbour in the same tile is left out of the table: the neighbour's position is larger, its slot the
// same.  Which pixels a lane has (seekpx_lane_span), whether its last has a neighbour (seekpx_next_ok) and what it leaves in the table
// (seekpx_lane_marks) stand here too: the kernel only loads, shuffles and takes the maxima.
//
// Plain sequential code over a memory functor `Mem` (load(aligned byte address) -> dword), compiled for the device by hipcc (qoi_seek.hip:
// real loads) and - by tests/host/seekpx_host.cpp only - for the host, where the functor checks every address, so the fetch is compared with
// the Python model on the CPU before it runs on a GPU.
#pragma once
#include <stdint.h>

#include "qoi_seek_core.h"   // kSeekTilePx; qoi_crop_core.h: crop_align, the low dword of {hi, lo} >> 8 * s

namespace qoimi {

constexpr uint32_t kSeekPxLane = 4;              // consecutive pixels of a lane
constexpr uint32_t kSeekPxThreads = kSeekTilePx / kSeekPxLane;   // lanes of a tile: the workgroup of seekpx_last
static_assert(kSeekPxThreads == 256u, "seekpx_last is launched with 256 threads");

QOIMI_CROP_HD uint32_t seekpx_slot(uint32_t px) {   // (3r + 5g + 7b + 11a) % 64: slot_of (qoi_dev.h)
    return ((px & 0xFFu) * 3u + ((px >> 8) & 0xFFu) * 5u + ((px >> 16) & 0xFFu) * 7u + (px >> 24) * 11u) & 63u;
}

// The aligned dwords that hold the bytes [addr, addr + nbytes), nbytes <= 16: 0 for none, else 1..5.
QOIMI_CROP_HD uint32_t seekpx_dwords(uint64_t addr, uint32_t nbytes) { return nbytes != 0u ? ((uint32_t)(addr & 3u) + nbytes + 3u) >> 2 : 0u; }

// px[0 .. n): the n <= 4 pixels of ch bytes at the byte address addr; px[n .. 4) is not defined.  Fully unrolled: the dwords are registers.
template <class Mem>
QOIMI_CROP_HD void seekpx_fetch(const Mem& mem, uint64_t addr, uint32_t n, uint32_t ch, uint32_t (&px)[kSeekPxLane]) {
    const uint32_t s = (uint32_t)(addr & 3u), nd = seekpx_dwords(addr, n * ch);
    const uint64_t a = addr - s;
    uint32_t w[5];
    QOIMI_CROP_UNROLL
    for (uint32_t k = 0; k < 5u; ++k) w[k] = k < nd ? mem.load(a + 4u * k) : 0u;
    const uint32_t b0 = crop_align(w[1], w[0], s), b1 = crop_align(w[2], w[1], s), b2 = crop_align(w[3], w[2], s), b3 = crop_align(w[4], w[3], s);
    if (ch == 4u) { px[0] = b0; px[1] = b1; px[2] = b2; px[3] = b3; }
    else {                                       // 12 bytes: pixel j is the bytes [3j, 3j + 3) of b0 b1 b2, alpha 255
        px[0] = b0 | 0xFF000000u; px[1] = crop_align(b1, b0, 3u) | 0xFF000000u;
        px[2] = crop_align(b2, b1, 2u) | 0xFF000000u; px[3] = (b2 >> 8) | 0xFF000000u;
    }
}

// The pixel of ch bytes at the byte address addr.
template <class Mem>
QOIMI_CROP_HD uint32_t seekpx_one(const Mem& mem, uint64_t addr, uint32_t ch) {
    uint32_t px[kSeekPxLane];
    seekpx_fetch(mem, addr, 1u, ch, px);
    return px[0];
}

// Whether pixel j < n of a lane leaves its position in the table: not if its right neighbour - pixel j + 1 of the lane, or `next`, the first
// pixel of the lane to the right, where next_ok says that there is one in this tile and this wavefront - holds the same value.
QOIMI_CROP_HD bool seekpx_keep(const uint32_t (&px)[kSeekPxLane], uint32_t n, uint32_t j, uint32_t next, bool next_ok) {
    const uint32_t right = j + 1u < kSeekPxLane ? px[j + 1u < kSeekPxLane ? j + 1u : 0u] : next;
    const bool has = j + 1u < kSeekPxLane ? j + 1u < n : next_ok;
    return !(has && right == px[j]);
}

// Lane tid of tile `sub` of an interval of ipx pixels: i, its first pixel's place in the interval, and n <= 4, how many of its pixels lie
// inside the interval (0: the lane has nothing to do).
QOIMI_CROP_HD void seekpx_lane_span(uint32_t sub, uint32_t tid, uint32_t ipx, uint32_t& i, uint32_t& n) {
    i = sub * kSeekTilePx + tid * kSeekPxLane;
    n = i < ipx ? (ipx - i < kSeekPxLane ? ipx - i : kSeekPxLane) : 0u;
}

// Whether the lane to the right (tid + 1) holds a pixel this lane's last one may be compared with: it is in the same wavefront - its first
// pixel comes by __shfl_down - and that pixel lies inside the interval.  (Then this lane is full: n == 4.)
QOIMI_CROP_HD bool seekpx_next_ok(uint32_t tid, uint32_t i, uint32_t ipx) { return (tid & 63u) < 63u && i + kSeekPxLane < ipx; }

// What a lane leaves in the tile's table: mark(slot, position + 1) for each of its n pixels that is kept.  at: the position of the lane's
// first pixel in the image (the interval's first pixel + i); next: px[0] of lane tid + 1.
template <class Mark>
QOIMI_CROP_HD void seekpx_lane_marks(const uint32_t (&px)[kSeekPxLane], uint32_t n, uint32_t next, bool next_ok, uint32_t at, const Mark& mark) {
    QOIMI_CROP_UNROLL
    for (uint32_t j = 0; j < kSeekPxLane; ++j)
        if (j < n && seekpx_keep(px, n, j, next, next_ok)) mark(seekpx_slot(px[j]), at + j + 1u);
}

}  // namespace qoimi

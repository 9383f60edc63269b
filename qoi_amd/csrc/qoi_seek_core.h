// qoi_seek_core.h — the arithmetic of the row seek index: the pixels and bytes of a chunk, the walk of one 64-byte piece of a stream that
// seek_locate runs, what stands in front of a band stream's tail (header, loads, pad run) and the items band_assemble writes a band stream in.
//
// The definition (normative; qoi_amd/seekindex.py states it in Python).  A seek point holds the decoder's state at a row boundary: byte_off
// and skip (where the byte-bounded chunk walk stands at pixel P, and how many pixels of the QOI_OP_RUN there lie in front of P), prev (pixel
// P - 1) and table (the last pixel in front of P per hash slot, else 0).  A band stream is: a 14-byte header; the LOADS - every table[s],
// s ascending, that is neither 0 nor prev, then prev, each as FF r g b a: n <= 64 chunks; pad_rows = max(1, ceil((n + skip) / w)); the PAD
// RUN of R = pad_rows * w - skip - n pixels, R / 62 bytes 0xFD and one byte 0xC0 | (R % 62 - 1) if R % 62 != 0; the TAIL, bytes of the
// original stream.  Header and loads (the HEAD, at most 334 bytes) are written by seek_write_head on the host; the kernel takes them from
// there, the pad run from two numbers and the tail from the stream.
//
// Plain sequential code, compiled for the device by hipcc (qoi_seek.hip) and - by tests/host/seek_host.cpp only - for the host, where it is
// compared with the Python model on the CPU before it runs on a GPU.
#pragma once
#include <stdint.h>

#include "qoi_crop_core.h"   // crop_items, crop_store: an output at any address in aligned 16-byte words, never a read-modify-write

#define QOIMI_SEEK_HD QOIMI_CROP_HD
#define QOIMI_SEEK_UNROLL QOIMI_CROP_UNROLL

namespace qoimi {

constexpr uint32_t kSeekMinIntervalPx = 128;     // interval_rows * width at least: n + skip <= 125, so pad_rows <= interval_rows
constexpr uint32_t kSeekMaxSkip = 61;
constexpr uint32_t kSeekMaxLoads = 64;            // a point of a stream has table[hash(prev)] == prev: 63 other slots and prev.  An index is the caller's
                                                 // data: seek_prefix_plan counts whatever it holds (up to 65), and whoever writes a head checks n first
constexpr uint32_t kSeekHeadMost = 14u + 5u * kSeekMaxLoads;
constexpr uint32_t kSeekHeadSlot = 336;          // bytes of a head in the table band_assemble reads (a multiple of 16)
constexpr uint32_t kSeekThreads = 256;           // items of a tile: the workgroup of band_assemble
constexpr uint32_t kSeekTilePx = 1024;           // pixels of a tile of seekpx_last: four per lane
constexpr uint32_t kSeekNoPos = 64;              // seek_piece_walk: the count never passed the target

struct SeekPoint { uint32_t byte_off, skip, prev, reserved, table[64]; };      // = qoimi_seek_point
static_assert(sizeof(SeekPoint) == 272, "qoimi_seek_point");

// pixels and bytes of the chunk whose tag byte is b (qoi.h:547-575)
QOIMI_SEEK_HD uint32_t seek_chunk_px(uint32_t b) { return (b < 0xFEu && (b >> 6) == 3u) ? (b & 63u) + 1u : 1u; }
QOIMI_SEEK_HD uint32_t seek_chunk_len(uint32_t b) { return b >= 0xFEu ? b - 0xFAu : ((b >> 6) == 2u ? 2u : 1u); }

// ceil(h / K) - 1 seek points, or -1 if K == 0 or K * w < 128
QOIMI_SEEK_HD int64_t seek_point_count(uint32_t w, uint32_t h, uint32_t K) {
    if (K == 0u || (uint64_t)K * w < kSeekMinIntervalPx) return -1;
    return (int64_t)(((uint64_t)h + K - 1u) / K) - 1;
}

// tiles of kSeekTilePx pixels per interval of ipx pixels (ipx below 400 000 000: an interval in front of a point lies inside the image)
QOIMI_SEEK_HD uint32_t seek_interval_tiles(uint32_t ipx) { return (ipx + kSeekTilePx - 1u) / kSeekTilePx; }

// The walk of one piece - plen <= 64 bytes as 16 dwords - that is entered with its first chunk at byte p (0..4: the chunk in front reaches
// that far in).  A chunk's pixels belong to the piece its tag byte is in.  Returns the pixels of the piece's chunks; pos and before: the byte
// of the first chunk at which the count passes `target` (before + pixels of that chunk > target) and the count in front of it, kSeekNoPos
// if there is none.  Fully unrolled: the dwords are registers.
QOIMI_SEEK_HD uint32_t seek_piece_walk(const uint32_t (&d)[16], uint32_t plen, uint32_t p, uint32_t target, uint32_t& pos, uint32_t& before) {
    uint32_t px = 0;
    pos = kSeekNoPos; before = 0u;
    QOIMI_SEEK_UNROLL
    for (uint32_t at = 0; at < 64u; ++at) {
        const uint32_t b = (d[at >> 2] >> (8u * (at & 3u))) & 0xFFu;
        if (p == at && at < plen) {
            const uint32_t n = seek_chunk_px(b);
            if (pos == kSeekNoPos && px + n > target) { pos = at; before = px; }
            px += n;
            p = at + seek_chunk_len(b);
        }
    }
    return px;
}

// What stands in front of a band stream's tail.  head_len: header and loads; run_full bytes 0xFD; run_last: the last byte of the pad run, 0: none.
struct SeekPrefix { uint32_t n, pad_rows, head_len, run_full, run_last; };
QOIMI_SEEK_HD uint32_t seek_prefix_len(const SeekPrefix& f) { return f.head_len + f.run_full + (f.run_last != 0u ? 1u : 0u); }

// e: the point the band starts at, nullptr: row 0 (no loads, no pad rows)
QOIMI_SEEK_HD SeekPrefix seek_prefix_plan(const SeekPoint* e, uint32_t w) {
    SeekPrefix f = {0u, 0u, 14u, 0u, 0u};
    if (!e) return f;
    f.n = 1u;
    for (uint32_t s = 0; s < 64u; ++s) f.n += (e->table[s] != 0u && e->table[s] != e->prev) ? 1u : 0u;
    f.pad_rows = (f.n + e->skip + w - 1u) / w;
    if (f.pad_rows == 0u) f.pad_rows = 1u;
    const uint32_t R = (uint32_t)((uint64_t)f.pad_rows * w - e->skip - f.n);
    f.head_len = 14u + 5u * f.n; f.run_full = R / 62u; f.run_last = R % 62u != 0u ? (0xC0u | (R % 62u - 1u)) : 0u;
    return f;
}

// header and loads of the band stream into out[0 .. head_len): height = pad_rows + rows of the band.  For points with
// seek_prefix_plan(e, w).n <= kSeekMaxLoads only: then head_len <= kSeekHeadMost.
QOIMI_SEEK_HD void seek_write_head(const SeekPoint* e, uint32_t w, uint32_t height, uint32_t channels, uint32_t colorspace, uint8_t* out) {
    out[0] = 'q'; out[1] = 'o'; out[2] = 'i'; out[3] = 'f';
    for (uint32_t k = 0; k < 4u; ++k) { out[4u + k] = (uint8_t)(w >> (24u - 8u * k)); out[8u + k] = (uint8_t)(height >> (24u - 8u * k)); }
    out[12] = (uint8_t)channels; out[13] = (uint8_t)colorspace;
    if (!e) return;
    uint8_t* at = out + 14;
    for (uint32_t s = 0; s <= 64u; ++s) {
        const uint32_t v = s < 64u ? e->table[s] : e->prev;
        if (s < 64u && (v == 0u || v == e->prev)) continue;
        at[0] = 0xFFu; at[1] = (uint8_t)v; at[2] = (uint8_t)(v >> 8); at[3] = (uint8_t)(v >> 16); at[4] = (uint8_t)(v >> 24);
        at += 5;
    }
}

// A band stream of B bytes at the address q, written in the items of a crop's output (qoi_crop_core.h): item k is the aligned 16-byte word k
// that [q, q + B) touches.  Byte i of the band stream: i < head_len: mem.head(i); i < prefix_len: of the pad run; else byte i - prefix_len of
// the tail.  A word wholly inside the tail is mem.tail16 (its 16 source bytes at any alignment) and one 16-byte store; every other word is put
// together byte by byte and written with the stores of crop_store - whole if it lies wholly inside the band stream, else the band stream's
// own bytes in naturally aligned pieces.  Mem: head(i), tail1(i), tail16(i, W), store1 / store2 / store4 / store16(address, ...).
template <class Mem>
QOIMI_SEEK_HD void seek_band_item(const Mem& mem, const SeekPrefix& f, uint64_t q, uint32_t B, uint32_t k) {
    const int64_t lo = (int64_t)16 * (int64_t)k - (int64_t)(q & 15u);
    const uint32_t b0 = lo < 0 ? 0u : (uint32_t)lo;
    const uint32_t b1 = lo + 16 < (int64_t)B ? (uint32_t)(lo + 16) : B;
    const uint32_t prefix = seek_prefix_len(f);
    uint32_t W[4] = {0u, 0u, 0u, 0u};
    if (b0 >= prefix && b1 - b0 == 16u) mem.tail16(b0 - prefix, W);
    else {
        QOIMI_SEEK_UNROLL
        for (uint32_t t = 0; t < 16u; ++t) {
            const uint32_t i = b0 + t;
            if (i < b1) {
                const uint32_t v = i < f.head_len ? mem.head(i) : i < f.head_len + f.run_full ? 0xFDu : i < prefix ? f.run_last : mem.tail1(i - prefix);
                W[t >> 2] |= (v & 0xFFu) << (8u * (t & 3u));
            }
        }
    }
    crop_store(mem, q + b0, b1 - b0, W);
}

}  // namespace qoimi

// seekpx_host.cpp — the pixel fetch of qoimi_seek_index_from_pixels (qoi_amd/csrc/qoi_seekpx_core.h) compiled for the host: the tiles of
// seekpx_last lane by lane as the kernel walks them and the single-pixel reads of seekpx_carry, over a memory functor that checks every
// address - an aligned dword that holds no byte of the image is counted as bad - so that tests/test_seekpx_core_host.py can compare both with
// the Python model (qoi_amd/seekindex.py) without a GPU.  With -DSEEKPX_HOST_MAIN the same source is a stand-alone program that runs the same
// walk with plain loads over heap buffers of exactly the aligned dwords that hold the image and compares it with a sequential reader (the test
// builds it with -fsanitize=address,undefined and runs it: a dword read beyond the image is reported).  Not part of the library.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../qoi_amd/csrc/qoi_seek_core.h"
#include "../../qoi_amd/csrc/qoi_seekpx_core.h"

namespace {

constexpr uint32_t kThreads = qoimi::kSeekPxThreads;                     // the workgroup of seekpx_last

// buf[0 .. len) stands at the addresses [lo, lo + len); lo is a multiple of 4
struct CheckedMem {
    const uint8_t* buf; uint64_t lo, len;
    long long* bad; long long* loads;
    uint32_t load(uint64_t a) const {
        ++*loads;
        if (a % 4u != 0u || a < lo || a + 4u > lo + len) { ++*bad; return 0u; }
        uint32_t v;
        memcpy(&v, buf + (a - lo), 4);
        return v;
    }
};

// real addresses, nothing checked here: the sanitizer does it
struct RawMem {
    uint32_t load(uint64_t a) const {
        uint32_t v;
        memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), 4);
        return v;
    }
};

// One tile of seekpx_last, in the kernel's steps (span, fetch, the neighbour lane's first pixel, marks - all of qoi_seekpx_core.h): interval
// iv of ipx pixels of an image of ch bytes per pixel at the address base, tile `sub` of the interval.  last[64]: the interval's words (maxima
// of position + 1); seen[p]: pixel p as the lanes unpacked it (may be nullptr).
template <class Mem>
void tile_last(const Mem& mem, uint64_t base, uint32_t ch, uint32_t ipx, uint32_t iv, uint32_t sub, uint32_t* last, uint32_t* seen) {
    static uint32_t px[kThreads + 1u][qoimi::kSeekPxLane];
    const uint32_t p0 = iv * ipx;
    uint32_t i, n;
    for (uint32_t tid = 0; tid < kThreads; ++tid) {
        qoimi::seekpx_lane_span(sub, tid, ipx, i, n);
        qoimi::seekpx_fetch(mem, base + (uint64_t)(p0 + i) * ch, n, ch, px[tid]);
        for (uint32_t j = 0; seen && j < n; ++j) seen[p0 + i + j] = px[tid][j];
    }
    for (uint32_t tid = 0; tid < kThreads; ++tid) {
        qoimi::seekpx_lane_span(sub, tid, ipx, i, n);
        // __shfl_down(px[0], 1); lane 63 of a wavefront gets no lane's value - here the one that would do most harm, its own last pixel's
        const uint32_t next = (tid & 63u) < 63u ? px[tid + 1u][0] : px[tid][qoimi::kSeekPxLane - 1u];
        qoimi::seekpx_lane_marks(px[tid], n, next, qoimi::seekpx_next_ok(tid, i, ipx), p0 + i,
                                 [&](uint32_t slot, uint32_t pos1) { if (pos1 > last[slot]) last[slot] = pos1; });
    }
}

// seekpx_last over np intervals, then seekpx_carry: prev[np], table[np][64]
template <class Mem>
void all_points(const Mem& mem, uint64_t base, uint32_t ch, uint32_t ipx, uint32_t np, uint32_t* last, uint32_t* seen, uint32_t* prev, uint32_t* table) {
    const uint32_t tpi = (ipx + qoimi::kSeekTilePx - 1u) / qoimi::kSeekTilePx;
    for (uint32_t iv = 0; iv < np; ++iv)
        for (uint32_t sub = 0; sub < tpi; ++sub) tile_last(mem, base, ch, ipx, iv, sub, last + 64u * iv, seen);
    uint32_t cur[64] = {0};
    for (uint32_t j = 0; j < np; ++j) {
        for (uint32_t s = 0; s < 64u; ++s) {
            if (last[64u * j + s] != 0u) cur[s] = last[64u * j + s];
            table[64u * j + s] = cur[s] != 0u ? qoimi::seekpx_one(mem, base + (uint64_t)(cur[s] - 1u) * ch, ch) : 0u;
        }
        prev[j] = qoimi::seekpx_one(mem, base + ((uint64_t)(j + 1u) * ipx - 1u) * ch, ch);
    }
}

}  // namespace

extern "C" {

// An image of np * ipx pixels of ch bytes at buf + align (align 0..3); buf[0 .. len) are the aligned dwords that hold it.  last[np][64] zeroed
// by the caller; seen[np * ipx], prev[np], table[np][64] are written.  Returns the dword loads made, or -1 - the number of bad ones.
long long seekpx_host_points(const uint8_t* buf, uint64_t len, uint32_t align, uint32_t ch, uint32_t ipx, uint32_t np, uint32_t* last, uint32_t* seen,
                             uint32_t* prev, uint32_t* table) {
    long long bad = 0, loads = 0;
    const uint64_t lo = 0x40000u;
    const CheckedMem mem = {buf, lo, len, &bad, &loads};
    all_points(mem, lo + align, ch, ipx, np, last, seen, prev, table);
    return bad ? -1 - bad : loads;
}

unsigned seekpx_host_dwords(uint64_t addr, uint32_t nbytes) { return qoimi::seekpx_dwords(addr, nbytes); }

}

#ifdef SEEKPX_HOST_MAIN
#include <stdio.h>
#include <vector>

int main() {
    long long tiles = 0;
    for (uint32_t ch : {3u, 4u})
        for (uint32_t align = 0; align < 4u; ++align)
            for (uint32_t ipx : {1u, 3u, 255u, 256u, 1023u, 1024u, 1025u, 2064u})
                for (uint32_t np : {1u, 3u}) {
                    const uint32_t npx = np * ipx;
                    const size_t nbytes = (size_t)npx * ch, ndw = (align + nbytes + 3u) / 4u;
                    std::vector<uint32_t> heap(ndw);                          // exactly the aligned dwords that hold the image
                    uint8_t* img = reinterpret_cast<uint8_t*>(heap.data()) + align;
                    memset(heap.data(), 0xEE, ndw * 4u);
                    uint32_t x = 12345u + ipx * 7u + align + ch;
                    for (uint32_t p = 0; p < npx; ++p) {                      // a few colours, short runs: equal neighbours at every lane edge
                        if (p % 5u != 1u && p % 67u != 0u) x = x * 1664525u + 1013904223u;
                        const uint32_t v = (x >> 9) % 7u;
                        for (uint32_t k = 0; k < ch; ++k) img[(size_t)p * ch + k] = (uint8_t)(v * 37u + k * 11u + (p < 9u ? p : 0u));
                    }
                    // the plain reader
                    std::vector<uint32_t> want(npx), want_table((size_t)np * 64u), want_prev(np);
                    uint32_t cur[64] = {0};
                    for (uint32_t p = 0; p < npx; ++p) {
                        const uint8_t* q = img + (size_t)p * ch;
                        want[p] = q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((ch == 4u ? (uint32_t)q[3] : 255u) << 24);
                        cur[qoimi::seekpx_slot(want[p])] = want[p];
                        if ((p + 1u) % ipx == 0u) {
                            memcpy(&want_table[(size_t)(p / ipx) * 64u], cur, sizeof(cur));
                            want_prev[p / ipx] = want[p];
                        }
                    }
                    std::vector<uint32_t> last((size_t)np * 64u, 0u), seen(npx, 0x5A5A5A5Au), prev(np), table((size_t)np * 64u);
                    all_points(RawMem(), (uint64_t)reinterpret_cast<uintptr_t>(img), ch, ipx, np, last.data(), seen.data(), prev.data(), table.data());
                    if (seen != want || prev != want_prev || table != want_table) {
                        printf("differs: ch %u align %u ipx %u np %u\n", ch, align, ipx, np);
                        return 1;
                    }
                    tiles += (long long)np * ((ipx + qoimi::kSeekTilePx - 1u) / qoimi::kSeekTilePx);
                }
    printf("seekpx_host: %lld tiles ok\n", tiles);
    return 0;
}
#endif

// host_mem.h — the memory functors the host harnesses of this directory hand to a core in place of the kernel's, and what their stand-alone
// programs share.  A new core's harness starts here: pick StagedMem or RectMem, walk the core tile by tile, return checked(bad, loads).
// Addresses are virtual: `base` (a multiple of 16) stands for out[0], so the test chooses every alignment of q.  Every access outside an
// array (or the rectangle) or not naturally aligned is counted in *bad and dropped; writes[i] counts the stores to out[i].  Header-only,
// plain C++17; not part of the library.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace hostmem {

// The store half.  A member left out of the braces is null: *stores is counted only where a harness reports it.
struct StoreMem {
    uint8_t* out; uint8_t* writes; uint64_t out_len, base;
    long long* bad;
    long long* stores;
    void put(uint64_t a, uint32_t v, uint32_t bytes) const {
        if (stores) ++*stores;
        if (a % bytes != 0u || a < base || a - base + bytes > out_len) { ++*bad; return; }
        for (uint32_t k = 0; k < bytes; ++k) { out[a - base + k] = (uint8_t)(v >> (8u * k)); ++writes[a - base + k]; }
    }
    void store1(uint64_t a, uint32_t v) const { put(a, v, 1u); }
    void store2(uint64_t a, uint32_t v) const { put(a, v, 2u); }
    void store4(uint64_t a, uint32_t v) const { put(a, v, 4u); }
    void store16(uint64_t a, const uint32_t (&W)[4]) const {
        if (a % 16u != 0u) { ++*bad; return; }
        for (uint32_t k = 0; k < 4u; ++k) put(a + 4u * k, W[k], 4u);
    }
};

// Loads bounded by the staged array, which the tests end with the item's last row (the crop, resize, bilinear, bicubic and Lanczos
// harnesses; the weaker of the two checks: RectMem below also takes a load beside the rectangle as bad).
// {{out, writes, out_len, base, &bad}, stage, stage_px, &loads}
struct StagedMem : StoreMem {
    const uint32_t* stage; uint64_t stage_px;
    long long* loads;
    uint32_t load(uint64_t i) const {
        ++*loads;
        if (i >= stage_px) { ++*bad; return 0u; }
        return stage[i];
    }
};

// Loads bounded by the item's rectangle x, y, cw, rh in rows of w: a load of any other staged pixel is bad (the warp, nearest and mode
// harnesses).  A new harness takes this one unless its core may read beside the rectangle.
// {{out, writes, out_len, base, &bad}, stage, stage_px, w, x, y, cw, rh, &loads}
struct RectMem : StoreMem {
    const uint32_t* stage; uint64_t stage_px;
    uint32_t w, x, y, cw, rh;
    long long* loads;
    uint32_t load(uint64_t i) const {
        ++*loads;
        const uint64_t r = i / w, k = i % w;
        if (i >= stage_px || r < y || r >= (uint64_t)y + rh || k < x || k >= (uint64_t)x + cw) { ++*bad; return 0u; }
        return stage[i];
    }
};

// Single output pixels of geometries no array can hold: the staged pixel at index i is synth(i); loads from stage_px on are counted as bad.
// One store4 lands in *px.
struct SynthMem {
    uint64_t stage_px; uint32_t* px; long long* bad; long long* loads; long long* stores;
    static uint32_t synth(uint64_t i) {
        uint64_t z = (i + 1u) * 0x9E3779B97F4A7C15ull;
        z ^= z >> 29;
        return (uint32_t)(z >> 16);
    }
    uint32_t load(uint64_t i) const {
        ++*loads;
        if (i >= stage_px) { ++*bad; return 0u; }
        return synth(i);
    }
    void store1(uint64_t, uint32_t) const { ++*bad; }
    void store2(uint64_t, uint32_t) const { ++*bad; }
    void store4(uint64_t a, uint32_t v) const { ++*stores; if (a % 4u != 0u) ++*bad; *px = v; }
};

// What a _run returns: the count, or -1 - the number of bad accesses if there was one.
inline long long checked(long long bad, long long count) { return bad ? -1 - bad : count; }

// ---- for the stand-alone programs ----

const uint8_t kGuard = 0xA5;

// A staged image and the rectangle and output size of an item in it.
struct Case { uint32_t w, h, x, y, cw, rh, ow, oh; };

// out and writes hold lo guard bytes, B output bytes and guard bytes to the end.  The first index whose byte is outside and
// written or no longer kGuard, or inside and not written exactly once; -1 if there is none.
inline long long first_miswritten(const std::vector<uint8_t>& out, const std::vector<uint8_t>& writes, size_t lo, size_t B) {
    for (size_t i = 0; i < out.size(); ++i) {
        const bool inside = i >= lo && i < lo + B;
        if (writes[i] != (inside ? 1 : 0) || (!inside && out[i] != kGuard)) return (long long)i;
    }
    return -1;
}

// The element that holds channel ch of n at (X, Y) of the unflipped ow x oh result: planar when chw, else interleaved; flags & 1 mirrors
// x, flags & 2 mirrors y.
inline size_t element_index(bool chw, uint32_t flags, uint32_t ow, uint32_t oh, uint32_t n, uint32_t X, uint32_t Y, uint32_t ch) {
    const uint32_t xo = (flags & 1u) ? ow - 1u - X : X, yo = (flags & 2u) ? oh - 1u - Y : Y;
    return chw ? ((size_t)ch * oh + yo) * ow + xo : ((size_t)yo * ow + xo) * n + ch;
}

}  // namespace hostmem

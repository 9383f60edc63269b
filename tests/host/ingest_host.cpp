// ingest_host.cpp — the item arithmetic of qoimi_encode_tiles over tensor sources (qoi_amd/csrc/qoi_ingest_core.h) compiled for the host, so
// that tests/test_ingest_core_host.py can compare every item of every tile with the Python model without a GPU.  Not part of the library.
// With -DINGEST_HOST_MAIN it is a stand-alone program (built with -fsanitize=address,undefined by the same test and run directly): the same
// walk against a plain double loop in this file.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../qoi_amd/csrc/qoi_ingest_core.h"

namespace {

// The kernel's memory with every address checked.  A load of a float image is one or more whole elements: aligned to its own size and
// inside the image.  A 4-byte load of a u8 image is aligned and holds at least one byte of the image; no other load of it is allowed.  A
// store is aligned dwords inside the slot.  Every access is counted by its kind in n[]; with touch == false the addresses are virtual: they
// are checked and counted, loads give 0 and stores are dropped (ingest_host_paths).
enum { kLoad2, kLoad4, kLoad8, kLoad16, kStore4, kStore12, kStore16, kKinds };
struct HostMem {
    uint64_t img_lo, img_hi, out_lo, out_hi;
    uint32_t elem;
    bool touch = true;
    mutable int bad = 0;
    mutable uint64_t n[kKinds] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    bool inside(uint64_t a, uint32_t n) const { return elem != 1u && n >= elem && (a % n) == 0u && a >= img_lo && a + n <= img_hi; }
    uint32_t load2(uint64_t a) const {
        ++n[kLoad2];
        if (!inside(a, 2u)) { bad |= 1; return 0u; }
        if (!touch) return 0u;
        uint16_t v; memcpy(&v, (const void*)(uintptr_t)a, 2); return v;
    }
    uint32_t load4(uint64_t a) const {
        ++n[kLoad4];
        if (elem == 1u ? ((a & 3u) != 0u || a + 4u <= img_lo || a >= img_hi) : !inside(a, 4u)) { bad |= 1; return 0u; }
        if (!touch) return 0u;
        uint32_t v; memcpy(&v, (const void*)(uintptr_t)a, 4); return v;
    }
    void load8(uint64_t a, uint32_t (&W)[2]) const {
        ++n[kLoad8];
        W[0] = W[1] = 0u;
        if (!inside(a, 8u)) { bad |= 2; return; }
        if (touch) memcpy(W, (const void*)(uintptr_t)a, 8);
    }
    void load16(uint64_t a, uint32_t (&W)[4]) const {
        ++n[kLoad16];
        W[0] = W[1] = W[2] = W[3] = 0u;
        if (!inside(a, 16u)) { bad |= 2; return; }
        if (touch) memcpy(W, (const void*)(uintptr_t)a, 16);
    }
    void store(uint64_t a, const uint32_t* W, uint32_t n, uint32_t align) const {
        if ((a % align) != 0u || a < out_lo || a + n > out_hi) { bad |= 4; return; }
        if (touch) memcpy((void*)(uintptr_t)a, W, n);
    }
    void store4(uint64_t a, uint32_t v) const { ++n[kStore4]; store(a, &v, 4u, 4u); }
    void store12(uint64_t a, const uint32_t (&W)[3]) const { ++n[kStore12]; store(a, W, 12u, 4u); }
    void store16(uint64_t a, const uint32_t (&W)[4]) const { ++n[kStore16]; store(a, W, 16u, 16u); }
};

template <uint32_t DT>
void item(const HostMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint32_t k) {
    const uint32_t sch = (e.cfg >> 16) & 15u;
    if ((e.cfg & 4u) != 0u) { if (sch == 4u) qoimi::ingest_item<DT, true, 4u>(mem, e, base, q, k); else qoimi::ingest_item<DT, true, 3u>(mem, e, base, q, k); }
    else { if (sch == 4u) qoimi::ingest_item<DT, false, 4u>(mem, e, base, q, k); else qoimi::ingest_item<DT, false, 3u>(mem, e, base, q, k); }
}

// The walk of one tile over the memory at `base` (the image) and q (the slot); touch: the addresses are real.
long long walk(uint64_t base, uint64_t q, bool touch, uint32_t w, uint32_t h, uint32_t sch, uint32_t src_flags, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch,
               uint32_t flags, uint32_t och, uint64_t* counts) {
    qoimi::TileEntry e;
    memset(&e, 0, sizeof e);
    e.w = w; e.x = x; e.y = y; e.cw = cw; e.ch = ch; e.tw = cw; e.th = ch;
    e.f = h;                                                                  // (an ingest entry holds the image's height there)
    e.cfg = qoimi::ingest_cfg(src_flags, sch, och, flags);
    const uint32_t dtype = qoimi::ingest_dtype(src_flags), elem = qoimi::ingest_elem(dtype);
    const size_t slot = ((size_t)cw * ch * och + 255u) & ~(size_t)255u;
    HostMem mem = {base, base + (uint64_t)w * h * sch * elem, q, q + slot, elem, touch};
    const uint64_t items = qoimi::ingest_items(cw, ch), tiles = qoimi::ingest_tiles(cw, ch);
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint32_t lane = 0; lane < qoimi::kTileThreads; ++lane) {
            const uint64_t k = t * qoimi::kTileThreads + lane;
            if (k >= items) continue;
            switch (dtype) {
                case qoimi::kIngestU8:   item<qoimi::kIngestU8>(mem, e, base, q, (uint32_t)k); break;
                case qoimi::kIngestF16:  item<qoimi::kIngestF16>(mem, e, base, q, (uint32_t)k); break;
                case qoimi::kIngestBF16: item<qoimi::kIngestBF16>(mem, e, base, q, (uint32_t)k); break;
                default:                 item<qoimi::kIngestF32>(mem, e, base, q, (uint32_t)k); break;
            }
        }
    if (counts) memcpy(counts, mem.n, sizeof mem.n);
    return mem.bad ? -(long long)mem.bad : (long long)tiles;
}

}  // namespace

extern "C" {

// One tile, item by item and tile by tile as tensor_ingest numbers them.  img: the tensor's first byte (a multiple of the element size; 16
// readable bytes in front of it and behind it); src_flags: QOIMI_TILE_SRC*; out: 256-aligned, (cw * ch * och rounded up to 256) bytes.
// Returns the tiles walked, or -(bits) where an address was wrong (1: an element load, 2: a wide load, 4: a store).
long long ingest_host_run(const uint8_t* img, uint32_t w, uint32_t h, uint32_t sch, uint32_t src_flags, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch,
                          uint32_t flags, uint32_t och, uint8_t* out) {
    return walk((uint64_t)(uintptr_t)img, (uint64_t)(uintptr_t)out, true, w, h, sch, src_flags, x, y, cw, ch, flags, och, nullptr);
}

// The same walk over virtual addresses - no memory is touched, so the image may be of any legal size: the image at an address that is
// base_mod modulo 256 (a multiple of the element size), the slot at a multiple of 256.  counts[7]: the loads of 2, 4, 8 and 16 bytes and the
// stores of 4, 12 and 16 bytes the tile makes - which branches of ingest_item, ingest_pixel and ingest_load_run it reaches.  Returns as
// ingest_host_run does; -8: base_mod is no address of an element.
long long ingest_host_paths(uint32_t w, uint32_t h, uint32_t sch, uint32_t src_flags, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t flags,
                            uint32_t och, uint32_t base_mod, uint64_t* counts) {
    if (base_mod >= 256u || base_mod % qoimi::ingest_elem(qoimi::ingest_dtype(src_flags)) != 0u) return -8;
    return walk(((uint64_t)1 << 40) + base_mod, (uint64_t)1 << 44, false, w, h, sch, src_flags, x, y, cw, ch, flags, och, counts);
}

uint64_t ingest_host_tiles(uint32_t cw, uint32_t ch) { return qoimi::ingest_tiles(cw, ch); }
uint64_t ingest_host_items(uint32_t cw, uint32_t ch) { return qoimi::ingest_items(cw, ch); }

// n elements with the bits in[i] of `dtype` in `range` (0, 1, 2) to bytes: the conversion alone
void ingest_host_bytes(const uint32_t* in, uint32_t n, uint32_t dtype, uint32_t range, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = (uint8_t)(dtype == qoimi::kIngestU8 ? in[i] & 255u : qoimi::ingest_byte(qoimi::ingest_widen(in[i], dtype), range));
}

}

#ifdef INGEST_HOST_MAIN
// The definition, written again: the element's value from its fields, the byte from the value.
static float value(uint32_t bits, uint32_t dtype) {
    if (dtype == 3u) { float f; memcpy(&f, &bits, 4); return f; }
    if (dtype == 2u) { bits <<= 16; float f; memcpy(&f, &bits, 4); return f; }
    const int e = (int)((bits >> 10) & 31u), m = (int)(bits & 0x3FFu);
    float v = e == 31 ? (m ? NAN : INFINITY) : e ? ldexpf((float)(1024 + m), e - 25) : ldexpf((float)m, -24);
    return (bits & 0x8000u) ? -v : v;
}
static uint8_t to_byte(float x, uint32_t range) {
    volatile float t = x;
    if (range == 0u) t = x * 255.0f;
    if (range == 1u) { t = x * 127.5f; t = t + 127.5f; }
    const float u = t;
    if (isnan(u) || u <= 0.0f) return 0;
    if (u >= 255.0f) return 255;
    return (uint8_t)nearbyintf(u);
}

int main() {
    struct Src { uint32_t w, h, off; };                                      // off: elements from a 16-aligned address
    const Src srcs[] = {{1, 1, 1}, {5, 3, 3}, {37, 23, 1}, {70, 9, 5}};
    uint32_t seed = 2024u;
    long long runs = 0;
    for (const Src& s : srcs)
        for (uint32_t dtype = 0; dtype < 4; ++dtype)
            for (uint32_t chw = 0; chw < 2; ++chw)
                for (uint32_t sch = 3; sch <= 4; ++sch)
                    for (uint32_t range = 0; range < (dtype == 0u ? 1u : 3u); ++range) {
                        const uint32_t elem = dtype == 0u ? 1u : dtype == 3u ? 4u : 2u;
                        const size_t count = (size_t)s.w * s.h * sch, bytes = count * elem;
                        uint8_t* raw = (uint8_t*)aligned_alloc(16, (bytes + 96u + 15u) & ~(size_t)15u);
                        uint8_t* img = raw + 16 + (size_t)s.off * elem;
                        std::vector<uint8_t> B(count);                           // h x w x sch
                        for (size_t i = 0; i < bytes + 64u; ++i) { seed = seed * 1664525u + 1013904223u; raw[i] = (uint8_t)(seed >> 24); }
                        for (size_t i = 0; i < count; ++i) {
                            uint32_t bits = 0;
                            if (dtype != 0u && (i % 5u) != 0u) {                    // mostly values around the range, some raw bit patterns
                                seed = seed * 1664525u + 1013904223u;
                                float f = (float)(seed >> 8) / 16777216.0f * 1.5f - 0.25f;
                                if (range == 1u) f = f * 2.0f - 1.0f;
                                if (range == 2u) f = f * 255.0f;
                                uint32_t fb; memcpy(&fb, &f, 4);
                                if (dtype == 3u) memcpy(img + i * 4u, &fb, 4);
                                else if (dtype == 2u) { const uint16_t hbits = (uint16_t)(fb >> 16); memcpy(img + i * 2u, &hbits, 2); }
                                else {                                            // truncated to binary16; below 2^-14 some subnormal
                                    const uint32_t a = fb & 0x7FFFFFFFu;
                                    const uint16_t hbits = (uint16_t)(((fb >> 16) & 0x8000u) | (a < 0x38800000u ? (a >> 20) & 0x3FFu : (a - 0x38000000u) >> 13));
                                    memcpy(img + i * 2u, &hbits, 2);
                                }
                            }
                            memcpy(&bits, img + i * elem, elem);
                            const size_t plane = (size_t)s.w * s.h;
                            const size_t at = chw ? (i % plane) * sch + i / plane : i;
                            B[at] = dtype == 0u ? (uint8_t)bits : to_byte(value(bits, dtype), range);
                        }
                        const uint32_t rects[][4] = {{0, 0, s.w, s.h}, {s.w > 2 ? 1u : 0u, 0, s.w > 2 ? s.w - 2 : s.w, s.h}, {s.w > 4 ? s.w - 4 : 0u, s.h > 1 ? 1u : 0u, s.w > 4 ? 4u : s.w, s.h > 1 ? s.h - 1 : s.h}};
                        const uint32_t src_flags = 16u | (chw ? 32u : 0u) | (dtype << 6) | (range << 8);
                        for (const auto& r : rects)
                            for (uint32_t flags = 0; flags < 4; ++flags)
                                for (uint32_t och = 3; och <= 4; ++och) {
                                    const size_t slot = ((size_t)r[2] * r[3] * och + 255u) & ~(size_t)255u;
                                    uint8_t* out = (uint8_t*)aligned_alloc(256, slot);
                                    memset(out, 0xEE, slot);
                                    const long long rc = ingest_host_run(img, s.w, s.h, sch, src_flags, r[0], r[1], r[2], r[3], flags, och, out);
                                    bool ok = rc >= 0;
                                    for (uint32_t Y = 0; ok && Y < r[3]; ++Y)
                                        for (uint32_t X = 0; ok && X < r[2]; ++X) {
                                            const uint32_t sx = r[0] + ((flags & 1u) ? r[2] - 1 - X : X), sy = r[1] + ((flags & 2u) ? r[3] - 1 - Y : Y);
                                            for (uint32_t c = 0; c < och; ++c) {
                                                const uint8_t want = c < sch ? B[((size_t)sy * s.w + sx) * sch + c] : 255;
                                                if (out[((size_t)Y * r[2] + X) * och + c] != want) ok = false;
                                            }
                                        }
                                    if (!ok) {
                                        fprintf(stderr, "FAIL %ux%u+%u dtype %u chw %u sch %u range %u rect %u,%u %ux%u flags %u och %u rc %lld\n", s.w, s.h, s.off, dtype, chw, sch, range,
                                                r[0], r[1], r[2], r[3], flags, och, rc);
                                        return 1;
                                    }
                                    free(out);
                                    ++runs;
                                }
                        free(raw);
                    }
    printf("ingest_host: %lld tiles ok\n", runs);
    return 0;
}
#endif

// label_id_host.cpp — the two ends of 24-bit label ids compiled for the host: the item loop of qoimi_encode_tiles over label sources with
// QOIMI_TILE_LABELS_ID24 (qoi_amd/csrc/qoi_label_core.h with its template parameter ID = 1) and the store of QOIMI_TENSOR_HW_ID24
// (qoi_amd/csrc/qoi_tensor_core.h: tensor_store).  The walk is label_host.cpp's - one table entry, tile by tile, the 256 lanes of a tile in
// a loop, another lane's registers read out of an array of 256 - with the variant chosen as label_ingest chooses it, from the entry's dtype
// field.  The plane stands in real memory at any element-aligned address and every load is checked against it: whole, naturally aligned
// elements inside the plane.  The slot and the tensor are the virtual array of host_mem.h (StoreMem): every store is checked and counted.
// tests/test_label_id_core_host.py compares it with the Python models without a GPU.  With -DLABEL_ID_HOST_MAIN the same source is a
// stand-alone program that walks a grid of tiles against a plain counting loop (the test builds it with -fsanitize=address,undefined and
// runs it).  Not part of the library.
#include <string.h>

#include "../../qoi_amd/csrc/qoi_label_core.h"
#include "../../qoi_amd/csrc/qoi_tensor_core.h"
#include "host_mem.h"

namespace {

// The kernel's memory.  A load is whole, naturally aligned elements inside the plane: of an int32 plane 4 bytes or 16, of an int64 plane 8
// or 16; of a u8 plane only the aligned dword, which holds at least one of its bytes.  The stores are StoreMem's.
struct IdHostMem : hostmem::StoreMem {
    uint64_t img_lo, img_hi;
    uint32_t elem;
    long long* loads;                                          // [4]: loads of 4, 8, 16 bytes, and all of them
    bool whole(uint64_t a, uint32_t n) const { return elem != 1u && n >= elem && (a % n) == 0u && a >= img_lo && a + n <= img_hi; }
    uint32_t load4(uint64_t a) const {
        ++loads[0]; ++loads[3];
        if (elem == 1u ? ((a & 3u) != 0u || a + 4u <= img_lo || a >= img_hi) : !whole(a, 4u)) { ++*bad; return 0u; }
        uint32_t v; memcpy(&v, (const void*)(uintptr_t)a, 4); return v;
    }
    void load8(uint64_t a, uint32_t (&W)[2]) const {
        ++loads[1]; ++loads[3];
        W[0] = W[1] = 0u;
        if (!whole(a, 8u)) { ++*bad; return; }
        memcpy(W, (const void*)(uintptr_t)a, 8);
    }
    void load16(uint64_t a, uint32_t (&W)[4]) const {
        ++loads[2]; ++loads[3];
        W[0] = W[1] = W[2] = W[3] = 0u;
        if (!whole(a, 16u)) { ++*bad; return; }
        memcpy(W, (const void*)(uintptr_t)a, 16);
    }
    void store12(uint64_t a, const uint32_t (&W)[3]) const {
        for (uint32_t k = 0; k < 3u; ++k) put(a + 4u * k, W[k], 4u);
    }
};

template <uint32_t DT, uint32_t ID>
void copy_tile(const IdHostMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tile) {
    for (uint32_t t = 0; t < qoimi::kTileThreads; ++t) {
        const uint64_t k = tile * qoimi::kTileThreads + t;
        if (k < qoimi::ingest_items(e.cw, e.ch)) qoimi::label_item<DT, ID>(mem, e, base, q, (uint32_t)k);
    }
}

template <uint32_t DT, uint32_t ID>
void nearest_tile(const IdHostMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tile) {
    for (uint32_t t = 0; t < qoimi::kTileThreads; ++t) {
        const uint64_t o = tile * qoimi::kTileThreads + t;
        if (o < (uint64_t)e.tw * e.th) qoimi::label_nearest_item<DT, ID>(mem, e, base, q, (uint32_t)o);
    }
}

// One tile as the kernel runs it: every one of the 256 lanes takes every step, whether its output pixel exists or not.
template <uint32_t DT, uint32_t ID>
void vote_tile(const IdHostMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tile) {
    using namespace qoimi;
    const uint32_t lg = e.cfg & 255u, L = 1u << lg;
    ModeHeld h[kTileThreads];
    uint32_t count[kTileThreads][kModeHold];
    uint64_t best[kTileThreads], next[kTileThreads], o[kTileThreads];
    bool valid[kTileThreads];
    for (uint32_t t = 0; t < kTileThreads; ++t) {
        const uint64_t item = tile * kTileThreads + t;
        o[t] = item >> lg;
        valid[t] = o[t] < (uint64_t)e.tw * e.th;
        if (valid[t]) label_vote_hold<DT, ID>(mem, e, base, (uint32_t)o[t], (uint32_t)item & (L - 1u), lg, h[t]);
        else mode_none(h[t]);
        for (uint32_t j = 0; j < kModeHold; ++j) count[t][j] = 0u;
    }
    for (uint32_t s = 0; s < L; ++s)                                  // (s = 0: the lane's own pixels)
        for (uint32_t t = 0; t < kTileThreads; ++t) {
            const uint32_t other = (t & ~(L - 1u)) | ((t + s) & (L - 1u));   // __shfl(., l + s, L)
            mode_meet(h[t], h[other].v, h[other].n, count[t]);
        }
    for (uint32_t t = 0; t < kTileThreads; ++t) best[t] = mode_best(h[t], count[t]);
    for (uint32_t step = 1u; step < L; step <<= 1) {                  // __shfl_xor(., step)
        for (uint32_t t = 0; t < kTileThreads; ++t) next[t] = best[t ^ step] > best[t] ? best[t ^ step] : best[t];
        for (uint32_t t = 0; t < kTileThreads; ++t) best[t] = next[t];
    }
    for (uint32_t t = 0; t < kTileThreads; ++t)
        if (valid[t] && (t & (L - 1u)) == 0u) tile_put(mem, e, q, (uint32_t)o[t], mode_pick(best[t]));
}

template <uint32_t DT, uint32_t ID>
void walk(const IdHostMem& mem, const qoimi::TileEntry& e, uint64_t base, uint64_t q, uint64_t tiles) {
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        if (e.f == 1u) copy_tile<DT, ID>(mem, e, base, q, tile);
        else if ((e.cfg & (1u << 24)) == 0u) nearest_tile<DT, ID>(mem, e, base, q, tile);
        else vote_tile<DT, ID>(mem, e, base, q, tile);
    }
}

}  // namespace

extern "C" {

// One table entry as label_ingest walks it.  img: the plane's first byte (w x h elements of dtype 0 u8 / 1 i32 / 2 i64, a multiple of the
// element size; 16 readable bytes in front of it and behind it); flags: the flips, and bit 15 (QOIMI_TILE_LABELS_ID24) or not; vote: the
// call's mode is QOIMI_TILE_MODE; the slot begins at out[q - base], q a multiple of 256; writes[i] counts the stores to out[i]; loads[4]: the
// loads of 4, 8 and 16 bytes and their sum.  Returns the tiles walked, or -1 - the number of bad accesses if there was one, or -1000000 if
// the entry's dtype field holds a value the kernel has no case for.
long long label_id_host_run(const uint8_t* img, uint32_t w, uint32_t h, uint32_t dtype, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t f,
                            uint32_t flags, uint32_t och, uint32_t vote, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len, long long* loads) {
    using namespace qoimi;
    long long bad = 0, none[4] = {0, 0, 0, 0};
    TileEntry e;
    memset(&e, 0, sizeof e);
    e.w = w; e.x = x; e.y = y; e.cw = cw; e.ch = ch; e.f = f;
    e.tw = thumb_extent(cw, f); e.th = thumb_extent(ch, f);
    e.cfg = label_cfg((dtype << kTileLabelsDtypeShift) | kTileLabels | flags, f, vote != 0u, och);
    const uint64_t at = (uint64_t)(uintptr_t)img;
    const uint32_t elem = label_elem(dtype);
    IdHostMem mem = {{out, writes, out_len, base, &bad, nullptr}, at, at + (uint64_t)w * h * elem, elem, loads ? loads : none};
    const uint64_t tiles = label_tiles(cw, ch, f, vote != 0u, och);
    switch ((e.cfg >> 16) & 15u) {                                      // (the cases of label_ingest)
        case kLabelU8:               walk<kLabelU8, 0u>(mem, e, at, q, tiles); break;
        case kLabelI32:              walk<kLabelI32, 0u>(mem, e, at, q, tiles); break;
        case kLabelI64:              walk<kLabelI64, 0u>(mem, e, at, q, tiles); break;
        case kLabelId24 | kLabelU8:  walk<kLabelU8, 1u>(mem, e, at, q, tiles); break;
        case kLabelId24 | kLabelI32: walk<kLabelI32, 1u>(mem, e, at, q, tiles); break;
        case kLabelId24 | kLabelI64: walk<kLabelI64, 1u>(mem, e, at, q, tiles); break;
        default: return -1000000;
    }
    return hostmem::checked(bad, (long long)tiles);
}

uint32_t label_id_host_cfg(uint32_t flags, uint32_t f, uint32_t vote, uint32_t och) { return qoimi::label_cfg(flags, f, vote != 0u, och); }

// n int64 values (as lo, hi dwords) and their low dwords as int32 to ids: the saturation alone
void label_id_host_ids(const uint32_t* in, uint32_t n, uint32_t* out64, uint32_t* out32) {
    for (uint32_t i = 0; i < n; ++i) { out64[i] = qoimi::label_id64(in[2u * i], in[2u * i + 1u]); out32[i] = qoimi::label_id32(in[2u * i]); }
}

// tensor_store of the ow x oh pixels px (r | g << 8 | b << 16 | a << 24, in the order of the unflipped result) with the layout
// QOIMI_TENSOR_HW_ID24 and the dtype given (5 I32, 6 I64) to the tensor at q.  Returns the stores, or -1 - the number of bad ones.
long long label_id_host_store(const uint32_t* px, uint32_t ow, uint32_t oh, uint32_t och, uint32_t dtype, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes,
                              uint64_t out_len) {
    long long bad = 0, stores = 0;
    const hostmem::StoreMem mem = {out, writes, out_len, base, &bad, &stores};
    qoimi::TensorFormat fmt;
    fmt.dtype = dtype; fmt.layout = qoimi::kTensorHWId24;
    for (int k = 0; k < 4; ++k) { fmt.scale[k] = 1.0f; fmt.bias[k] = 0.0f; }
    for (uint32_t Y = 0; Y < oh; ++Y)
        for (uint32_t X = 0; X < ow; ++X) qoimi::tensor_store(mem, fmt, q, och, ow, oh, X, Y, px[(size_t)Y * ow + X]);
    return hostmem::checked(bad, stores);
}

}

#ifdef LABEL_ID_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

// The definition, written again: the id of element (k, r) of the rectangle, from the value.
static uint32_t plain_id(const uint8_t* img, uint32_t w, uint32_t dtype, uint32_t x, uint32_t y, uint32_t k, uint32_t r) {
    const size_t i = (size_t)(y + r) * w + x + k;
    long long v;
    if (dtype == 0u) v = img[i];
    else if (dtype == 1u) { int32_t s; memcpy(&s, img + 4u * i, 4); v = s; }
    else { int64_t s; memcpy(&s, img + 8u * i, 8); v = s; }
    return v < 0 ? 0u : v > 16777215 ? 16777215u : (uint32_t)v;
}

// The vote's order among winners: r << 24 | g << 16 | b << 8 | a of the pixel (id & 255, id >> 8 & 255, id >> 16, 255)
static uint32_t plain_key(uint32_t id) { return (id & 255u) << 24 | ((id >> 8) & 255u) << 16 | (id >> 16) << 8 | 255u; }

// ... and of output pixel (X, Y): the centre, or the vote as a plain counting loop over the block's ids
static uint32_t plain_pixel(const uint8_t* img, uint32_t w, uint32_t dtype, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t f, bool vote, uint32_t X, uint32_t Y) {
    const uint32_t nx = cw - X * f < f ? cw - X * f : f, ny = ch - Y * f < f ? ch - Y * f : f;
    const uint32_t centre = plain_id(img, w, dtype, x, y, X * f + nx / 2u, Y * f + ny / 2u);
    if (!vote) return centre;
    uint32_t ids[256], top = 0, n_centre = 0;
    const uint32_t n = nx * ny;
    for (uint32_t r = 0; r < ny; ++r) for (uint32_t k = 0; k < nx; ++k) ids[r * nx + k] = plain_id(img, w, dtype, x, y, X * f + k, Y * f + r);
    uint32_t best = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < n; ++j) c += ids[j] == ids[i] ? 1u : 0u;
        if (ids[i] == centre) n_centre = c;
        if (c > top || (c == top && plain_key(ids[i]) < plain_key(best))) { top = c; best = ids[i]; }
    }
    return n_centre == top ? centre : best;
}

// Planes of a few ids that differ in their low, middle and high bytes and some values far outside 0..2^24 - 1, at every element-aligned
// residue of 16 the dtype has; rectangles at odd corners; factors with their own splits, both och, all four flips.  The slot stands between
// two guard bands.  Then the store: every pixel's id as I32 and I64, the tensor between two guard bands.
int main() {
    struct Src { uint32_t w, h; };
    const Src srcs[] = {{1, 1}, {5, 1}, {37, 23}, {70, 45}, {1025, 2}};
    const uint32_t factors[] = {1, 2, 3, 5, 16, 64};
    const long long few[] = {0, 1, 256, 65536, 65537, 16777215, 70000, 513};
    const long long wild[] = {16777216, -1, -100, 2147483647LL, -2147483647LL - 1, 4294967296LL, 4294967301LL, -4294967289LL, 9223372036854775807LL, -9223372036854775807LL - 1};
    const uint64_t base = 4096, guard = 256;
    uint32_t seed = 4242u;
    long long runs = 0;
    for (const Src& s : srcs)
        for (uint32_t dtype = 0; dtype < 3; ++dtype) {
            const uint32_t elem = dtype == 0u ? 1u : dtype == 1u ? 4u : 8u;
            for (uint32_t res = 0; res < 16u; res += (elem == 1u ? 1u : elem)) {
                if (elem == 1u && res >= 4u) break;
                const size_t bytes = (size_t)s.w * s.h * elem;
                uint8_t* raw = (uint8_t*)aligned_alloc(16, (bytes + 64u + 15u) & ~(size_t)15u);
                uint8_t* img = raw + 16 + res;
                for (size_t i = 0; i < bytes + 48u; ++i) raw[i] = 0x5Au;
                for (size_t p = 0; p < (size_t)s.w * s.h; ++p) {
                    seed = seed * 1664525u + 1013904223u;
                    long long v = few[(seed >> 24) % (dtype == 0u ? 2u : 8u)];
                    if (((seed >> 16) & 15u) == 0u) v = wild[(seed >> 8) % 10u];
                    if (dtype == 0u) img[p] = (uint8_t)(v * 85);
                    else if (dtype == 1u) { const int32_t t = (int32_t)v; memcpy(img + 4u * p, &t, 4); }
                    else { const int64_t t = v; memcpy(img + 8u * p, &t, 8); }
                }
                const uint32_t rects[][4] = {{0, 0, s.w, s.h}, {s.w > 8 ? 3u : 0u, s.h > 12 ? 5u : 0u, s.w > 8 ? s.w - 7 : s.w, s.h > 12 ? s.h - 9 : s.h}};
                for (const auto& r : rects)
                    for (uint32_t vote = 0; vote < 2; ++vote)
                        for (uint32_t f : factors)
                            for (uint32_t flags = 0; flags < 4; ++flags)
                                for (uint32_t och = 3; och <= 4; ++och) {
                                    if (vote && f > 16u) continue;
                                    const uint32_t tw = (r[2] + f - 1) / f, th = (r[3] + f - 1) / f;
                                    const size_t P = (size_t)tw * th, B = P * och, slot = (B + 255u) & ~(size_t)255u;
                                    const size_t stored = f != 1u ? B : och == 4u ? 16u * ((P + 3u) / 4u) : 4u * ((3u * P + 3u) / 4u);
                                    std::vector<uint8_t> out(guard + slot + guard, hostmem::kGuard), writes(out.size(), 0);
                                    const long long rc = label_id_host_run(img, s.w, s.h, dtype, r[0], r[1], r[2], r[3], f, flags | qoimi::kTileLabelsId24, och, vote, base + guard, base,
                                                                           out.data(), writes.data(), guard + slot, nullptr);       // (a store behind the slot is a bad access)
                                    if (rc < 0) { printf("%lld bad accesses: %ux%u dtype %u +%u rect %u,%u %ux%u vote %u f %u flags %u och %u\n", -1 - rc, s.w, s.h, dtype, res, r[0], r[1], r[2], r[3], vote, f, flags, och); return 1; }
                                    const long long off = hostmem::first_miswritten(out, writes, guard, stored);
                                    if (off >= 0) { printf("byte %lld written %u times: dtype %u vote %u f %u och %u\n", off, writes[off], dtype, vote, f, och); return 1; }
                                    std::vector<uint32_t> px(P);
                                    for (uint32_t Y = 0; Y < th; ++Y)
                                        for (uint32_t X = 0; X < tw; ++X) {
                                            const uint32_t id = plain_pixel(img, s.w, dtype, r[0], r[1], r[2], r[3], f, vote != 0u, X, Y);
                                            const uint32_t dx = (flags & 1u) ? tw - 1 - X : X, dy = (flags & 2u) ? th - 1 - Y : Y;
                                            uint32_t got = 0;
                                            for (uint32_t c = 0; c < och; ++c) got |= (uint32_t)out[guard + ((size_t)dy * tw + dx) * och + c] << (8u * c);
                                            px[(size_t)dy * tw + dx] = got;
                                            if (got != (och == 4u ? id | 0xFF000000u : id)) {
                                                printf("wrong pixel: %ux%u dtype %u +%u rect %u,%u %ux%u vote %u f %u flags %u och %u at (%u, %u): %08x for id %u\n", s.w, s.h, dtype, res, r[0], r[1],
                                                       r[2], r[3], vote, f, flags, och, X, Y, got, id);
                                                return 1;
                                            }
                                        }
                                    // the store end: the tile's pixels to ids again, as I32 and as I64
                                    for (uint32_t td = 5; td <= 6; ++td) {
                                        const size_t E = td == 5u ? 4u : 8u, T = P * E;
                                        std::vector<uint8_t> ten(guard + T + guard, hostmem::kGuard), tw_(ten.size(), 0);
                                        const long long st = label_id_host_store(px.data(), tw, th, och, td, base + guard, base, ten.data(), tw_.data(), ten.size());
                                        if (st != (long long)(P * (E / 4u))) { printf("store: %lld for %zu pixels of dtype %u\n", st, P, td); return 1; }
                                        if (hostmem::first_miswritten(ten, tw_, guard, T) >= 0) { printf("store: a byte beside the tensor, or one written twice\n"); return 1; }
                                        for (size_t i = 0; i < P; ++i) {
                                            uint64_t v = 0;
                                            memcpy(&v, ten.data() + guard + i * E, E);
                                            if (v != (px[i] & 0xFFFFFFu)) { printf("store: element %zu is %llu, pixel %08x\n", i, (unsigned long long)v, px[i]); return 1; }
                                        }
                                    }
                                    ++runs;
                                }
                free(raw);
            }
        }
    printf("label_id_host: %lld tiles ok\n", runs);
    return 0;
}
#endif

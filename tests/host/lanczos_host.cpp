// lanczos_host.cpp — the arithmetic of qoimi_decode_tensors with QOIMI_FILTER_LANCZOS (qoi_amd/csrc/qoi_lanczos_core.h over the generated
// table qoi_lanczos_table.h) compiled for the host: the walk of tensor_lanczos over an item, tile by tile - first the normalisation of the
// tile's columns and rows into two tables of exactly the size the kernel's LDS has, then lane by lane - over a synthetic staging array and a
// memory functor that checks and counts every access, so that tests/test_lanczos_core_host.py can compare it with the Python model without a
// GPU.  The sums of a pixel's lanes are added here where the kernel takes its butterfly steps; the store is TensorSink of qoi_tensor_core.h
// with u8 HWC, as the kernel's.  lanczos_host_pixel computes single output pixels of geometries no array can hold: its functor makes a staged
// pixel from its index.  With -DLANCZOS_HOST_MAIN the same source is a stand-alone program that walks a grid of items against a plain loop
// over all taps (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../qoi_amd/csrc/qoi_lanczos_table.h"
#include "../../qoi_amd/csrc/qoi_lanczos_core.h"
#include "../../qoi_amd/csrc/qoi_tensor_core.h"

namespace {

static_assert(sizeof(qoimi::kLanczosTable) == qoimi::kLanczosEntries * sizeof(int32_t), "the table the core indexes");

// Addresses are virtual: `base` (a multiple of 16) stands for out[0], so the test chooses every alignment of q.
struct HostMem {
    const uint32_t* stage; uint64_t stage_px;
    uint8_t* out; uint8_t* writes; uint64_t out_len, base;
    long long* bad;                      // accesses outside an array or not naturally aligned
    long long* loads;
    uint32_t load(uint64_t i) const {
        ++*loads;
        if (i >= stage_px) { ++*bad; return 0u; }
        return stage[i];
    }
    void put(uint64_t a, uint32_t v, uint32_t bytes) const {
        if (a % bytes != 0u || a < base || a - base + bytes > out_len) { ++*bad; return; }
        for (uint32_t k = 0; k < bytes; ++k) { out[a - base + k] = (uint8_t)(v >> (8u * k)); ++writes[a - base + k]; }
    }
    void store1(uint64_t a, uint32_t v) const { put(a, v, 1u); }
    void store2(uint64_t a, uint32_t v) const { put(a, v, 2u); }
    void store4(uint64_t a, uint32_t v) const { put(a, v, 4u); }
};

// The staged pixel at index i is lanczos_host_synth(i); loads from stage_px on are counted as bad.  One store4 lands in *px.
struct SynthMem {
    uint64_t stage_px; uint32_t* px; long long* bad; long long* loads; long long* stores;
    uint32_t load(uint64_t i) const {
        ++*loads;
        if (i >= stage_px) { ++*bad; return 0u; }
        uint64_t z = (i + 1u) * 0x9E3779B97F4A7C15ull;
        z ^= z >> 29;
        return (uint32_t)(z >> 16);
    }
    void store1(uint64_t, uint32_t) const { ++*bad; }
    void store2(uint64_t, uint32_t) const { ++*bad; }
    void store4(uint64_t a, uint32_t v) const { ++*stores; if (a % 4u != 0u) ++*bad; *px = v; }
};

const uint16_t kPoison = 0xFFFFu;        // no table entry: it would be q = 3 * 2^14 - 1, the end of the asserted range, and the largest q is 42130

// The tables of a tile as the kernel's LDS holds them: every entry of the columns and rows the tile holds written once, nothing else.
struct Tables {
    std::vector<uint16_t> qx, qy;
    Tables() : qx(qoimi::kLanczosColSlots), qy(qoimi::kLanczosRowSlots) {}
    bool fill(const qoimi::CubicTile& t, const qoimi::ResizeGeom& g) {
        if ((uint64_t)t.nx * t.sx > qx.size() || (uint64_t)t.ny * t.sy > qy.size()) return false;
        qx.assign(qx.size(), kPoison); qy.assign(qy.size(), kPoison);
        for (uint32_t i = 0; i < t.nx + t.ny; ++i) qoimi::lanczos_tile_norm(qoimi::kLanczosTable, t, g, i, qx.data(), qy.data());
        for (size_t i = 0; i < qx.size(); ++i) if ((qx[i] == kPoison) != (i >= (size_t)t.nx * t.sx)) return false;
        for (size_t i = 0; i < qy.size(); ++i) if ((qy[i] == kPoison) != (i >= (size_t)t.ny * t.sy)) return false;
        return true;
    }
};

template <class Mem>
void pixel_sums(const Mem& mem, const qoimi::ResizeGeom& g, const qoimi::CubicTile& t, const Tables& tb, uint32_t lg, uint32_t c, uint64_t o, uint32_t X, uint32_t Y,
                bool wgt, qoimi::ResizeSums& sum) {
    sum = qoimi::ResizeSums{{0, 0, 0, 0}, {0, 0, 0}};
    const uint16_t* qx = tb.qx.data() + (size_t)qoimi::cubic_tile_slot(t, o, X) * t.sx;
    const uint16_t* qy = tb.qy.data() + (size_t)(Y - t.Y0) * t.sy;
    for (uint32_t l = 0; l < (1u << lg); ++l) {
        qoimi::ResizeSums s;
        if (wgt) qoimi::lanczos_lane<true>(mem, g, qx, qy, t.sy, X, Y, l, c, s);
        else qoimi::lanczos_lane<false>(mem, g, qx, qy, t.sy, X, Y, l, c, s);
        for (int k = 0; k < 4; ++k) sum.S[k] += s.S[k];
        for (int k = 0; k < 3; ++k) sum.W[k] += s.W[k];
    }
}

}  // namespace

extern "C" {

// One item as tensor_lanczos walks it with a u8 HWC format: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes begins
// at out[q - base].  writes[i] counts the stores to out[i].  Returns the loads made, or -1 - the number of bad accesses if there was one (a
// table that does not fit or is not written exactly counts as one); *tiles_walked reports the tiles, *normalised
// the columns and rows normalised over all tiles.
long long lanczos_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                           uint32_t flags, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len,
                           unsigned long long* tiles_walked, unsigned long long* normalised) {
    long long bad = 0, loads = 0;
    const HostMem mem = {stage, stage_px, out, writes, out_len, base, &bad, &loads};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, flags};
    const qoimi::TensorSink sink{{qoimi::kTensorU8, qoimi::kTensorHWC, {1.0f, 1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f, 0.0f}}};
    uint32_t lg, c;
    qoimi::lanczos_split(cw, ow, lg, c);
    const uint64_t tiles = qoimi::lanczos_tiles(cw, ow, oh);
    const bool wgt = weighted != 0 && och == 4u;
    unsigned long long norm = 0;
    Tables tb;
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        const qoimi::CubicTile t = qoimi::lanczos_tile(g, lg, c, tile);
        if (!tb.fill(t, g)) { ++bad; break; }
        norm += t.nx + t.ny;
        for (uint32_t p = 0; p < t.px; ++p) {                                          // the lanes of one output pixel
            const uint64_t o = t.o0 + p;
            const uint32_t Y = (uint32_t)qoimi::resize_div(o, ow), X = (uint32_t)(o - (uint64_t)Y * ow);
            qoimi::ResizeSums sum;
            pixel_sums(mem, g, t, tb, lg, c, o, X, Y, wgt, sum);
            sink(mem, g, q, och, X, Y, qoimi::cubic_pixel(sum, wgt));
        }
    }
    if (tiles_walked) *tiles_walked = tiles;
    if (normalised) *normalised = norm;
    return bad ? -1 - bad : loads;
}

// Output pixel (X, Y) of the unflipped result of an item over synthetic staged pixels (rows of w, stage_px of them), 4 channels, written as
// one dword to *px; sums[0..6] receive N_r, N_g, N_b, N_a, M_r, M_g, M_b (signed).  Returns the loads, or -1 - bad accesses.
long long lanczos_host_pixel(uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, int weighted,
                             uint32_t X, uint32_t Y, uint32_t* px, long long* sums) {
    long long bad = 0, loads = 0, stores = 0;
    const SynthMem mem = {stage_px, px, &bad, &loads, &stores};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, 0u};
    const qoimi::TensorSink sink{{qoimi::kTensorU8, qoimi::kTensorHWC, {1.0f, 1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f, 0.0f}}};
    uint32_t lg, c;
    qoimi::lanczos_split(cw, ow, lg, c);
    const uint64_t o = (uint64_t)Y * ow + X;
    const qoimi::CubicTile t = qoimi::lanczos_tile(g, lg, c, o / (qoimi::kResizeThreads >> lg));
    Tables tb;
    if (!tb.fill(t, g)) return -1;
    qoimi::ResizeSums sum;
    pixel_sums(mem, g, t, tb, lg, c, o, X, Y, weighted != 0, sum);
    sink(mem, g, 0u, 4u, X, Y, qoimi::cubic_pixel(sum, weighted != 0));
    for (int k = 0; k < 4; ++k) sums[k] = (long long)sum.S[k];
    for (int k = 0; k < 3; ++k) sums[4 + k] = (long long)sum.W[k];
    if (stores != 1) ++bad;
    return bad ? -1 - bad : loads;
}

uint32_t lanczos_host_synth(uint64_t i) {
    long long bad = 0, loads = 0, stores = 0;
    uint32_t px = 0;
    const SynthMem mem = {~0ull, &px, &bad, &loads, &stores};
    return mem.load(i);
}

int lanczos_host_table(uint32_t i) { return qoimi::kLanczosTable[i]; }
void lanczos_host_split(uint32_t cw, uint32_t ow, uint32_t* lg, uint32_t* c) { qoimi::lanczos_split(cw, ow, *lg, *c); }
uint32_t lanczos_host_taps(uint32_t cw, uint32_t ow) { return qoimi::lanczos_taps(cw, ow); }
uint32_t lanczos_host_first(uint32_t Z, uint32_t n_src, uint32_t n_out) { return qoimi::filter_first(Z, n_src, n_out, qoimi::kLanczosLobes); }
long long lanczos_host_weight(uint32_t Z, uint32_t k, uint32_t n_src, uint32_t n_out) {
    return qoimi::lanczos_weight(qoimi::kLanczosTable, (2u * Z + 1u) * n_src, k, n_out, qoimi::cubic_unit(n_src, n_out));
}
// q(Z, first + j) for j < slots <= 96 into q[j]
void lanczos_host_norm(uint32_t Z, uint32_t n_src, uint32_t n_out, uint32_t slots, int* q) {
    uint16_t tab[96];
    qoimi::lanczos_norm(qoimi::kLanczosTable, Z, n_src, n_out, slots, tab);
    for (uint32_t j = 0; j < slots; ++j) q[j] = (int)tab[j] - qoimi::kLanczosBias;
}
unsigned long long lanczos_host_tiles(uint32_t cw, uint32_t ow, uint32_t oh) { return qoimi::lanczos_tiles(cw, ow, oh); }

}

#ifdef LANCZOS_HOST_MAIN
#include <stdio.h>

static int64_t floor_div(int64_t n, int64_t d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }

// q of one axis by the definition, over all samples
static std::vector<int64_t> axis_weights(int64_t Z, int64_t n_src, int64_t n_out) {
    const int64_t u = 2 * (n_src > n_out ? n_src : n_out), o = (2 * Z + 1) * n_src;
    std::vector<int64_t> c(n_src), q(n_src);
    int64_t W = 0, best = 0, sum = 0;
    for (int64_t k = 0; k < n_src; ++k) {
        const int64_t s = (2 * k + 1) * n_out, d = o > s ? o - s : s - o;
        c[k] = 0;
        if (d < 3 * u) {
            const int64_t z = 1024 * d, i = z / u, r = z - i * u;
            c[k] = (int64_t)qoimi::kLanczosTable[i] * (u - r) + (int64_t)qoimi::kLanczosTable[i + 1] * r;
        }
        W += c[k];
        if (c[k] > c[best]) best = k;
    }
    for (int64_t k = 0; k < n_src; ++k) { q[k] = floor_div(c[k] * 32768 + W / 2, W); sum += q[k]; }
    q[best] += 32768 - sum;
    return q;
}

static int64_t clamp255(int64_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Every och, mode and flag value, a set of alignments and of size pairs (identity, reductions up to the cap with 96 taps, enlargements, mixed
// axes, more than one tile, tiles of many rows), in arrays of exactly the size the walk may touch: the staging ends with the item's last row,
// the output with its guard band.
int main() {
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {11, 9, 3, 2}, {11, 9, 13, 11}, {11, 9, 11, 9}, {12, 8, 3, 2}, {5, 3, 13, 7}, {1, 1, 4, 3}, {31, 3, 2, 3},
                                 {64, 32, 4, 2}, {9, 130, 20, 9}, {40, 40, 37, 23}, {3, 1, 2, 1}, {2, 300, 1, 290}, {5, 3, 300, 2}, {3, 3, 19, 11}, {128, 3, 8, 1}};
    const uint64_t base = 4096, guard = 32;
    long long items = 0;
    for (uint32_t och = 3; och <= 4; ++och)
        for (int weighted = 0; weighted < 2; ++weighted)
            for (uint32_t a : {0u, 1u, 6u, 15u})
                for (uint32_t flags = 0; flags < 4; ++flags)
                    for (const auto& sz : sizes) {
                        const uint32_t cw = sz[0], rh = sz[1], ow = sz[2], oh = sz[3], x = 3, y = 2, w = cw + 5;
                        std::vector<uint32_t> stage((size_t)w * (y + rh));
                        for (size_t i = 0; i < stage.size(); ++i) {
                            stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                            if (i % 5u == 0u) stage[i] &= 0x00FFFFFFu;                       // some transparent pixels
                            if (i % 7u == 0u) stage[i] = (i % 2u) ? 0xFFFFFFFFu : 0u;        // hard edges: the lobes overshoot
                        }
                        const uint64_t B = (uint64_t)ow * oh * och;
                        std::vector<uint8_t> out(guard + a + B + guard, 0xA5), writes(out.size(), 0);
                        const uint64_t q = base + guard + a;
                        unsigned long long tiles = 0, norm = 0;
                        const long long rc = lanczos_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, och, weighted, q, base, out.data(),
                                                              writes.data(), out.size(), &tiles, &norm);
                        if (rc < 0) { printf("bad access: och %u a %u flags %u %ux%u -> %ux%u: %lld\n", och, a, flags, cw, rh, ow, oh, rc); return 1; }
                        for (size_t i = 0; i < out.size(); ++i) {
                            const bool inside = i >= guard + a && i < guard + a + B;
                            if (writes[i] != (inside ? 1 : 0) || (!inside && out[i] != 0xA5)) { printf("byte %zu written %u times\n", i, writes[i]); return 1; }
                        }
                        for (uint32_t Y = 0; Y < oh; ++Y) {
                            const std::vector<int64_t> qy = axis_weights(Y, rh, oh);
                            for (uint32_t X = 0; X < ow; ++X) {
                                const std::vector<int64_t> qx = axis_weights(X, cw, ow);
                                int64_t N[4] = {0, 0, 0, 0}, M[3] = {0, 0, 0};
                                for (uint32_t r = 0; r < rh; ++r)
                                    for (uint32_t k = 0; k < cw; ++k) {
                                        const int64_t wt = qy[r] * qx[k];
                                        const uint32_t px = stage[(size_t)(y + r) * w + x + k];
                                        for (int ch = 0; ch < 4; ++ch) N[ch] += wt * (int64_t)((px >> (8 * ch)) & 255u);
                                        for (int ch = 0; ch < 3; ++ch) M[ch] += wt * (int64_t)((px >> (8 * ch)) & 255u) * (int64_t)(px >> 24);
                                    }
                                const uint32_t xo = (flags & 1u) ? ow - 1u - X : X, yo = (flags & 2u) ? oh - 1u - Y : Y;
                                for (uint32_t ch = 0; ch < och; ++ch) {
                                    int64_t v = clamp255(floor_div(N[ch] + (1ll << 29), 1ll << 30));
                                    if (weighted && och == 4u && ch < 3u && N[3] > 0) v = clamp255(floor_div(M[ch] + N[3] / 2, N[3]));
                                    if (out[guard + a + ((size_t)yo * ow + xo) * och + ch] != (uint8_t)v) {
                                        printf("wrong byte: och %u mode %d a %u flags %u %ux%u -> %ux%u at (%u, %u).%u\n", och, weighted, a, flags, cw, rh, ow, oh, X, Y, ch);
                                        return 1;
                                    }
                                }
                            }
                        }
                        ++items;
                    }
    printf("lanczos_host: %lld items ok\n", items);
    return 0;
}
#endif

// lanczos_host.cpp — the arithmetic of qoimi_decode_tensors with QOIMI_FILTER_LANCZOS (qoi_amd/csrc/qoi_lanczos_core.h over the generated
// table qoi_lanczos_table.h) compiled for the host: the walk of tensor_lanczos over an item as table_filter_host.h makes it, over a synthetic
// staging array and the checking memory functors of host_mem.h, so that tests/test_lanczos_core_host.py can compare it with the Python model
// without a GPU.  lanczos_host_pixel computes single output pixels of geometries no array can hold.  With -DLANCZOS_HOST_MAIN the same source
// is a stand-alone program that walks a grid of items against a plain loop over all taps (the test builds it with the sanitizers and runs
// it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_lanczos_table.h"
#include "../../qoi_amd/csrc/qoi_lanczos_core.h"
#include "table_filter_host.h"

namespace {

static_assert(sizeof(qoimi::kLanczosTable) == qoimi::kLanczosEntries * sizeof(int32_t), "the table the core indexes");

struct LanczosHost {
    static constexpr uint32_t kColSlots = qoimi::kLanczosColSlots, kRowSlots = qoimi::kLanczosRowSlots;
    static qoimi::CubicTile tile(const qoimi::ResizeGeom& g, uint32_t lg, uint32_t c, uint64_t tile) { return qoimi::lanczos_tile(g, lg, c, tile); }
    static void norm(const qoimi::CubicTile& t, const qoimi::ResizeGeom& g, uint32_t i, uint16_t* qx, uint16_t* qy) {
        qoimi::lanczos_tile_norm(qoimi::kLanczosTable, t, g, i, qx, qy);
    }
    template <bool WEIGHTED, class Mem>
    static void lane(const Mem& mem, const qoimi::ResizeGeom& g, const uint16_t* qx, const uint16_t* qy, uint32_t sy, uint32_t X, uint32_t Y, uint32_t l, uint32_t c,
                     qoimi::ResizeSums& s) {
        qoimi::lanczos_lane<WEIGHTED>(mem, g, qx, qy, sy, X, Y, l, c, s);
    }
    static void split(uint32_t cw, uint32_t ow, uint32_t& lg, uint32_t& c) { qoimi::lanczos_split(cw, ow, lg, c); }
    static uint64_t tiles(uint32_t cw, uint32_t ow, uint32_t oh) { return qoimi::lanczos_tiles(cw, ow, oh); }
};

}  // namespace

extern "C" {

// table_filter_run and table_filter_pixel of table_filter_host.h with the Lanczos filter
long long lanczos_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                           uint32_t flags, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len,
                           unsigned long long* tiles_walked, unsigned long long* normalised) {
    return hostmem::table_filter_run<LanczosHost>(stage, stage_px, w, x, y, cw, rh, ow, oh, flags, och, weighted, q, base, out, writes, out_len, tiles_walked, normalised);
}
long long lanczos_host_pixel(uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, int weighted,
                             uint32_t X, uint32_t Y, uint32_t* px, long long* sums) {
    return hostmem::table_filter_pixel<LanczosHost>(stage_px, w, x, y, cw, rh, ow, oh, weighted, X, Y, px, sums);
}
uint32_t lanczos_host_synth(uint64_t i) { return hostmem::SynthMem::synth(i); }

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
                        std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                        const uint64_t q = base + guard + a;
                        unsigned long long tiles = 0, norm = 0;
                        const long long rc = lanczos_host_run(stage.data(), stage.size(), w, x, y, cw, rh, ow, oh, flags, och, weighted, q, base, out.data(),
                                                              writes.data(), out.size(), &tiles, &norm);
                        if (rc < 0) { printf("bad access: och %u a %u flags %u %ux%u -> %ux%u: %lld\n", och, a, flags, cw, rh, ow, oh, rc); return 1; }
                        const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                        if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
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
                                for (uint32_t ch = 0; ch < och; ++ch) {
                                    int64_t v = clamp255(floor_div(N[ch] + (1ll << 29), 1ll << 30));
                                    if (weighted && och == 4u && ch < 3u && N[3] > 0) v = clamp255(floor_div(M[ch] + N[3] / 2, N[3]));
                                    if (out[guard + a + hostmem::element_index(false, flags, ow, oh, och, X, Y, ch)] != (uint8_t)v) {
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

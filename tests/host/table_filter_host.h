// table_filter_host.h — the walk bicubic_host.cpp and lanczos_host.cpp share, as the kernels share table_tiles<> (qoi_table_tiles.h): an item
// tile by tile - first the normalisation of the tile's columns and rows into two tables of exactly the size the kernel's LDS has, then lane
// by lane, the sums of a pixel's lanes added where the kernel takes its butterfly steps - into TensorSink with u8 HWC, as the kernel's.  A
// filter is a traits struct F of the shape of CubicFilter / LanczosFilter in qoi_cubic.hip / qoi_lanczos.hip:
//     kColSlots, kRowSlots; tile(g, lg, c, tile); norm(t, g, i, qx, qy); lane<WEIGHTED>(mem, g, qx, qy, sy, X, Y, l, c, s);
//     split(cw, ow, lg, c); tiles(cw, ow, oh)
// Not part of the library.
#pragma once
#include <vector>

#include "../../qoi_amd/csrc/qoi_cubic_core.h"
#include "host_mem.h"
#include "host_sink.h"

namespace hostmem {

const uint16_t kPoison = 0xFFFFu;        // no table entry: q + bias stays below it for both filters (cubic: at most 6 * 2^13, Lanczos: 42130)

// The tables of a tile as the kernel's LDS holds them: every entry of the columns and rows the tile holds written once, nothing else.
template <class F>
struct Tables {
    std::vector<uint16_t> qx, qy;
    Tables() : qx(F::kColSlots), qy(F::kRowSlots) {}
    bool fill(const qoimi::CubicTile& t, const qoimi::ResizeGeom& g) {
        if ((uint64_t)t.nx * t.sx > qx.size() || (uint64_t)t.ny * t.sy > qy.size()) return false;
        qx.assign(qx.size(), kPoison); qy.assign(qy.size(), kPoison);
        for (uint32_t i = 0; i < t.nx + t.ny; ++i) F::norm(t, g, i, qx.data(), qy.data());
        for (size_t i = 0; i < qx.size(); ++i) if ((qx[i] == kPoison) != (i >= (size_t)t.nx * t.sx)) return false;
        for (size_t i = 0; i < qy.size(); ++i) if ((qy[i] == kPoison) != (i >= (size_t)t.ny * t.sy)) return false;
        return true;
    }
};

template <class F, class Mem>
void pixel_sums(const Mem& mem, const qoimi::ResizeGeom& g, const qoimi::CubicTile& t, const Tables<F>& tb, uint32_t lg, uint32_t c, uint64_t o, uint32_t X, uint32_t Y,
                bool wgt, qoimi::ResizeSums& sum) {
    sum = qoimi::ResizeSums{{0, 0, 0, 0}, {0, 0, 0}};
    const uint16_t* qx = tb.qx.data() + (size_t)qoimi::cubic_tile_slot(t, o, X) * t.sx;
    const uint16_t* qy = tb.qy.data() + (size_t)(Y - t.Y0) * t.sy;
    for (uint32_t l = 0; l < (1u << lg); ++l) {
        qoimi::ResizeSums s;
        if (wgt) F::template lane<true>(mem, g, qx, qy, t.sy, X, Y, l, c, s);
        else F::template lane<false>(mem, g, qx, qy, t.sy, X, Y, l, c, s);
        for (int k = 0; k < 4; ++k) sum.S[k] += s.S[k];
        for (int k = 0; k < 3; ++k) sum.W[k] += s.W[k];
    }
}

// One item as the filter's kernel walks it with a u8 HWC format: stage holds stage_px pixels (rows of w), the output of ow * oh * och bytes
// begins at out[q - base].  writes[i] counts the stores to out[i].  Returns the loads made, or -1 - the number of bad accesses if there was
// one (a table that does not fit or is not written exactly counts as one); *tiles_walked reports the tiles, *normalised the columns and rows
// normalised over all tiles.
template <class F>
long long table_filter_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                           uint32_t flags, uint32_t och, int weighted, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len,
                           unsigned long long* tiles_walked, unsigned long long* normalised) {
    long long bad = 0, loads = 0;
    const StagedMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, &loads};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, flags};
    const qoimi::TensorSink sink = tensor_sink_u8_hwc();
    uint32_t lg, c;
    F::split(cw, ow, lg, c);
    const uint64_t tiles = F::tiles(cw, ow, oh);
    const bool wgt = weighted != 0 && och == 4u;
    unsigned long long norm = 0;
    Tables<F> tb;
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        const qoimi::CubicTile t = F::tile(g, lg, c, tile);
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
    return checked(bad, loads);
}

// Output pixel (X, Y) of the unflipped result of an item over synthetic staged pixels (rows of w, stage_px of them), 4 channels, written as
// one dword to *px; sums[0..6] receive N_r, N_g, N_b, N_a, M_r, M_g, M_b (signed).  Returns the loads, or -1 - bad accesses.
template <class F>
long long table_filter_pixel(uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, int weighted,
                             uint32_t X, uint32_t Y, uint32_t* px, long long* sums) {
    long long bad = 0, loads = 0, stores = 0;
    const SynthMem mem = {stage_px, px, &bad, &loads, &stores};
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, 0u};
    const qoimi::TensorSink sink = tensor_sink_u8_hwc();
    uint32_t lg, c;
    F::split(cw, ow, lg, c);
    const uint64_t o = (uint64_t)Y * ow + X;
    const qoimi::CubicTile t = F::tile(g, lg, c, o / (qoimi::kResizeThreads >> lg));
    Tables<F> tb;
    if (!tb.fill(t, g)) return -1;
    qoimi::ResizeSums sum;
    pixel_sums(mem, g, t, tb, lg, c, o, X, Y, weighted != 0, sum);
    sink(mem, g, 0u, 4u, X, Y, qoimi::cubic_pixel(sum, weighted != 0));
    for (int k = 0; k < 4; ++k) sums[k] = (long long)sum.S[k];
    for (int k = 0; k < 3; ++k) sums[4 + k] = (long long)sum.W[k];
    if (stores != 1) ++bad;
    return checked(bad, loads);
}

}  // namespace hostmem

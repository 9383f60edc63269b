// mode_host.cpp — qoimi_decode_tensors with QOIMI_FILTER_MODE (qoi_amd/csrc/qoi_mode_core.h: mode_hold, mode_meet, mode_best, mode_pick; the
// store end: qoi_tensor_core.h: TensorSink) compiled for the host: the walk of tensor_mode over an item, tile by tile, with the lanes of a
// tile walked in a loop - where the kernel moves pixels between lanes (__shfl of width L, __shfl_xor) this file reads the other lane's
// entry of an array of 256 - over a synthetic staging array and the checking memory functor of host_mem.h (RectMem).
// tests/test_mode_core_host.py compares it with the Python models without a GPU.  With -DMODE_HOST_MAIN the same source is a stand-alone program that walks a grid of
// items against a plain counting loop (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_mode_core.h"
#include "host_mem.h"
#include "host_sink.h"

namespace {

// One tile as the kernel runs it: every one of the 256 lanes takes every step, whether its output pixel exists or not.
template <class Sink>
void mode_tile(const hostmem::RectMem& mem, const qoimi::ResizeGeom& g, uint64_t q, uint32_t och, uint32_t lg, uint64_t tile, const Sink& sink) {
    using namespace qoimi;
    const uint32_t L = 1u << lg;
    ModeHeld h[kResizeThreads];
    uint32_t count[kResizeThreads][kModeHold];
    uint64_t best[kResizeThreads], next[kResizeThreads];
    uint32_t X[kResizeThreads], Y[kResizeThreads];
    bool valid[kResizeThreads];
    for (uint32_t t = 0; t < kResizeThreads; ++t) {
        const uint64_t item = tile * kResizeThreads + t, o = item >> lg;
        valid[t] = o < (uint64_t)g.ow * g.oh;
        Y[t] = valid[t] ? (uint32_t)o / g.ow : 0u;
        X[t] = valid[t] ? (uint32_t)o - Y[t] * g.ow : 0u;
        if (valid[t]) mode_hold(mem, g, X[t], Y[t], (uint32_t)item & (L - 1u), lg, h[t]);
        else mode_none(h[t]);
        for (uint32_t j = 0; j < kModeHold; ++j) count[t][j] = 0u;
    }
    for (uint32_t s = 0; s < L; ++s)                                  // (s = 0: the lane's own pixels)
        for (uint32_t t = 0; t < kResizeThreads; ++t) {
            const uint32_t other = (t & ~(L - 1u)) | ((t + s) & (L - 1u));   // __shfl(., l + s, L)
            mode_meet(h[t], h[other].v, h[other].n, count[t]);
        }
    for (uint32_t t = 0; t < kResizeThreads; ++t) best[t] = mode_best(h[t], count[t]);
    for (uint32_t step = 1u; step < L; step <<= 1) {                  // __shfl_xor(., step)
        for (uint32_t t = 0; t < kResizeThreads; ++t) next[t] = best[t ^ step] > best[t] ? best[t ^ step] : best[t];
        for (uint32_t t = 0; t < kResizeThreads; ++t) best[t] = next[t];
    }
    for (uint32_t t = 0; t < kResizeThreads; ++t)
        if (valid[t] && (t & (L - 1u)) == 0u) sink(mem, g, q, och, X[t], Y[t], mode_pick(best[t]));
}

}  // namespace

extern "C" {

// One item as tensor_mode walks it: stage holds stage_px pixels (rows of w), the tensor begins at out[q - base]; flags: the item's flips;
// lg: mode_split's, or another one the caller forces (a lane must still hold every pixel of its share: cells <= 4 << lg); the format as
// the call's.  writes[i] counts the stores to out[i].  Returns the loads made, or -1 - the number of bad accesses if there was one.
long long mode_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                        uint32_t flags, uint32_t och, uint32_t lg, uint32_t dtype, uint32_t layout, const float* scale, const float* bias, uint64_t q, uint64_t base,
                        uint8_t* out, uint8_t* writes, uint64_t out_len) {
    long long bad = 0, loads = 0;
    const hostmem::RectMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, w, x, y, cw, rh, &loads};
    const qoimi::TensorSink sink = hostmem::tensor_sink(dtype, layout, scale, bias);
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, flags};
    const uint64_t tiles = ((((uint64_t)ow * oh) << lg) + qoimi::kResizeThreads - 1u) / qoimi::kResizeThreads;
    for (uint64_t tile = 0; tile < tiles; ++tile) mode_tile(mem, g, q, och, lg, tile, sink);
    return hostmem::checked(bad, loads);
}

uint64_t mode_host_tiles(uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh) { return qoimi::mode_tiles(cw, rh, ow, oh); }
uint32_t mode_host_split(uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh) { uint32_t lg, c; qoimi::mode_split(cw, rh, ow, oh, lg, c); return lg | (c << 8); }
uint32_t mode_host_first(uint32_t Z, uint32_t n_src, uint32_t n_out) { return qoimi::mode_first(Z, n_src, n_out); }
uint32_t mode_host_range(uint32_t Z, uint32_t n_src, uint32_t n_out) { uint32_t lo, n; qoimi::mode_range(Z, n_src, n_out, lo, n); return lo | (n << 16); }
uint64_t mode_host_word(uint32_t count, uint32_t centre, uint32_t px) { return qoimi::mode_word(count, centre != 0u, px); }
uint32_t mode_host_pick(uint64_t word) { return qoimi::mode_pick(word); }
uint32_t mode_host_max_ratio() { return qoimi::kModeMaxRatio; }
uint32_t mode_host_max_size() { return qoimi::kModeMaxSize; }

}

#ifdef MODE_HOST_MAIN
#include <stdio.h>
#include <string.h>

// The winner of a cell by plain counting over the cell's pixels, the cell found by the centre inequality and not by first()
static uint32_t plain_vote(const std::vector<uint32_t>& stage, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, uint32_t X, uint32_t Y) {
    std::vector<uint32_t> px;
    const uint32_t kc = (uint32_t)(((2ull * X + 1u) * cw) / (2ull * ow)), rc = (uint32_t)(((2ull * Y + 1u) * rh) / (2ull * oh));
    std::vector<uint32_t> ks, rs;
    for (uint32_t k = 0; k < cw; ++k) if (2ull * X * cw <= (2ull * k + 1u) * ow && (2ull * k + 1u) * ow < 2ull * (X + 1u) * cw) ks.push_back(k);
    for (uint32_t r = 0; r < rh; ++r) if (2ull * Y * rh <= (2ull * r + 1u) * oh && (2ull * r + 1u) * oh < 2ull * (Y + 1u) * rh) rs.push_back(r);
    if (ks.empty()) ks.push_back(kc);
    if (rs.empty()) rs.push_back(rc);
    for (uint32_t r : rs) for (uint32_t k : ks) px.push_back(stage[(size_t)(y + r) * w + x + k]);
    const uint32_t centre = stage[(size_t)(y + rc) * w + x + kc];
    size_t top = 0;
    for (uint32_t a : px) { size_t n = 0; for (uint32_t b : px) n += a == b; if (n > top) top = n; }
    bool have = false, centre_wins = false; uint32_t low = 0; uint64_t low_key = 0;
    for (uint32_t a : px) {
        size_t n = 0; for (uint32_t b : px) n += a == b;
        if (n != top) continue;
        const uint64_t key = ((uint64_t)(a & 255u) << 24) | ((a >> 8 & 255u) << 16) | ((a >> 16 & 255u) << 8) | (a >> 24);
        if (a == centre) centre_wins = true;
        if (!have || key < low_key) { have = true; low = a; low_key = key; }
    }
    return centre_wins ? centre : low;
}

// Label maps of 2 to 5 classes (so that votes, ties and lowest keys all happen) with rectangles at odd corners, every lg the split
// chooses and one above it, both flips, both och, a set of dtypes, layouts and alignments - in arrays of exactly the size the walk may
// touch: the staging ends with the rectangle's last row, the output with its guard band.
int main() {
    using hostmem::Case;
    const Case cases[] = {{1, 1, 0, 0, 1, 1, 1, 1}, {1, 1, 0, 0, 1, 1, 7, 5}, {37, 29, 0, 0, 37, 29, 9, 7}, {37, 29, 3, 5, 31, 23, 50, 7}, {37, 29, 1, 2, 33, 25, 5, 41},
                          {70, 45, 0, 0, 70, 45, 16, 11}, {70, 45, 5, 3, 64, 40, 32, 20}, {70, 45, 3, 1, 64, 44, 4, 3}, {64, 48, 0, 0, 64, 48, 4, 3}, {130, 3, 1, 0, 129, 3, 9, 1},
                          {3, 130, 0, 1, 3, 129, 1, 9}, {40, 40, 1, 1, 37, 37, 37, 37}, {300, 2, 0, 0, 300, 2, 19, 1}};
    const uint32_t formats[][2] = {{0, 0}, {6, 3}, {5, 1}, {1, 0}};
    const float one[4] = {1.f, 1.f, 1.f, 1.f}, zero[4] = {0.f, 0.f, 0.f, 0.f};
    const uint64_t base = 4096, guard = 32;
    long long items = 0;
    uint32_t seed = 12345u;
    for (const Case& c : cases) {
        std::vector<uint32_t> stage((size_t)c.w * (c.y + c.rh));
        const uint32_t classes = 2u + (c.w + c.h) % 4u;
        for (size_t i = 0; i < stage.size(); ++i) { seed = seed * 1664525u + 1013904223u; stage[i] = 0xFF000000u | ((seed >> 24) % classes) * 0x010203u; }
        uint32_t lg0, cc;
        qoimi::mode_split(c.cw, c.rh, c.ow, c.oh, lg0, cc);
        for (uint32_t lg = lg0; lg <= lg0 + 1u && lg <= qoimi::kModeMaxLg; ++lg)
            for (const auto& f : formats)
                for (uint32_t och = 3; och <= 4; ++och)
                    for (uint32_t flags = 0; flags < 4; ++flags) {
                        const uint32_t dtype = f[0], layout = f[1], elem = qoimi::tensor_elem(dtype), n = layout == 3u ? 1u : och, a = elem * (flags + 1u) % 16u;
                        const uint64_t B = (uint64_t)c.ow * c.oh * n * elem;
                        std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                        const long long rc = mode_host_run(stage.data(), stage.size(), c.w, c.x, c.y, c.cw, c.rh, c.ow, c.oh, flags, och, lg, dtype, layout, one, zero,
                                                           base + guard + a, base, out.data(), writes.data(), out.size());
                        if (rc < 0) { printf("%lld bad accesses: %ux%u -> %ux%u lg %u dtype %u layout %u\n", -1 - rc, c.cw, c.rh, c.ow, c.oh, lg, dtype, layout); return 1; }
                        const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                        if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                        if (dtype == 1u) { ++items; continue; }         // (binary16: the stores are checked, the values by the Python test)
                        for (uint32_t Y = 0; Y < c.oh; ++Y)
                            for (uint32_t X = 0; X < c.ow; ++X) {
                                const uint32_t px = plain_vote(stage, c.w, c.x, c.y, c.cw, c.rh, c.ow, c.oh, X, Y);
                                for (uint32_t ch = 0; ch < n; ++ch) {
                                    const size_t idx = hostmem::element_index(layout == 1u, flags, c.ow, c.oh, n, X, Y, ch);
                                    uint64_t got = 0;
                                    memcpy(&got, &out[guard + a + idx * elem], elem);
                                    if (got != ((px >> (8u * ch)) & 255u)) {
                                        printf("wrong element: %ux%u -> %ux%u lg %u dtype %u layout %u och %u flags %u at (%u, %u).%u\n", c.cw, c.rh, c.ow, c.oh, lg, dtype, layout, och, flags, X, Y, ch);
                                        return 1;
                                    }
                                }
                            }
                        ++items;
                    }
    }
    printf("mode_host: %lld items ok\n", items);
    return 0;
}
#endif

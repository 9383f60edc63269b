// nearest_host.cpp — qoimi_decode_tensors with QOIMI_FILTER_NEAREST (qoi_amd/csrc/qoi_nearest_core.h: nearest_work; the store end:
// qoi_tensor_core.h: TensorSink with the integer dtypes and the one-plane layout) compiled for the host: the walk of tensor_nearest over an
// item, tile by tile and work item by work item, over a synthetic staging array and the checking memory functor of host_mem.h (RectMem), so
// that tests/test_labels_core_host.py can compare it with the Python models without a GPU.  With -DNEAREST_HOST_MAIN the same source is a
// stand-alone program that walks a grid of items against a plain double loop (the test builds it with -fsanitize=address,undefined and runs
// it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_nearest_core.h"
#include "host_mem.h"
#include "host_sink.h"

extern "C" {

// One item as tensor_nearest walks it: stage holds stage_px pixels (rows of w), the tensor begins at out[q - base]; flags: the item's flips;
// the format as the call's.  writes[i] counts the stores to out[i].  Returns the loads made, or -1 - the number of bad accesses if there was
// one.
long long nearest_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh,
                           uint32_t flags, uint32_t och, uint32_t dtype, uint32_t layout, const float* scale, const float* bias, uint64_t q, uint64_t base,
                           uint8_t* out, uint8_t* writes, uint64_t out_len) {
    long long bad = 0, loads = 0;
    const hostmem::RectMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, w, x, y, cw, rh, &loads};
    const qoimi::TensorSink sink = hostmem::tensor_sink(dtype, layout, scale, bias);
    const qoimi::ResizeGeom g = {w, x, y, cw, rh, ow, oh, flags};
    const uint64_t tiles = qoimi::nearest_tiles(cw, ow, oh);
    for (uint64_t tile = 0; tile < tiles; ++tile)
        for (uint32_t t = 0; t < qoimi::kResizeThreads; ++t) qoimi::nearest_work(mem, g, q, och, tile * qoimi::kResizeThreads + t, sink);
    return hostmem::checked(bad, loads);
}

uint64_t nearest_host_tiles(uint32_t cw, uint32_t ow, uint32_t oh) { return qoimi::nearest_tiles(cw, ow, oh); }
uint32_t nearest_host_index(uint32_t Z, uint32_t n_src, uint32_t n_out) { return qoimi::nearest_index(Z, n_src, n_out); }
uint32_t nearest_host_elem(uint32_t dtype) { return qoimi::tensor_elem(dtype); }
uint32_t nearest_host_max_size() { return qoimi::kNearestMaxSize; }

}

#ifdef NEAREST_HOST_MAIN
#include <stdio.h>
#include <string.h>

// The element of the value v = 0..255 under scale 1 and bias 0, another way: every such value is exact in all four float formats
static uint64_t plain_element(uint32_t v, uint32_t dtype) {
    if (dtype == qoimi::kTensorU8 || dtype == qoimi::kTensorI32 || dtype == qoimi::kTensorI64) return v;
    if (v == 0u) return 0u;
    uint32_t e = 0;
    while ((v >> (e + 1u)) != 0u) ++e;                               // 2^e <= v < 2^(e + 1), e <= 7
    if (dtype == qoimi::kTensorF16) return ((e + 15u) << 10) | ((v << (10u - e)) & 0x3FFu);
    const uint32_t f32 = ((e + 127u) << 23) | ((v << (23u - e)) & 0x7FFFFFu);
    return dtype == qoimi::kTensorF32 ? f32 : f32 >> 16;
}

// Sources of 1 x 1, 1 x 130, 37 x 29 and 70 x 45 with rectangles at odd corners; outputs that enlarge, reduce by 100 and more and hit exact
// boundaries; every flip, och, dtype and layout, a set of alignments - in arrays of exactly the size the walk may touch: the staging ends
// with the rectangle's last row, the output with its guard band.
int main() {
    using hostmem::Case;
    const Case cases[] = {{1, 1, 0, 0, 1, 1, 1, 1}, {1, 1, 0, 0, 1, 1, 7, 5}, {1, 130, 0, 3, 1, 127, 1, 1}, {1, 130, 0, 0, 1, 130, 3, 257}, {130, 1, 1, 0, 129, 1, 1, 1},
                          {37, 29, 3, 5, 31, 23, 50, 41}, {37, 29, 1, 1, 2, 14, 41, 23}, {37, 29, 0, 0, 37, 29, 37, 29}, {70, 45, 5, 3, 63, 41, 3, 2},
                          {70, 45, 7, 1, 60, 40, 20, 8}, {16384, 1, 1, 0, 16383, 1, 2, 1}, {300, 2, 0, 0, 300, 2, 3, 1}};
    const uint32_t dtypes[] = {0, 1, 2, 3, 5, 6}, layouts[] = {0, 1, 3};
    const float one[4] = {1.f, 1.f, 1.f, 1.f}, zero[4] = {0.f, 0.f, 0.f, 0.f};
    const uint64_t base = 4096, guard = 32;
    long long items = 0;
    for (const Case& c : cases) {
        std::vector<uint32_t> stage((size_t)c.w * (c.y + c.rh));
        for (size_t i = 0; i < stage.size(); ++i) stage[i] = (uint32_t)(i * 2654435761u + 12345u);
        for (uint32_t dtype : dtypes)
            for (uint32_t layout : layouts)
                for (uint32_t och = 3; och <= 4; ++och)
                    for (uint32_t flags = 0; flags < 4; ++flags) {
                        const uint32_t elem = nearest_host_elem(dtype), n = layout == 3u ? 1u : och;
                        for (uint32_t a = 0; a < 16u; a += (elem == 1u ? 3u : elem) * ((dtype + flags) % 3u + 1u)) {
                            const uint64_t B = (uint64_t)c.ow * c.oh * n * elem;
                            std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                            const long long rc = nearest_host_run(stage.data(), stage.size(), c.w, c.x, c.y, c.cw, c.rh, c.ow, c.oh, flags, och, dtype, layout, one, zero,
                                                                  base + guard + a, base, out.data(), writes.data(), out.size());
                            if (rc != (long long)c.ow * c.oh) { printf("%lld loads or bad accesses: %ux%u -> %ux%u dtype %u layout %u\n", rc, c.cw, c.rh, c.ow, c.oh, dtype, layout); return 1; }
                            const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                            if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                            for (uint32_t Y = 0; Y < c.oh; ++Y)
                                for (uint32_t X = 0; X < c.ow; ++X) {
                                    const uint64_t k = ((2ull * X + 1u) * c.cw) / (2ull * c.ow), r = ((2ull * Y + 1u) * c.rh) / (2ull * c.oh);
                                    const uint32_t px = stage[(size_t)(c.y + r) * c.w + c.x + k];
                                    for (uint32_t ch = 0; ch < n; ++ch) {
                                        const size_t idx = hostmem::element_index(layout == 1u, flags, c.ow, c.oh, n, X, Y, ch);
                                        uint64_t got = 0;
                                        memcpy(&got, &out[guard + a + idx * elem], elem);
                                        if (got != plain_element((px >> (8u * ch)) & 255u, dtype)) {
                                            printf("wrong element: %ux%u -> %ux%u dtype %u layout %u och %u flags %u at (%u, %u).%u\n", c.cw, c.rh, c.ow, c.oh, dtype, layout, och, flags, X, Y, ch);
                                            return 1;
                                        }
                                    }
                                }
                            ++items;
                        }
                    }
    }
    printf("nearest_host: %lld items ok\n", items);
    return 0;
}
#endif

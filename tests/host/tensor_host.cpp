// tensor_host.cpp — the store end of qoimi_decode_tensors / qoimi_decode_warped_tensors (qoi_amd/csrc/qoi_tensor_core.h) compiled for the host:
// every pixel of an output handed to TensorSink as the filter tiles and the warp tile hand it over, with the store half of host_mem.h (StoreMem), which checks and counts
// every store, so that tests/test_tensor_core_host.py can compare it with qoi_amd/tensors.py without a GPU.  With -DTENSOR_HOST_MAIN the same
// source is a stand-alone program that walks a grid of formats against a plain loop (the test builds it with -fsanitize=address,undefined and
// runs it).  Not part of the library.
#include "host_mem.h"
#include "host_sink.h"

extern "C" {

// px holds the ow * oh pixels of the UNFLIPPED result as r | g << 8 | b << 16 | a << 24, row-major; each is handed to the sink at (X, Y) with
// the item's flags (warp != 0: through the warp tile's overload, which knows no flips).  The tensor begins at out[q - base]; writes[i] counts
// the stores to out[i].  Returns the stores made, or -1 - the number of bad stores if there was one.
long long tensor_host_run(const uint32_t* px, uint32_t ow, uint32_t oh, uint32_t och, uint32_t flags, int warp, uint32_t dtype, uint32_t layout,
                          const float* scale, const float* bias, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len) {
    long long bad = 0, stores = 0;
    const hostmem::StoreMem mem = {out, writes, out_len, base, &bad, &stores};
    const qoimi::TensorSink sink = hostmem::tensor_sink(dtype, layout, scale, bias);
    const qoimi::ResizeGeom rg = {ow, 0u, 0u, ow, oh, ow, oh, flags};
    const qoimi::WarpGeom wg = {ow, 0u, 0u, ow, oh, ow, oh, 0u, 65536, 0, 0, 65536, 0u, 0, 0};
    for (uint32_t Y = 0; Y < oh; ++Y)
        for (uint32_t X = 0; X < ow; ++X) {
            if (warp) sink(mem, wg, q, och, X, Y, px[(uint64_t)Y * ow + X]);
            else sink(mem, rg, q, och, X, Y, px[(uint64_t)Y * ow + X]);
        }
    return hostmem::checked(bad, stores);
}

// The bits tensor_value stores for the channel value v
uint32_t tensor_host_value(uint32_t v, float scale, float bias, uint32_t dtype) { return qoimi::tensor_value(v, scale, bias, dtype); }

uint32_t tensor_host_f16(uint32_t bits) { return qoimi::tensor_f16(bits); }
uint32_t tensor_host_bf16(uint32_t bits) { return qoimi::tensor_bf16(bits); }
uint32_t tensor_host_elem(uint32_t dtype) { return qoimi::tensor_elem(dtype); }

}  // extern "C"

#if defined(TENSOR_HOST_MAIN)
#include <math.h>
#include <stdio.h>
#include <string.h>

// The value another way: the product through a volatile, binary16 through the math library
static uint32_t plain_value(uint32_t v, float scale, float bias, uint32_t dtype) {
    if (dtype == qoimi::kTensorU8) return v;
    volatile float m = (float)v * scale;
    const float s = m + bias;
    uint32_t u;
    memcpy(&u, &s, 4);
    if (dtype == qoimi::kTensorF32) return u;
    if (dtype == qoimi::kTensorBF16) return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    // binary16 through the math library: the nearest multiple of the quantum at s's exponent, ties to even (nearbyint in the default mode)
    const uint32_t sign = (u >> 16) & 0x8000u;
    const double x = fabs((double)s);
    if (x >= 65520.0) return sign | 0x7C00u;
    if (x == 0.0) return sign;
    const int e = ilogb(x) < -14 ? -14 : ilogb(x);
    const double value = nearbyint(ldexp(x, 10 - e)) * ldexp(1.0, e - 10);
    if (value < ldexp(1.0, -14)) return sign | (uint32_t)ldexp(value, 24);
    const int e2 = ilogb(value);
    return sign | (((uint32_t)(e2 + 15) << 10) + ((uint32_t)ldexp(value, 10 - e2) - 1024u));
}

int main() {
    const float scales[][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f / 255.f, 0.017124753f, 0.017507004f, 0.25f}, {300.f, 1e-6f, 2.4e-8f, 1e-40f}, {-257.f, 65504.f / 255.f, 1e30f, 3e38f}};
    const float biases[][4] = {{0.f, 0.f, 0.f, 0.f}, {-2.117904f, -2.0357144f, -1.8044444f, -0.f}, {-300.f, 6e-8f, -1e-41f, 0.f}, {65535.f, 16.f, -1e30f, 3e38f}};
    long long items = 0;
    for (uint32_t dtype = 0; dtype < 4u; ++dtype)
        for (uint32_t layout = 0; layout < 2u; ++layout)
            for (uint32_t och = 3; och <= 4u; ++och)
                for (uint32_t flags = 0; flags < 4u; ++flags)
                    for (int warp = 0; warp < 2; ++warp)
                        for (size_t k = 0; k < 4u; ++k) {
                            if (dtype == qoimi::kTensorU8 && k != 0u) continue;
                            const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {17, 16}};
                            for (const auto& wh : sizes) {
                                const uint32_t ow = wh[0], oh = wh[1], elem = qoimi::tensor_elem(dtype);
                                std::vector<uint32_t> px((size_t)ow * oh);
                                for (size_t i = 0; i < px.size(); ++i) px[i] = (uint32_t)(i * 2654435761u + 12345u * k);
                                const size_t B = (size_t)ow * oh * och * elem, band = 32;
                                for (uint32_t a = 0; a < 16u; a += elem) {
                                    std::vector<uint8_t> out(band + a + B + band, hostmem::kGuard), writes(out.size(), 0);
                                    const uint64_t base = 1u << 20;
                                    if (tensor_host_run(px.data(), ow, oh, och, flags, warp, dtype, layout, scales[k], biases[k], base + band + a, base, out.data(),
                                                        writes.data(), out.size()) < 0) { printf("bad store\n"); return 1; }
                                    const long long off = hostmem::first_miswritten(out, writes, band + a, B);
                                    if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                                    for (uint32_t Y = 0; Y < oh; ++Y)
                                        for (uint32_t X = 0; X < ow; ++X)
                                            for (uint32_t c = 0; c < och; ++c) {
                                                const size_t idx = hostmem::element_index(layout != 0u, warp ? 0u : flags, ow, oh, och, X, Y, c);
                                                uint32_t got = 0;
                                                memcpy(&got, &out[band + a + idx * elem], elem);
                                                const uint32_t want = plain_value((px[(size_t)Y * ow + X] >> (8u * c)) & 255u, scales[k][c], biases[k][c], dtype);
                                                if (got != want) { printf("dtype %u layout %u och %u k %zu (%u, %u, %u): %08x, not %08x\n", dtype, layout, och, k, X, Y, c, got, want); return 1; }
                                            }
                                    ++items;
                                }
                            }
                        }
    printf("tensor_host: %lld items ok\n", items);
    return 0;
}
#endif

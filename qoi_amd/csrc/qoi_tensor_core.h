// qoi_tensor_core.h — the store end of qoimi_decode_tensors and qoimi_decode_warped_tensors: one rounded pixel of a filter tile or of the warp
// tile, still in a register, to the elements of a tensor - u8, binary16, bfloat16 or binary32, interleaved or planar, scaled and shifted per
// channel; or, for label maps, 32- or 64-bit integers, and the first channel alone as one plane.
//
// The definition (normative; qoi_amd/tensors.py: convert states it in Python).  px = r | g << 8 | b << 16 | a << 24 is the pixel the u8 call
// would store at pixel (xo, yo) of an ow x oh output with och = 3 or 4 channels; v = channel c of it, an integer 0..255.
//   U8              the element is v (the host accepts only scale 1 and bias +0)
//   F32             t = float(v); m = t * scale[c], rounded to nearest even in binary32; s = m + bias[c], rounded to nearest even in binary32 -
//                   TWO roundings, never a fused multiply-add; the element is s
//   F16, BF16       s converted to binary16 / bfloat16, round to nearest even
//   I32, I64        the element is v as a little-endian two's-complement integer of 4 / 8 bytes (the host accepts only scale 1 and bias +0)
// Subnormals are kept in every format, a result too large becomes infinity; scale and bias are finite, so no NaN arises.
// The element is stored at element index (yo * ow + xo) * och + c (HWC) or (c * oh + yo) * ow + xo (CHW) from the absolute address q, which is a
// multiple of the element size: every store is one whole, naturally aligned element - the item's own bytes only, never a word that would have
// to be read first.  Where u8 HWC holds 4 bytes per pixel and the address is aligned the pixel is one dword, as resize_store writes it.
// With HW only channel 0 (r) of a pixel is stored, at element index yo * ow + xo: one plane of ow * oh elements; och still says how the image
// was decoded.  An 8-byte element is two aligned dword stores, the value at a and 0 at a + 4 (Mem has no 8-byte store).
// With HW_ID24 (I32 and I64 only, the host sees to it) the one element of a pixel, at element index yo * ow + xo, is r | g << 8 | b << 16 = px & 0xFFFFFF,
// the 24-bit id of the COCO panoptic convention; alpha is ignored: the dword at a, and 0 at a + 4 for I64.
//
// Plain sequential code over a memory functor `Mem` (store1 / store2 / store4(address, value)), compiled for the device by hipcc
// (qoi_tensor.hip: the conversions are the hardware's) and - by tests/host/tensor_host.cpp only - for the host, where the narrowing is integer
// arithmetic on the binary32 bits and the functor checks every store.
#pragma once
#include <stdint.h>

#include "qoi_warp_core.h"

namespace qoimi {

constexpr uint32_t kTensorU8 = 0, kTensorF16 = 1, kTensorBF16 = 2, kTensorF32 = 3, kTensorI32 = 5, kTensorI64 = 6;   // (4 is not a dtype)
constexpr uint32_t kTensorHWC = 0, kTensorCHW = 1, kTensorHW = 3;                                                    // (2 is not a layout)
constexpr uint32_t kTensorHWId24 = 5;                                                                                // (nor is 4)

// What the kernels take by value: ten dwords (qoimi_tensor_format without its reserved words)
struct TensorFormat { uint32_t dtype, layout; float scale[4], bias[4]; };

// Bytes of an element
QOIMI_RESIZE_HD uint32_t tensor_elem(uint32_t dtype) {
    if (dtype == kTensorI64) return 8u;
    return dtype == kTensorU8 ? 1u : ((dtype == kTensorF32 || dtype == kTensorI32) ? 4u : 2u);
}

// The integer dtypes: the element is the channel value itself
QOIMI_RESIZE_HD bool tensor_integer(uint32_t dtype) { return dtype == kTensorU8 || dtype == kTensorI32 || dtype == kTensorI64; }

QOIMI_RESIZE_HD uint32_t tensor_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// v * scale + bias with both roundings
QOIMI_RESIZE_HD float tensor_affine(uint32_t v, float scale, float bias) {
#if defined(__clang__)
#pragma clang fp contract(off)                                     // (whatever the build's -ffp-contract says; HIP's __fmul_rn / __fadd_rn are plain operators that fuse)
    const float m = (float)v * scale;
    return m + bias;
#else
    float m = (float)v * scale;
    __asm__ volatile("" : "+m"(m));                                // (the product is rounded before the sum sees it: no contraction)
    return m + bias;
#endif
}

// The binary32 value with the bits x (finite or infinite) as bfloat16, round to nearest even
QOIMI_RESIZE_HD uint32_t tensor_bf16(uint32_t x) { return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16; }

// ... as binary16: normal numbers by rebiasing the exponent, below 2^-14 the subnormals, 65520 and above infinity
QOIMI_RESIZE_HD uint32_t tensor_f16(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a >= 0x38800000u) {                                        // 2^-14 and above
        if (a >= 0x47800000u) return sign | 0x7C00u;               // 2^16 and above, infinity
        uint32_t r = a - 0x38000000u;
        r += 0xFFFu + ((r >> 13) & 1u);
        r >>= 13;
        return sign | (r > 0x7C00u ? 0x7C00u : r);
    }
    const uint32_t e = a >> 23;
    if (e < 101u) return sign;                                     // below 2^-25: zero
    const uint32_t mant = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;   // 14..25: units of 2^-24
    uint32_t h = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u) != 0u)) ++h;
    return sign | h;
}

// The bits to store for the channel value v = 0..255
QOIMI_RESIZE_HD uint32_t tensor_value(uint32_t v, float scale, float bias, uint32_t dtype) {
    if (tensor_integer(dtype)) return v;                           // (I64: the low dword; the high one is 0)
    const float s = tensor_affine(v, scale, bias);
    if (dtype == kTensorF32) return tensor_bits(s);
#if defined(__HIP_DEVICE_COMPILE__)
    if (dtype == kTensorF16) { const _Float16 h = (_Float16)s; uint16_t u; __builtin_memcpy(&u, &h, 2); return u; }
    const __bf16 b = (__bf16)s; uint16_t u; __builtin_memcpy(&u, &b, 2); return u;
#else
    return dtype == kTensorF16 ? tensor_f16(tensor_bits(s)) : tensor_bf16(tensor_bits(s));
#endif
}

// Pixel px to pixel (xo, yo) - the place in the OUTPUT, flips applied - of the ow x oh tensor at q.
template <class Mem>
QOIMI_RESIZE_HD void tensor_store(const Mem& mem, const TensorFormat& fmt, uint64_t q, uint32_t och, uint32_t ow, uint32_t oh, uint32_t xo, uint32_t yo, uint32_t px) {
    const uint64_t at = (uint64_t)yo * ow + xo;
    if (fmt.dtype == kTensorU8 && fmt.layout == kTensorHWC) {
        const uint64_t a = q + at * och;
        if (och == 4u && (a & 3u) == 0u) { mem.store4(a, px); return; }
        mem.store1(a, px); mem.store1(a + 1u, px >> 8); mem.store1(a + 2u, px >> 16);
        if (och == 4u) mem.store1(a + 3u, px >> 24);
        return;
    }
    const uint32_t elem = tensor_elem(fmt.dtype);
    if (fmt.layout == kTensorHWId24) {                             // (I32 or I64: one aligned dword, or two)
        const uint64_t a = q + at * elem;
        mem.store4(a, px & 0xFFFFFFu);
        if (elem == 8u) mem.store4(a + 4u, 0u);
        return;
    }
    const uint64_t plane = (uint64_t)ow * oh;
    const uint32_t n = fmt.layout == kTensorHW ? 1u : och;         // elements of a pixel
    QOIMI_RESIZE_UNROLL
    for (uint32_t c = 0; c < 4u; ++c) {                            // (unrolled: scale[c] and bias[c] are named registers)
        if (c >= n) break;
        const uint32_t bits = tensor_value((px >> (8u * c)) & 255u, fmt.scale[c], fmt.bias[c], fmt.dtype);
        const uint64_t a = q + (fmt.layout == kTensorCHW ? c * plane + at : at * n + c) * elem;
        if (elem == 8u) { mem.store4(a, bits); mem.store4(a + 4u, 0u); }
        else if (elem == 4u) mem.store4(a, bits);
        else if (elem == 2u) mem.store2(a, bits);
        else mem.store1(a, bits);
    }
}

// The finish step of the filter tiles and of the warp tile (qoi_resize_core.h: ResizeByteSink, qoi_warp_core.h: WarpByteSink) with a tensor
// as the output.
struct TensorSink {
    TensorFormat fmt;
    template <class Mem>
    QOIMI_RESIZE_HD void operator()(const Mem& mem, const ResizeGeom& g, uint64_t q, uint32_t och, uint32_t X, uint32_t Y, uint32_t px) const {
        const uint32_t xo = (g.flags & kResizeFlipX) != 0u ? g.ow - 1u - X : X, yo = (g.flags & kResizeFlipY) != 0u ? g.oh - 1u - Y : Y;
        tensor_store(mem, fmt, q, och, g.ow, g.oh, xo, yo, px);
    }
    template <class Mem>
    QOIMI_RESIZE_HD void operator()(const Mem& mem, const WarpGeom& g, uint64_t q, uint32_t och, uint32_t X, uint32_t Y, uint32_t px) const {
        tensor_store(mem, fmt, q, och, g.ow, g.oh, X, Y, px);
    }
};

}  // namespace qoimi

// qoi_tensor.hip — qoimi_decode_tensors and qoimi_decode_warped_tensors: the resampled rectangles of qoimi_decode_resized,
// qoimi_decode_bilinear and qoimi_decode_warped written as tensors - u8, binary16, bfloat16 or binary32 elements, interleaved (HWC) or planar
// (CHW), each channel scaled and shifted - by the kernels tensor_area, tensor_tent and tensor_warp.  gfx950, wave64.  The host side:
// qoi_host_tensor.hip (qoi_kernels.h declares the launchers).
//
// The result (normative; qoi_amd/tensors.py: convert states it in Python, qoi_tensor_core.h holds the arithmetic): a pure function of the bytes
// the u8 call writes for the same items - element (Y, X, c) is float(byte) * scale[c] + bias[c] with two roundings, narrowed once.
//
//   tensor_area, tensor_tent, tensor_warp
//                 The tiles of resize_filter, bilinear_filter and warp_gather as they are (qoi_gather_tiles.h: filter_tiles, warp_walk - one
//                 body, not a copy): tables, work items, loads, sums and the one rounding to r | g << 8 | b << 16 | a << 24 in a register
//                 are theirs.  Only the finish step differs: TensorSink (qoi_tensor_core.h) unpacks the word's bytes (a bit-field extract and
//                 v_cvt_f32_ubyte0), multiplies and adds (v_mul_f32, v_add_f32 - never an fma: contraction is off there), narrows (v_cvt_f16_f32, v_cvt_pk_bf16_f32) and stores och whole,
//                 naturally aligned elements: no second pass over the output, no LDS, no second buffer, not one byte outside an item's
//                 output, never a word that would have to be read first.
//                 The format - dtype, layout, four scales, four biases: ten dwords - is a kernel argument by value, so it stands in SGPRs;
//                 dtype, layout and och are the same for every lane of a launch or of an entry: their branches are scalar.
//                 In CHW a pixel's och elements go to och planes; with L = 1 lane per pixel (every item that does not reduce) consecutive
//                 lanes hold consecutive pixels of a row, so each of the och store instructions writes consecutive elements of its plane.
#include "qoi_gather_tiles.h"
#include "qoi_tensor_core.h"

namespace qoimi {

__global__ __launch_bounds__(kResizeThreads) void tensor_area(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               uint8_t* out, TensorFormat fmt) {
    filter_tiles<AreaFilter>(stage, tab, m, tiles, out, TensorSink{fmt});
}

__global__ __launch_bounds__(kResizeThreads) void tensor_tent(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               uint8_t* out, TensorFormat fmt) {
    filter_tiles<TentFilter>(stage, tab, m, tiles, out, TensorSink{fmt});
}

__global__ __launch_bounds__(kWarpThreads) void tensor_warp(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                             uint8_t* out, TensorFormat fmt) {
    warp_walk(stage, tab, m, tiles, out, TensorSink{fmt});
}

void launch_tensor_area(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_area, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

void launch_tensor_tent(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_tent, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

void launch_tensor_warp(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, const TensorFormat& fmt, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_warp, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out, fmt);
}

}  // namespace qoimi

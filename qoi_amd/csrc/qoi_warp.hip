// qoi_warp.hip — qoimi_decode_warped: rectangles of a sub-batch of decoded images sampled through an affine map - rotation, transposition, shear,
// anisotropic scale about a point - with bilinear weights in exact integers (warp_gather).  gfx950, wave64.  The host side:
// qoi_host_staged.hip (qoi_kernels.h holds the table and declares the launcher).
//
// The result (normative; qoi_amd/warp.py: warp states it in Python, qoi_warp_core.h holds the arithmetic): image i stands in the staging arena
// as w x rows pixels of 4 bytes (the decoder's output at 4 channels down to the last row an item needs: a 256-aligned slot, every pixel an
// aligned dword); an item is a rectangle cw x rh of it and the inverse map from the pixels of an ow x oh output into the rectangle; every
// output pixel is the blend of the 2 x 2 staged pixels around its position, those outside the rectangle replaced by the nearest inside or by
// the item's fill colour, rounded once, plain or with the colours weighted by alpha, written tightly packed with och = 3 or 4 bytes per pixel
// at any byte address.
//
//   warp_gather   Work is cut over the OUTPUT in two dimensions.  A TILE is 16 x 16 output pixels of ONE item, a work item one pixel of it;
//                 thread t of the workgroup takes the pixel (t & 15, t >> 4) of its tile, so a wavefront covers 16 columns x 4 rows.  Cut
//                 row-major - 64 consecutive pixels of an output row per wavefront, as resize_filter cuts - a map that turns by 90 degrees
//                 would send the 64 lanes of every load to 64 different staged rows, the slowest shape a wave-wide load has; a 16 x 4 patch
//                 of the output is a 16 x 4 or a 4 x 16 patch of the source (or a slanted one of that size) at any angle.  The tiles of
//                 a launch are laid over the table the host builds (a WarpEntry holds its item's first tile); a workgroup takes a contiguous
//                 range of tiles (qoi_dev.h: walk_tiles), so one launch serves every item of a sub-batch.
//                 A lane computes both of its positions in 64 bits, tests the border on the 64-bit sample indices, loads up to four staged
//                 pixels as aligned dwords - plain loads: items may share source pixels; none for a sample that takes the fill or has no
//                 weight -, blends horizontally in 32 bits and vertically with one 32 x 32 -> 64 multiply-add per term, rounds with a
//                 shift (the weights of a pixel add up to 2^34) and stores the pixel (qoi_warp_core.h: warp_store): one dword where the
//                 output holds 4 bytes per pixel and the address is aligned, else 3 or 4 bytes - never a word it would have to read first,
//                 two outputs may share one.  No LDS, no barrier, no atomics; not one byte outside an item's output is written.
#include "qoi_gather_tiles.h"

namespace qoimi {

// (the tile walk: qoi_gather_tiles.h: warp_walk - tensor_warp of qoi_tensor.hip runs it too, with another finish step)
__global__ __launch_bounds__(kWarpThreads) void warp_gather(const uint8_t* __restrict__ stage, const WarpEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                             uint8_t* out) {
    warp_walk(stage, tab, m, tiles, out, WarpByteSink());
}

void launch_warp(const uint8_t* stage, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(warp_gather, dim3(grid), dim3(kWarpThreads), 0, st, stage, tab, m, tiles, out);
}

}  // namespace qoimi

// qoi_resize.hip — qoimi_decode_resized and qoimi_decode_bilinear: rectangles of a sub-batch of decoded images resampled to caller-chosen sizes
// by an exact integer area filter (resize_filter) or by an antialiased bilinear (triangle) filter in exact integers (bilinear_filter).  gfx950,
// wave64.  The host side: qoi_host_staged.hip (qoi_kernels.h holds the table and declares the launchers).
//
// The result (normative; qoi_amd/resize.py: resize and qoi_amd/bilinear.py: bilinear state it in Python, qoi_resize_core.h and
// qoi_bilinear_core.h hold the arithmetic): image i stands in the staging arena as w x rows pixels of 4 bytes (the decoder's output at 4 channels
// down to the last row an item needs: a 256-aligned slot, every pixel an aligned dword); an item is a rectangle cw x rh of it, resampled to
// ow x oh pixels - with the weights wy * wx of the overlaps, or with the weights ty * tx of the tents around the output pixel's centre
// renormalised by their sum -, rounded once, plain or with the colours weighted by alpha, rows and / or columns reversed, written tightly packed
// with och = 3 or 4 bytes per pixel at any byte address.
//
//   filter_tile   What both kernels run (qoi_gather_tiles.h; tensor_area and tensor_tent of qoi_tensor.hip run it too, with another finish step).
//                 Work is cut over the OUTPUT.  An output pixel has up to 65 x 65 staged pixels with a weight under the
//                 area filter (cw <= 64 * ow, rh <= 64 * oh), up to 64 x 64 under the tents (cw <= 32 * ow, rh <= 32 * oh; 2 x 2 when enlarging).
//                 Its columns belong to L = 1, 2, 4, 8 or 16 neighbouring lanes, chosen from the item's bound of columns per output column
//                 (resize_taps, bilinear_taps) so that a lane holds at most four of them (five for the area filter's 65); lane l takes the
//                 columns [k0 + l*c, + c) in every row with a weight.  A WORK ITEM is one lane's share; work item = (output pixel of the
//                 unflipped result, row-major) * L + l, so consecutive lanes read consecutive addresses of a staged row.  TILES of
//                 kResizeThreads work items of ONE item are laid over the table the host builds (a ResizeEntry holds its item's first tile);
//                 a workgroup takes a contiguous range of tiles (qoi_dev.h: walk_tiles), so one launch serves every item of a sub-batch.
//                 A lane computes its column weights once and a row weight per row from the closed form (no table in memory), loads its
//                 pixels as aligned dwords - plain loads: items may share source pixels - and adds weight * channel into 64-bit sums (four,
//                 seven with alpha weighting), one 32 x 32 -> 64 multiply-add each; under the tents it adds its column weights into an eighth.
//                 The L lanes of a pixel add their sums with log2(L) butterfly steps over both halves of each sum (L divides 64 and work
//                 items are numbered so that a pixel's lanes are neighbours in one wavefront); the first of them divides - by cw * rh, or by
//                 Wx * Wy: it has walked every row with a weight and holds their sum - and stores the pixel at its place, mirrored or not
//                 (qoi_resize_core.h: resize_pixel, resize_store): one dword where the output holds 4 bytes per pixel and the address is
//                 aligned, else 3 or 4 bytes - never a word it would have to read first, two outputs may share one.  No LDS, no barrier, no
//                 atomics; not one byte outside an item's output is written.
//                 The direct 2-D form of the tents takes (2s)^2 taps per pixel at a reduction s where the area filter takes s^2; a separable
//                 two-pass form is not built here.
#include "qoi_gather_tiles.h"

namespace qoimi {

__global__ __launch_bounds__(kResizeThreads) void resize_filter(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                 uint8_t* out) {
    filter_tiles<AreaFilter>(stage, tab, m, tiles, out, ResizeByteSink());
}

__global__ __launch_bounds__(kResizeThreads) void bilinear_filter(const uint8_t* __restrict__ stage, const ResizeEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                                   uint8_t* out) {
    filter_tiles<TentFilter>(stage, tab, m, tiles, out, ResizeByteSink());
}

void launch_resize(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(resize_filter, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out);
}

void launch_bilinear(const uint8_t* stage, const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(bilinear_filter, dim3(grid), dim3(kResizeThreads), 0, st, stage, tab, m, tiles, out);
}

}  // namespace qoimi

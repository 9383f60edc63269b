// qoi_crop.hip — qoimi_decode_crops: rectangles of a sub-batch of decoded images, gathered into the caller's outputs (crop_gather).  gfx950, wave64.
// The host side: qoi_host_staged.hip (qoi_kernels.h holds the table and declares the launcher).
//
// The result (normative; qoi_amd/crops.py: crop states it in Python, qoi_crop_core.h holds the arithmetic): image i stands in the staging
// arena as w x rows pixels of 4 bytes (the decoder's output at 4 channels down to the last row a crop needs: a 256-aligned slot, every pixel an
// aligned dword); a crop is its rectangle, rows and / or columns reversed, written tightly packed with och = 3 or 4 bytes per pixel at any
// byte address.
//
//   crop_gather   Work is cut over the OUTPUT in aligned 16-byte words: an ITEM is one aligned word that a crop's output touches (qoi_crop_core.h),
//                 consecutive lanes take consecutive words, so a wavefront stores one contiguous KiB and reads consecutive pixels of a source
//                 row (backwards with FLIP_X).  A lane turns its first byte into (row, column) of the crop with one division by the crop's width
//                 and steps on from there; it reads the 4 to 6 staged pixels its bytes come from as aligned dwords - plain loads: crops may
//                 share source pixels - puts the 16 bytes together with byte-align operations and stores them at once.  The first and the
//                 last word of a crop may be partial (both in one for a crop shorter than a word): such a lane writes the crop's own bytes
//                 with byte, halfword and dword stores, never a word it would have to read first - two crops may share an aligned word and
//                 are served by different lanes.  TILES of kCropThreads items of ONE crop are laid over the crop table the host builds (an
//                 entry holds its crop's first tile); a workgroup takes a contiguous range of tiles (qoi_dev.h: walk_tiles), so one launch
//                 serves every crop of a sub-batch.  No LDS, no barrier, no atomics; not one byte
//                 outside a crop's output is written.
#include "qoi_dev.h"
#include "qoi_crop_core.h"

namespace qoimi {

typedef uint32_t crop_u32x4 __attribute__((ext_vector_type(4)));

struct CropMem {
    const uint32_t* src;
    __device__ __forceinline__ uint32_t load(u64 i) const { return src[i]; }
    __device__ __forceinline__ void store1(u64 a, uint32_t v) const { *reinterpret_cast<uint8_t*>(a) = (uint8_t)v; }
    __device__ __forceinline__ void store2(u64 a, uint32_t v) const { *reinterpret_cast<uint16_t*>(a) = (uint16_t)v; }
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
    __device__ __forceinline__ void store16(u64 a, const uint32_t (&W)[4]) const {
        crop_u32x4 v; v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<crop_u32x4*>(a) = v;
    }
};

__global__ __launch_bounds__(kCropThreads) void crop_gather(const uint8_t* __restrict__ stage, const CropEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                             uint8_t* out) {
    walk_tiles(tab, m, tiles, [&](const CropEntry& e, uint32_t tile) {
        const uint32_t och = e.cfg & 255u;
        const CropRect g = {e.w, e.x, e.y, e.cw, e.ch, e.cfg >> 8};
        const CropMem mem = {reinterpret_cast<const uint32_t*>(stage + e.src_off)};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const uint32_t B = e.cw * e.ch * och;                     // (an image holds fewer than 400 000 000 pixels)
        const u64 k = (u64)tile * kCropThreads + threadIdx.x;
        if (k < crop_items(q, B)) {
            if (och == 3u) crop_item<3u>(mem, g, q, B, (uint32_t)k);
            else crop_item<4u>(mem, g, q, B, (uint32_t)k);
        }
    });
}

void launch_crop(const uint8_t* stage, const CropEntry* tab, uint32_t m, uint32_t tiles, uint8_t* out, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(crop_gather, dim3(grid), dim3(kCropThreads), 0, st, stage, tab, m, tiles, out);
}

}  // namespace qoimi

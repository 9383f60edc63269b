// qoi_ingest.hip — qoimi_encode_tiles over tensor sources (QOIMI_TILE_SRC): the tiles of a sub-batch, converted from the caller's u8 / f16 /
// bf16 / f32 tensors, interleaved or planar, into the encoder's staging.  gfx950, wave64.  The host side: qoi_host_pack.hip
// (qoi_ingest_core.h holds the conversion and the item arithmetic, qoi_kernels.h the launcher).
//
//   tensor_ingest The table and the walk of tile_gather (qoi_tile.hip); a tensor call runs this kernel in its place.  Work is cut over the
//                 OUTPUT: an item is four consecutive pixels of a tile in output order, 256 items to a tile of the walk, so a wavefront
//                 stores one contiguous KiB (och 4) or 768 bytes (och 3) of the slot as 16- or 12-byte stores, and consecutive lanes read
//                 consecutive elements of the source: per plane four elements a lane (one 4- / 8- / 16-byte load where aligned), or the
//                 pixel's elements (one 8- / 16-byte load where it has four and is aligned).  Dtype, layout and sch are the entry's: the
//                 workgroup branches once per tile of the walk, never per lane.  The conversion is a multiply (and an add that is not
//                 contracted into it), two compares and v_rndne_f32 per element.  Loads are plain.  No LDS, no barrier, no atomics;
//                 nothing of the caller's is written, and of an image nothing is read but its whole, naturally aligned elements (u8:
//                 the aligned dwords that hold one of its bytes).
#include "qoi_dev.h"
#include "qoi_ingest_core.h"

namespace qoimi {

typedef uint32_t ingest_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t ingest_u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) ingest_u32x3 { uint32_t x, y, z; };

struct IngestMem {
    __device__ __forceinline__ uint32_t load2(u64 a) const { return *reinterpret_cast<const uint16_t*>(a); }
    __device__ __forceinline__ uint32_t load4(u64 a) const { return *reinterpret_cast<const uint32_t*>(a); }
    __device__ __forceinline__ void load8(u64 a, uint32_t (&W)[2]) const {
        const ingest_u32x2 v = *reinterpret_cast<const ingest_u32x2*>(a);
        W[0] = v.x; W[1] = v.y;
    }
    __device__ __forceinline__ void load16(u64 a, uint32_t (&W)[4]) const {
        const ingest_u32x4 v = *reinterpret_cast<const ingest_u32x4*>(a);
        W[0] = v.x; W[1] = v.y; W[2] = v.z; W[3] = v.w;
    }
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
    __device__ __forceinline__ void store12(u64 a, const uint32_t (&W)[3]) const {
        ingest_u32x3 v; v.x = W[0]; v.y = W[1]; v.z = W[2];
        *reinterpret_cast<ingest_u32x3*>(a) = v;
    }
    __device__ __forceinline__ void store16(u64 a, const uint32_t (&W)[4]) const {
        ingest_u32x4 v; v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<ingest_u32x4*>(a) = v;
    }
};

template <uint32_t DT>
__device__ __forceinline__ void ingest_layout(const IngestMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t k) {
    const uint32_t sch = (e.cfg >> 16) & 15u;
    if ((e.cfg & 4u) != 0u) { if (sch == 4u) ingest_item<DT, true, 4u>(mem, e, base, q, k); else ingest_item<DT, true, 3u>(mem, e, base, q, k); }
    else { if (sch == 4u) ingest_item<DT, false, 4u>(mem, e, base, q, k); else ingest_item<DT, false, 3u>(mem, e, base, q, k); }
}

__global__ __launch_bounds__(kTileThreads) void tensor_ingest(const uint8_t* __restrict__ pixels, const TileEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               uint8_t* __restrict__ stage) {
    walk_tiles(tab, m, tiles, [&](const TileEntry& e, uint32_t tile) {
        const IngestMem mem;
        const u64 k = (u64)tile * kTileThreads + threadIdx.x;
        if (k >= ingest_items(e.cw, e.ch)) return;
        const u64 base = (u64)reinterpret_cast<uintptr_t>(pixels) + e.src_off;
        const u64 q = (u64)reinterpret_cast<uintptr_t>(stage) + e.dst_off;
        switch (e.cfg & 3u) {                                           // (the entry's: the whole workgroup takes the same way)
            case kIngestU8:   ingest_layout<kIngestU8>(mem, e, base, q, (uint32_t)k); break;
            case kIngestF16:  ingest_layout<kIngestF16>(mem, e, base, q, (uint32_t)k); break;
            case kIngestBF16: ingest_layout<kIngestBF16>(mem, e, base, q, (uint32_t)k); break;
            default:          ingest_layout<kIngestF32>(mem, e, base, q, (uint32_t)k); break;
        }
    });
}

void launch_tensor_ingest(const uint8_t* pixels, const TileEntry* tab, uint32_t m, uint32_t tiles, uint8_t* stage, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tensor_ingest, dim3(grid), dim3(kTileThreads), 0, st, pixels, tab, m, tiles, stage);
}

}  // namespace qoimi

// qoi_label.hip — qoimi_encode_tiles over label sources (QOIMI_TILE_LABELS): the tiles of a sub-batch, taken from the caller's one-plane u8 /
// int32 / int64 tensors of class indices, saturated to bytes and replicated to grey pixels on their way into the encoder's staging.
// gfx950, wave64.  The host side: qoi_host_pack.hip (qoi_label_core.h holds the conversion and the item arithmetic, qoi_kernels.h the
// launcher).
//
//   label_ingest  The table and the walk of tile_gather (qoi_tile.hip); a label call runs this kernel in its place.  Work is cut over the
//                 OUTPUT.  f == 1: tensor_ingest's items - four consecutive pixels of a tile in output order, 256 items to a tile of the
//                 walk, so a wavefront stores one contiguous KiB (och 4) or 768 bytes (och 3) of the slot as 16- or 12-byte stores, and
//                 consecutive lanes read consecutive runs of four elements of the plane: one or two dwords (u8), 16 bytes (i32) or 32 bytes
//                 (i64) a lane where the run is aligned.  f >= 2: tile_select's items.  NEAREST: a lane per output pixel loads the element
//                 at its block's centre.  MODE: L = 2^lg neighbouring lanes (the entry's) share an output pixel and hold at most four
//                 pixels of its block each; they meet and pick as tile_select's lanes do, with the functions of qoi_mode_core.h - the
//                 loop below is that kernel's cross-lane schedule, not a second vote.  Saturation is two integer compares and selects per
//                 element (i64: on the high dword, then the low), replication a multiply and an or.  Dtype, reduction and och are the
//                 entry's: the workgroup branches once per tile of the walk, never per lane, and every cross-lane operation is reached
//                 by all 256 lanes - lanes behind the tile's last pixel take part holding nothing.  Loads are plain.  No LDS, no
//                 barrier, no atomics; nothing of the caller's is written, and of a plane nothing is read but its whole, naturally aligned
//                 elements (u8: the aligned dwords that hold one of its bytes).  QOIMI_TILE_LABELS_ID24 is three more values of the
//                 entry's dtype field, so three more cases of that one branch: the same loads, items and stores, a saturation at
//                 2^24 - 1 in the place of 255 and an or in the place of the multiply.
#include "qoi_dev.h"
#include "qoi_label_core.h"

namespace qoimi {

typedef uint32_t label_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t label_u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) label_u32x3 { uint32_t x, y, z; };

struct LabelMem {
    __device__ __forceinline__ uint32_t load4(u64 a) const { return *reinterpret_cast<const uint32_t*>(a); }
    __device__ __forceinline__ void load8(u64 a, uint32_t (&W)[2]) const {
        const label_u32x2 v = *reinterpret_cast<const label_u32x2*>(a);
        W[0] = v.x; W[1] = v.y;
    }
    __device__ __forceinline__ void load16(u64 a, uint32_t (&W)[4]) const {
        const label_u32x4 v = *reinterpret_cast<const label_u32x4*>(a);
        W[0] = v.x; W[1] = v.y; W[2] = v.z; W[3] = v.w;
    }
    __device__ __forceinline__ void store1(u64 a, uint32_t v) const { *reinterpret_cast<uint8_t*>(a) = (uint8_t)v; }
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
    __device__ __forceinline__ void store12(u64 a, const uint32_t (&W)[3]) const {
        label_u32x3 v; v.x = W[0]; v.y = W[1]; v.z = W[2];
        *reinterpret_cast<label_u32x3*>(a) = v;
    }
    __device__ __forceinline__ void store16(u64 a, const uint32_t (&W)[4]) const {
        label_u32x4 v; v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<label_u32x4*>(a) = v;
    }
};

__device__ __forceinline__ u64 label_xor_max(u64 v, uint32_t step) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)step);
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}

// One tile of kTileThreads items of an entry with f == 1.
template <uint32_t DT, uint32_t ID>
__device__ __forceinline__ void label_copy(const LabelMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t tile) {
    const u64 k = (u64)tile * kTileThreads + threadIdx.x;
    if (k < ingest_items(e.cw, e.ch)) label_item<DT, ID>(mem, e, base, q, (uint32_t)k);
}

// One tile of kTileThreads items of a NEAREST entry with f >= 2: a lane per output pixel.
template <uint32_t DT, uint32_t ID>
__device__ __forceinline__ void label_nearest(const LabelMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t tile) {
    const u64 o = (u64)tile * kTileThreads + threadIdx.x;
    if (o < (u64)e.tw * e.th) label_nearest_item<DT, ID>(mem, e, base, q, (uint32_t)o);
}

// One tile of kTileThreads items of a MODE entry with f >= 2: tile_select's meeting loop and butterfly over the block.
template <uint32_t DT, uint32_t ID>
__device__ __forceinline__ void label_vote(const LabelMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t tile) {
    const uint32_t lg = e.cfg & 255u, L = 1u << lg;
    const u64 item = (u64)tile * kTileThreads + threadIdx.x, o = item >> lg;
    const uint32_t l = (uint32_t)item & (L - 1u);
    const bool valid = o < (u64)e.tw * e.th;                          // (a pixel's lanes are valid or not together)
    ModeHeld h;
    if (valid) label_vote_hold<DT, ID>(mem, e, base, (uint32_t)o, l, lg, h);
    else mode_none(h);
    uint32_t count[kModeHold] = {0u, 0u, 0u, 0u};
    mode_meet(h, h.v, h.n, count);
    for (uint32_t s = 1u; s < L; ++s) {                               // (lg is the entry's: the whole workgroup takes the same steps)
        uint32_t ov[kModeHold];
#pragma unroll
        for (uint32_t j = 0; j < kModeHold; ++j) ov[j] = (uint32_t)__shfl((int)h.v[j], (int)(l + s), (int)L);
        const uint32_t on = (uint32_t)__shfl((int)h.n, (int)(l + s), (int)L);
        mode_meet(h, ov, on, count);
    }
    u64 best = mode_best(h, count);
    for (uint32_t step = 1u; step < L; step <<= 1) best = label_xor_max(best, step);
    if (valid && l == 0u) tile_put(mem, e, q, (uint32_t)o, mode_pick(best));
}

template <uint32_t DT, uint32_t ID>
__device__ __forceinline__ void label_tile(const LabelMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t tile) {
    if (e.f == 1u) label_copy<DT, ID>(mem, e, base, q, tile);
    else if ((e.cfg & (1u << 24)) == 0u) label_nearest<DT, ID>(mem, e, base, q, tile);
    else label_vote<DT, ID>(mem, e, base, q, tile);
}

__global__ __launch_bounds__(kTileThreads) void label_ingest(const uint8_t* __restrict__ pixels, const TileEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                              uint8_t* __restrict__ stage) {
    walk_tiles(tab, m, tiles, [&](const TileEntry& e, uint32_t tile) {
        const LabelMem mem;
        const u64 base = (u64)reinterpret_cast<uintptr_t>(pixels) + e.src_off;
        const u64 q = (u64)reinterpret_cast<uintptr_t>(stage) + e.dst_off;
        switch ((e.cfg >> 16) & 15u) {                                  // (the entry's: the whole workgroup takes the same way)
            case kLabelU8:               label_tile<kLabelU8, 0u>(mem, e, base, q, tile); break;
            case kLabelI32:              label_tile<kLabelI32, 0u>(mem, e, base, q, tile); break;
            case kLabelI64:              label_tile<kLabelI64, 0u>(mem, e, base, q, tile); break;
            case kLabelId24 | kLabelU8:  label_tile<kLabelU8, 1u>(mem, e, base, q, tile); break;
            case kLabelId24 | kLabelI32: label_tile<kLabelI32, 1u>(mem, e, base, q, tile); break;
            case kLabelId24 | kLabelI64: label_tile<kLabelI64, 1u>(mem, e, base, q, tile); break;
            default: break;                                             // (label_cfg writes no other value)
        }
    });
}

void launch_label_ingest(const uint8_t* pixels, const TileEntry* tab, uint32_t m, uint32_t tiles, uint8_t* stage, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(label_ingest, dim3(grid), dim3(kTileThreads), 0, st, pixels, tab, m, tiles, stage);
}

}  // namespace qoimi

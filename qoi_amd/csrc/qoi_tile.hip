// qoi_tile.hip — qoimi_encode_tiles: the tiles of a sub-batch, gathered from the caller's images into the encoder's staging (tile_gather;
// tile_select, at the end of the file, for the label modes QOIMI_TILE_NEAREST / QOIMI_TILE_MODE).
// gfx950, wave64.  The host side: qoi_host_pack.hip (qoi_tile_core.h holds the table entry and the arithmetic, qoi_kernels.h the launcher).
//
// The result (normative; qoi_amd/tiles.py: tile states it in Python): a tile is a rectangle of an image of 3 or 4 bytes per pixel that
// stands tightly packed at ANY byte address of the caller's memory, box-reduced by f = 1..64, mirrored, written with och = 3 or 4 bytes
// per pixel into the pixel part of its slot of the staging arena - where qoimi_encode_images, as it is, encodes it from.
//
//   tile_gather   Work is cut over the OUTPUT.  TILES of kTileThreads items of ONE tile entry are laid over the table the host builds (an
//                 entry holds its first tile); a workgroup takes a contiguous range of them (qoi_dev.h: walk_tiles), so one launch serves
//                 every tile of a sub-batch, level 0 and level 6 of a pyramid alike.
//                 f == 1 (level 0: the bulk of a pyramid's bytes) is a strided copy: an item is one aligned 16-byte word of the output,
//                 consecutive lanes take consecutive words, a wavefront stores one contiguous KiB.  Where source and output both hold 4
//                 bytes per pixel and the word's four pixels are neighbours at a 16-byte aligned address, the lane loads them at once
//                 (backwards with FLIP_X); else it fetches its 4 to 6 pixels one by one - each from the one or two aligned dwords that
//                 hold it - and puts the word together with byte-align operations.  Every word is stored whole: the slot is 256-aligned
//                 and rounded up to 256 bytes.
//                 f >= 2 is thumb_reduce's lane split unchanged (qoi_thumb_core.h: a block belongs to L = 1 .. 16 neighbouring lanes, a
//                 lane takes at most four columns of every row of the block), the rectangle in the place of the image: 16-byte loads
//                 where the row pitch and the lane's first column are 16-byte aligned, else pixel by pixel; a 3-byte pixel enters the sums
//                 with alpha 255.  The L lanes add their sums with log2(L) butterfly steps, the first divides and stores the pixel where
//                 the flips put it: a dword at och == 4, three bytes at och == 3.
//                 Loads are plain: the levels of a pyramid read the same source pixels, one launch behind the other.  No LDS, no barrier,
//                 no atomics; nothing of the caller's is written, and of an image nothing is read but the aligned dwords that hold one
//                 of its bytes.
#include "qoi_dev.h"
#include "qoi_tile_core.h"

namespace qoimi {

typedef uint32_t tile_u32x4 __attribute__((ext_vector_type(4)));

struct TileMem {
    __device__ __forceinline__ uint32_t load4(u64 a) const { return *reinterpret_cast<const uint32_t*>(a); }
    __device__ __forceinline__ void load16(u64 a, uint32_t (&W)[4]) const {
        const tile_u32x4 v = *reinterpret_cast<const tile_u32x4*>(a);
        W[0] = v.x; W[1] = v.y; W[2] = v.z; W[3] = v.w;
    }
    __device__ __forceinline__ void store16(u64 a, const uint32_t (&W)[4]) const {
        tile_u32x4 v; v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<tile_u32x4*>(a) = v;
    }
};

// One tile of kTileThreads items of a reduced entry: items [item_base, item_base + kTileThreads) as far as the entry has them.
template <uint32_t SCH, bool WEIGHTED>
__device__ __forceinline__ void tile_reduce(const TileMem& mem, const TileEntry& e, u64 base, uint8_t* __restrict__ dst, uint32_t item_base) {
    const uint32_t lg = e.cfg & 255u, c = (e.cfg >> 8) & 255u, och = (e.cfg >> 20) & 15u;
    const uint32_t item = item_base + threadIdx.x;
    const ThumbShare sh = thumb_share(item, e.cw, e.ch, e.tw, e.th, e.f, lg, c);
    const bool valid = sh.o < e.tw * e.th;                        // (a block's lanes are valid or not together)
    uint32_t rb = 0, ga = 0, W[3] = {0, 0, 0};
    tile_share_sums<SCH, WEIGHTED>(mem, e, base, sh, rb, ga, W);
    uint32_t S[4] = {rb & 0xFFFFu, ga & 0xFFFFu, rb >> 16, ga >> 16};
    for (uint32_t s = 1u; s < (1u << lg); s <<= 1) {              // (lg is the entry's: the whole workgroup takes the same steps)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) S[k] += (uint32_t)__shfl_xor((int)S[k], (int)s);
        if (WEIGHTED) {
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) W[k] += (uint32_t)__shfl_xor((int)W[k], (int)s);
        }
    }
    if (valid && (item & ((1u << lg) - 1u)) == 0u) {
        const uint32_t px = thumb_pixel(S, W, sh.cnt, WEIGHTED);
        uint8_t* q = dst + (u64)tile_dest(e, sh.o) * och;
        if (och == 4u) *reinterpret_cast<uint32_t*>(q) = px;      // (the slot is 256-aligned)
        else { q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); }
    }
}

__global__ __launch_bounds__(kTileThreads) void tile_gather(const uint8_t* __restrict__ pixels, const TileEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                             uint8_t* __restrict__ stage) {
    walk_tiles(tab, m, tiles, [&](const TileEntry& e, uint32_t tile) {
        const TileMem mem;
        const uint32_t sch = (e.cfg >> 16) & 15u, och = (e.cfg >> 20) & 15u;
        const u64 base = (u64)reinterpret_cast<uintptr_t>(pixels) + e.src_off;
        if (e.f == 1u) {
            const u64 k = (u64)tile * kTileThreads + threadIdx.x;
            if (k < tile_items(e.cw, e.ch, 1u, och)) {
                const u64 q = (u64)reinterpret_cast<uintptr_t>(stage) + e.dst_off;
                if (sch == 4u) { if (och == 4u) tile_copy_item<4u, 4u>(mem, e, base, q, (uint32_t)k); else tile_copy_item<4u, 3u>(mem, e, base, q, (uint32_t)k); }
                else { if (och == 4u) tile_copy_item<3u, 4u>(mem, e, base, q, (uint32_t)k); else tile_copy_item<3u, 3u>(mem, e, base, q, (uint32_t)k); }
            }
        } else {
            const uint32_t item_base = tile * kTileThreads;
            uint8_t* dst = stage + e.dst_off;
            if (sch == 3u) tile_reduce<3u, false>(mem, e, base, dst, item_base);     // (with 3 source channels the mode is PLAIN)
            else if (e.cfg & (1u << 24)) tile_reduce<4u, true>(mem, e, base, dst, item_base);
            else tile_reduce<4u, false>(mem, e, base, dst, item_base);
        }
    });
}

void launch_tile_gather(const uint8_t* pixels, const TileEntry* tab, uint32_t m, uint32_t tiles, uint8_t* stage, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tile_gather, dim3(grid), dim3(kTileThreads), 0, st, pixels, tab, m, tiles, stage);
}

// ---- QOIMI_TILE_NEAREST / QOIMI_TILE_MODE (tile_select) ----

// TileMem with the stores of single pixels: a dword, or a byte, of the tile's slot.
struct TileSelectMem : TileMem {
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
    __device__ __forceinline__ void store1(u64 a, uint32_t v) const { *reinterpret_cast<uint8_t*>(a) = (uint8_t)v; }
};

__device__ __forceinline__ u64 tile_xor_max(u64 v, uint32_t step) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)step), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)step);
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}

// One tile of kTileThreads items of a NEAREST entry with f >= 2: a lane per output pixel.
template <uint32_t SCH>
__device__ __forceinline__ void tile_nearest(const TileSelectMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t tile) {
    const u64 o = (u64)tile * kTileThreads + threadIdx.x;
    if (o < (u64)e.tw * e.th) tile_put(mem, e, q, (uint32_t)o, tile_centre_pixel<SCH>(mem, e, base, (uint32_t)o));
}

// One tile of kTileThreads items of a MODE entry with f >= 2: tensor_mode's meeting loop and butterfly (qoi_mode.hip) over the block.
template <uint32_t SCH>
__device__ __forceinline__ void tile_vote(const TileSelectMem& mem, const TileEntry& e, u64 base, u64 q, uint32_t tile) {
    const uint32_t lg = e.cfg & 255u, L = 1u << lg;
    const u64 item = (u64)tile * kTileThreads + threadIdx.x, o = item >> lg;
    const uint32_t l = (uint32_t)item & (L - 1u);
    const bool valid = o < (u64)e.tw * e.th;                          // (a pixel's lanes are valid or not together)
    ModeHeld h;
    if (valid) tile_vote_hold<SCH>(mem, e, base, (uint32_t)o, l, lg, h);
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
    for (uint32_t step = 1u; step < L; step <<= 1) best = tile_xor_max(best, step);
    if (valid && l == 0u) tile_put(mem, e, q, (uint32_t)o, mode_pick(best));
}

//   tile_select   The table and the walk of tile_gather; a call in one of the two label modes runs this kernel in its place.  f == 1 is
//                 tile_gather's copy.  NEAREST: a lane per output pixel fetches the centre pixel of its block and stores it.  MODE: L = 2^lg
//                 neighbouring lanes (1..64, the entry's: qoi_tile_core.h: tile_select_cfg) share an output pixel and hold at most four
//                 pixels of its block each, fetched from the caller's memory as above; they count and pick as tensor_mode does.  lg is the
//                 entry's and the walk hands a tile to the whole workgroup, so every cross-lane operation is reached by all 256 lanes:
//                 lanes behind the tile's last pixel take part holding nothing.  No LDS, no barrier, no atomics; nothing of the caller's
//                 is written.
__global__ __launch_bounds__(kTileThreads) void tile_select(const uint8_t* __restrict__ pixels, const TileEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                             uint8_t* __restrict__ stage) {
    walk_tiles(tab, m, tiles, [&](const TileEntry& e, uint32_t tile) {
        const TileSelectMem mem;
        const uint32_t sch = (e.cfg >> 16) & 15u, och = (e.cfg >> 20) & 15u, kind = (e.cfg >> 25) & 7u;
        const u64 base = (u64)reinterpret_cast<uintptr_t>(pixels) + e.src_off;
        const u64 q = (u64)reinterpret_cast<uintptr_t>(stage) + e.dst_off;
        if (e.f == 1u) {
            const u64 k = (u64)tile * kTileThreads + threadIdx.x;
            if (k < tile_items(e.cw, e.ch, 1u, och)) {
                if (sch == 4u) { if (och == 4u) tile_copy_item<4u, 4u>(mem, e, base, q, (uint32_t)k); else tile_copy_item<4u, 3u>(mem, e, base, q, (uint32_t)k); }
                else { if (och == 4u) tile_copy_item<3u, 4u>(mem, e, base, q, (uint32_t)k); else tile_copy_item<3u, 3u>(mem, e, base, q, (uint32_t)k); }
            }
        } else if (kind == kTileKindNearest) {
            if (sch == 4u) tile_nearest<4u>(mem, e, base, q, tile); else tile_nearest<3u>(mem, e, base, q, tile);
        } else {
            if (sch == 4u) tile_vote<4u>(mem, e, base, q, tile); else tile_vote<3u>(mem, e, base, q, tile);
        }
    });
}

void launch_tile_select(const uint8_t* pixels, const TileEntry* tab, uint32_t m, uint32_t tiles, uint8_t* stage, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(tile_select, dim3(grid), dim3(kTileThreads), 0, st, pixels, tab, m, tiles, stage);
}

}  // namespace qoimi

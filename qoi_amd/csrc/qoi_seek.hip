// qoi_seek.hip — the row seek index: where the chunk walk of a stream stands at a pixel (seek_block_scan, seek_locate), the colour table and
// the previous pixel there (seekpx_last, seekpx_carry), and band streams written from an index (band_assemble).  gfx950, wave64.  The host side:
// qoi_host_seek.hip (qoi_kernels.h holds the tables and declares the launchers; qoi_seek_core.h the arithmetic; qoi_amd/seekindex.py the
// normative statement).
//
//   seek_block_scan  Behind the passes of qoimi_inspect_streams as they are (every block's entry phase, every piece's map, a partial count per
//                    16 KiB block).  A wavefront per stream: the pixels of a block are run_px plus the five non-run chunk counts; their
//                    exclusive 64-bit scan over the stream's blocks, 64 blocks a step.
//   seek_locate      A wavefront per seek point.  A binary search in the scan for the last block that begins at or below pixel P, then that
//                    block tile by tile as inspect_count walks it: every lane enters its 64-byte piece at its true phase and counts the
//                    pixels of its chunks (a chunk belongs to the piece its tag byte is in), the counts are scanned over the wavefront and
//                    carried from tile to tile, and the one lane whose piece holds P walks its piece again, up to the chunk.  No lane
//                    holds P: the walk ran out in front of P (the block is the stream's last), byte_off = size - 8, skip = 0.
//   seekpx_last      Over a pixel buffer - the caller's (qoimi_seek_index_from_pixels: 3 or 4 bytes per pixel, tightly packed at any byte
//                    address, one launch for all images of a call) or the staging arena (qoimi_build_seek_index: 4 bytes per pixel in
//                    256-byte-aligned slots, one launch per sub-batch): tiles of kSeekTilePx pixels of ONE interval (qoi_dev.h: walk_tiles);
//                    a lane takes four CONSECUTIVE pixels of its tile - 12 or 16 bytes as the three to five aligned dwords that hold them,
//                    turned with v_alignbyte (qoi_seekpx_core.h: seekpx_fetch; never a dword that holds no byte of the lane's pixels) -
//                    hashes them with alpha 255 where the image has none and leaves position + 1 with an LDS atomic maximum in the slot's
//                    word - a pixel that equals its right neighbour (the next of its own, or the first of the lane to the right) is left
//                    out, the neighbour's position is larger - then 64 lanes fold the tile's words into the interval's 64 words in global
//                    memory, atomic maxima as well.  Positions are below 400 000 000: 32 bits.
//   seekpx_carry     A wavefront per image, a lane per slot: walks the image's intervals and carries "the last position that wrote slot s"
//                    forward; at every point it reads the pixels at those positions - the table - and pixel P - 1 through the same fetch
//                    (one dword or two), joins what seek_locate found and writes the point's 272 bytes.
//   band_assemble    Work is cut over the OUTPUT in aligned 16-byte words, as crop_gather cuts it: consecutive lanes take consecutive words
//                    of one band stream, a word wholly inside the tail is its 16 source bytes - at any alignment: the aligned dwords that
//                    hold them, turned with v_alignbyte - and one 16-byte store; the words of the head and the pad run and the words at a
//                    band stream's ends are put together byte by byte and written with byte, halfword, dword or 16-byte stores of the band
//                    stream's own bytes.  Never a word that would have to be read first; not one byte beside a band stream is written.
#include "qoi_dev.h"
#include "qoi_seek_core.h"
#include "qoi_seekpx_core.h"

namespace qoimi {

__device__ __forceinline__ uint32_t seek_blocks_of(const InsStream& S) {
    const uint32_t body = S.off != ~0ull ? S.size - (uint32_t)(kHeaderBytes + kTrailerBytes) : 0u;
    return (body + kInsBlock - 1u) / kInsBlock;
}

__global__ __launch_bounds__(256) void seek_block_scan(const InsStream* __restrict__ tab, uint32_t n, const InsPartial* __restrict__ partial,
                                                        u64* __restrict__ blk_px) {
    const uint32_t lane = lane_id(), s = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= n) return;
    const InsStream S = tab[s];
    const uint32_t nblk = seek_blocks_of(S);
    u64 carry = 0;
    for (uint32_t base = 0; base < nblk; base += 64u) {
        const uint32_t b = base + lane;
        u64 mine = 0;
        if (b < nblk) {
            const InsPartial P = partial[S.first_blk + b];
            mine = (u64)P.run_px + P.ops[0] + P.ops[1] + P.ops[2] + P.ops[4] + P.ops[5];
        }
        u64 incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const u64 up = (u64)__shfl_up((unsigned long long)incl, d);
            if (lane >= d) incl += up;
        }
        if (b < nblk) blk_px[S.first_blk + b] = carry + incl - mine;
        carry += (u64)__shfl((unsigned long long)incl, 63);
    }
}

__global__ __launch_bounds__(256) void seek_locate(const uint8_t* __restrict__ streams, const InsStream* __restrict__ tab, const InsBlock* __restrict__ blocks,
                                                    const u64* __restrict__ blk_px, const uint8_t* __restrict__ entry, const uint16_t* __restrict__ piece_map,
                                                    const SeekJob* __restrict__ jobs, uint32_t n_jobs, SeekLoc* __restrict__ loc) {
    const uint32_t lane = lane_id(), j = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (j >= n_jobs) return;
    const SeekJob J = jobs[j];
    const InsStream S = tab[J.stream];
    const uint32_t nblk = seek_blocks_of(S);
    bool found = false;
    if (nblk != 0u) {
        uint32_t lo = 0;                                                 // the last block that begins at or below P (the first begins at 0)
        for (uint32_t hi = nblk - 1u; lo < hi;) {
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            if (blk_px[S.first_blk + mid] <= (u64)J.P) lo = mid; else hi = mid - 1u;
        }
        const uint32_t blk = S.first_blk + lo;
        const InsBlock B = blocks[blk];
        const uint32_t len = B.len & ~kInsFirst;
        const uint32_t e = (B.len & kInsFirst) ? 0u : (uint32_t)entry[blk];
        const uint32_t rel = (uint32_t)((u64)J.P - blk_px[blk]);           // pixels of the block in front of P (P < 400 000 000)
        uint32_t carry = 0;
        for (uint32_t t = 0; t * kInsTile < len && !found; ++t) {
            const uint32_t at = t * kInsTile + lane * kInsPiece;
            const uint32_t plen = at < len ? (len - at < kInsPiece ? len - at : kInsPiece) : 0u;
            uint32_t d[16];
            ins_load_piece(streams + B.off + at, plen, d);
            const uint32_t p = plen ? ((uint32_t)piece_map[(size_t)B.piece_base + t * 64u + lane] >> (3u * e)) & 7u : 0u;
            uint32_t pos, before;
            const uint32_t cnt = seek_piece_walk(d, plen, p, 0xFFFFFFFFu, pos, before);
            uint32_t incl = cnt;
#pragma unroll
            for (uint32_t s = 1; s < 64u; s <<= 1) {
                const uint32_t up = __shfl_up(incl, s);
                if (lane >= s) incl += up;
            }
            const uint32_t excl = carry + incl - cnt;
            const bool mine = cnt != 0u && excl <= rel && rel - excl < cnt;
            if (mine) {
                (void)seek_piece_walk(d, plen, p, rel - excl, pos, before);
                SeekLoc L;
                L.byte_off = (uint32_t)kHeaderBytes + lo * kInsBlock + at + pos; L.skip = rel - excl - before;
                loc[J.point] = L;
            }
            found = lanes_where(mine) != 0ull;
            carry += read_lane(incl, 63);
        }
    }
    if (!found && lane == 0u) {
        SeekLoc L;
        L.byte_off = S.size - (uint32_t)kTrailerBytes; L.skip = 0u;
        loc[J.point] = L;
    }
}

struct PxMem {       // an aligned dword of the pixel buffer
    __device__ __forceinline__ uint32_t load(u64 a) const { return *reinterpret_cast<const uint32_t*>(a); }
};

__global__ __launch_bounds__(kSeekPxThreads) void seekpx_last(const uint8_t* __restrict__ pixels, const SeekPxImage* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                    uint32_t* __restrict__ last) {
    __shared__ uint32_t s_last[64];
    const uint32_t tid = threadIdx.x;
    const PxMem mem;
    walk_tiles(tab, m, tiles, [&](const SeekPxImage& e, uint32_t tile) {
        const uint32_t iv = tile / e.tpi, sub = tile - iv * e.tpi;
        const uint32_t p0 = iv * e.ipx;                                  // (an image holds fewer than 400 000 000 pixels)
        uint32_t i, n;
        seekpx_lane_span(sub, tid, e.ipx, i, n);
        if (tid < 64u) s_last[tid] = 0u;
        __syncthreads();
        uint32_t px[kSeekPxLane];
        seekpx_fetch(mem, (u64)reinterpret_cast<uintptr_t>(pixels) + e.src_off + (u64)(p0 + i) * e.ch, n, e.ch, px);
        const uint32_t next = __shfl_down(px[0], 1u);
        seekpx_lane_marks(px, n, next, seekpx_next_ok(tid, i, e.ipx), p0 + i, [&](uint32_t slot, uint32_t pos1) { atomicMax(&s_last[slot], pos1); });
        __syncthreads();
        if (tid < 64u && s_last[tid] != 0u) atomicMax(&last[(size_t)(e.point_base + iv) * 64u + tid], s_last[tid]);
        __syncthreads();                                                 // s_last is zeroed again by the next tile
    });
}

__global__ __launch_bounds__(256) void seekpx_carry(const uint8_t* __restrict__ pixels, const SeekPxImage* __restrict__ tab, uint32_t m,
                                                     const uint32_t* __restrict__ last, const SeekLoc* __restrict__ loc, SeekPoint* __restrict__ points) {
    const uint32_t lane = lane_id(), i = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= m) return;
    const SeekPxImage E = tab[i];
    const PxMem mem;
    const u64 base = (u64)reinterpret_cast<uintptr_t>(pixels) + E.src_off;
    uint32_t cur = 0;                                                    // position + 1 of the last pixel so far whose slot is `lane`
    for (uint32_t j = 0; j < E.np; ++j) {
        const uint32_t v = last[(size_t)(E.point_base + j) * 64u + lane];
        cur = v != 0u ? v : cur;
        SeekPoint* o = points + E.point_base + j;
        o->table[lane] = cur != 0u ? seekpx_one(mem, base + (u64)(cur - 1u) * E.ch, E.ch) : 0u;
        if (lane == 0u) {
            const SeekLoc L = loc[E.point_base + j];
            o->byte_off = L.byte_off; o->skip = L.skip; o->prev = seekpx_one(mem, base + ((u64)(j + 1u) * E.ipx - 1u) * E.ch, E.ch); o->reserved = 0u;
        }
    }
}

typedef uint32_t seek_u32x4 __attribute__((ext_vector_type(4)));

struct BandMem {
    const uint8_t* heads; const uint8_t* tail;
    __device__ __forceinline__ uint32_t head(uint32_t i) const { return heads[i]; }
    __device__ __forceinline__ uint32_t tail1(uint32_t i) const { return tail[i]; }
    // the tail's bytes [i, i + 16): four aligned dwords, a fifth - the one that holds the last byte - where the source is not dword aligned
    __device__ __forceinline__ void tail16(uint32_t i, uint32_t (&W)[4]) const {
        const uint8_t* src = tail + i;
        const uint32_t s = (uint32_t)reinterpret_cast<uintptr_t>(src) & 3u;
        const uint32_t* a = reinterpret_cast<const uint32_t*>(src - s);
        const uint32_t w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3], w4 = s ? a[4] : 0u;
        W[0] = __builtin_amdgcn_alignbyte(w1, w0, s); W[1] = __builtin_amdgcn_alignbyte(w2, w1, s);
        W[2] = __builtin_amdgcn_alignbyte(w3, w2, s); W[3] = __builtin_amdgcn_alignbyte(w4, w3, s);
    }
    __device__ __forceinline__ void store1(u64 a, uint32_t v) const { *reinterpret_cast<uint8_t*>(a) = (uint8_t)v; }
    __device__ __forceinline__ void store2(u64 a, uint32_t v) const { *reinterpret_cast<uint16_t*>(a) = (uint16_t)v; }
    __device__ __forceinline__ void store4(u64 a, uint32_t v) const { *reinterpret_cast<uint32_t*>(a) = v; }
    __device__ __forceinline__ void store16(u64 a, const uint32_t (&W)[4]) const {
        seek_u32x4 v; v.x = W[0]; v.y = W[1]; v.z = W[2]; v.w = W[3];
        *reinterpret_cast<seek_u32x4*>(a) = v;
    }
};

__global__ __launch_bounds__(kSeekThreads) void band_assemble(const uint8_t* __restrict__ streams, const BandEntry* __restrict__ tab, uint32_t m, uint32_t tiles,
                                                               const uint8_t* __restrict__ heads, uint8_t* out) {
    walk_tiles(tab, m, tiles, [&](const BandEntry& e, uint32_t tile) {
        const SeekPrefix f = {0u, 0u, e.head_len, e.run_full, e.run_last};
        const BandMem mem = {heads + e.head_at, streams + e.src_off};
        const u64 q = (u64)reinterpret_cast<uintptr_t>(out) + e.dst_off;
        const u64 k = (u64)tile * kSeekThreads + threadIdx.x;
        if (k < crop_items(q, e.B)) seek_band_item(mem, f, q, e.B, (uint32_t)k);
    });
}

void launch_seek_locate(const uint8_t* streams, const InsStream* tab, uint32_t n_streams, const InsBlock* blocks, const InsPartial* partial,
                        const uint8_t* entry, const uint16_t* piece_map, u64* blk_px, const SeekJob* jobs, uint32_t n_jobs, SeekLoc* loc, hipStream_t st) {
    hipLaunchKernelGGL(seek_block_scan, dim3((n_streams + 3u) / 4u), dim3(256), 0, st, tab, n_streams, partial, blk_px);
    hipLaunchKernelGGL(seek_locate, dim3((n_jobs + 3u) / 4u), dim3(256), 0, st, streams, tab, blocks, (const u64*)blk_px, entry, piece_map, jobs, n_jobs, loc);
}

void launch_seek_tables_px(const uint8_t* pixels, const SeekPxImage* tab, uint32_t m, uint32_t tiles, uint32_t* last, const SeekLoc* loc, SeekPoint* points,
                           uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(seekpx_last, dim3(grid), dim3(kSeekPxThreads), 0, st, pixels, tab, m, tiles, last);
    hipLaunchKernelGGL(seekpx_carry, dim3((m + 3u) / 4u), dim3(256), 0, st, pixels, tab, m, (const uint32_t*)last, loc, points);
}

void launch_band_assemble(const uint8_t* streams, const BandEntry* tab, uint32_t m, uint32_t tiles, const uint8_t* heads, uint8_t* out, uint32_t grid,
                          hipStream_t st) {
    hipLaunchKernelGGL(band_assemble, dim3(grid), dim3(kSeekThreads), 0, st, streams, tab, m, tiles, heads, out);
}

}  // namespace qoimi

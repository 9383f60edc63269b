// qoi_inspect.hip — qoimi_inspect_streams: the chunk walk of a stream without pixel state (chunk counts, pixels, run pixels, repeated
// QOI_OP_INDEX, where the walk ends).  gfx950, wave64.  The host side: qoi_host_pack.hip (qoi_kernels.h holds the tables and declares the launcher).
//
// The walk is serial only in its PHASE: a piece of a stream that is entered e = 0..4 bytes behind its first byte (the chunk in front of
// it reaches e bytes in) leaves x = 0..4 bytes over into the next piece.  A piece is therefore a map {0..4} -> {0..4}: five 3-bit
// values, 15 bits, and the map of two pieces in a row is the composition of their maps - associative, so maps are scanned like sums.
// Nothing here assumes that the five phases ever meet (a body of 0xFF bytes keeps five different walks for ever): the whole map is
// carried everywhere.
//
//   inspect_maps    a wavefront per BLOCK (16 KiB of ONE stream's body, four tiles of 64 pieces of 64 bytes): every lane's piece map by one
//                   backward sweep over its 64 bytes (exit(pos) = exit(pos + chunk length at pos): all five phases in one chain), the maps
//                   scanned over the wavefront and from tile to tile; writes every piece's map of "block entry -> piece entry" (2 bytes per
//                   64 stream bytes) and the block's map.  The first block of a stream is entered at phase 0, so its map is written as the
//                   CONSTANT map of its exit: a constant map forgets what was in front of it, which makes the scan over all blocks of all
//                   streams one plain scan - no segment flags.
//   inspect_scan    one workgroup: exclusive scan of the block maps, applied to phase 0 -> every block's entry phase.
//   inspect_count   a wavefront per block again: every lane enters its piece at its true phase and walks it once, counting; counts are
//                   summed over the wavefront and written as one partial record per block (no atomics).
//   inspect_reduce  a wavefront per stream: sums its blocks' partials, adds the repeated-INDEX pairs that straddle a block edge, reads
//                   the 14 header and 8 trailer bytes and writes the result record (the host turns it into flags).
//
// The stream bytes are read twice (inspect_maps, inspect_count), always as the aligned dwords that hold bytes of the body [14, size - 8):
// a chunk that starts below size - 8 is counted by its tag byte alone, so nothing behind the body is needed for the walk.
#include "qoi_dev.h"

namespace qoimi {

// (kInsPiece, kInsTile, kInsTiles, kInsBlock, kInsFirst and the table structs: qoi_kernels.h)
constexpr uint32_t kInsIdentity = 0u | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12);
constexpr uint32_t kInsNoTag = 0x100u;          // "no chunk starts here" where a tag byte is expected

// bytes of the chunk whose tag byte is b (qoi.h:547-575)
__device__ __forceinline__ uint32_t ins_len(uint32_t b) { return b >= kTagRgb ? b - 0xFAu : ((b >> 6) == 2u ? 2u : 1u); }

// then[first[e]] for every e
__device__ __forceinline__ uint32_t ins_compose(uint32_t first, uint32_t then) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t e = 0; e < 5u; ++e) r |= ((then >> (3u * ((first >> (3u * e)) & 7u))) & 7u) << (3u * e);
    return r;
}

// (ins_load_piece - a lane's piece as 16 dwords: qoi_dev.h)
__device__ __forceinline__ uint32_t ins_byte(const uint32_t (&d)[16], uint32_t pos) { return (d[pos >> 2] >> (8u * (pos & 3u))) & 0xFFu; }

// The map of a piece of plen bytes.  exit(pos), the bytes left over by the walk that has a chunk start at pos, is pos - plen at and behind
// the piece's end and exit(pos + length of the chunk at pos) inside it: one backward sweep with the five exits behind pos in a window.
__device__ __forceinline__ uint32_t ins_piece_map(const uint32_t (&d)[16], uint32_t plen) {
    uint32_t win = 0;
#pragma unroll
    for (uint32_t j = 0; j < 5u; ++j) win |= ((kInsPiece + j - plen) & 7u) << (3u * j);
#pragma unroll
    for (int pos = (int)kInsPiece - 1; pos >= 0; --pos) {
        const uint32_t b = ins_byte(d, (uint32_t)pos);
        uint32_t x = (win >> (3u * (ins_len(b) - 1u))) & 7u;
        x = (uint32_t)pos < plen ? x : ((uint32_t)pos - plen) & 7u;
        win = (win << 3) | x;
    }
    return win & 0x7FFFu;
}

__device__ __forceinline__ uint32_t ins_wave_scan(uint32_t mine, uint32_t lane) {      // inclusive, lower lanes first
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl = ins_compose(up, incl);
    }
    return incl;
}

__global__ __launch_bounds__(256) void inspect_maps(const uint8_t* __restrict__ streams, const InsBlock* __restrict__ blocks, uint32_t n_blocks,
                                                     uint32_t* __restrict__ block_map, uint16_t* __restrict__ piece_map) {
    const uint32_t lane = lane_id(), blk = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blk >= n_blocks) return;
    const InsBlock B = blocks[blk];
    const uint32_t len = B.len & ~kInsFirst;
    uint32_t carry = kInsIdentity;                                   // block entry -> entry of the tile
    for (uint32_t t = 0; t * kInsTile < len; ++t) {
        const uint32_t at = t * kInsTile + lane * kInsPiece;
        const uint32_t plen = at < len ? (len - at < kInsPiece ? len - at : kInsPiece) : 0u;
        uint32_t d[16];
        ins_load_piece(streams + B.off + at, plen, d);
        const uint32_t incl = ins_wave_scan(ins_piece_map(d, plen), lane);
        uint32_t excl = __shfl_up(incl, 1u);
        if (lane == 0u) excl = kInsIdentity;
        if (plen != 0u) piece_map[(size_t)B.piece_base + t * 64u + lane] = (uint16_t)ins_compose(carry, excl);
        carry = ins_compose(carry, read_lane(incl, 63));
    }
    if (lane == 0u) block_map[blk] = (B.len & kInsFirst) ? (carry & 7u) * 0x1249u : carry;
}

// Exclusive scan of the block maps in one workgroup (the shape of pack_offsets): tiles of 8192 maps, eight consecutive ones per thread.
__global__ __launch_bounds__(1024) void inspect_scan(const uint32_t* __restrict__ block_map, uint32_t n, uint8_t* __restrict__ entry) {
    constexpr uint32_t kPer = 8, kTile = 1024u * kPer;
    __shared__ uint32_t s_wave[16];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t carry = kInsIdentity;
    for (uint32_t base = 0; base < n; base += kTile) {
        const uint32_t e0 = base + tid * kPer;
        uint32_t m[kPer], mine = kInsIdentity;
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            m[k] = e0 + k < n ? block_map[e0 + k] : kInsIdentity;
            mine = ins_compose(mine, m[k]);
        }
        const uint32_t incl = ins_wave_scan(mine, lane);
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = kInsIdentity, total = kInsIdentity;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t s = s_wave[k];
            if (k < wave) before = ins_compose(before, s);
            total = ins_compose(total, s);
        }
        __syncthreads();                                       // s_wave is rewritten by the next tile
        uint32_t excl = __shfl_up(incl, 1u);
        if (lane == 0u) excl = kInsIdentity;
        uint32_t run = ins_compose(ins_compose(carry, before), excl);
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            if (e0 + k < n) entry[e0 + k] = (uint8_t)(run & 7u);         // the blocks in front, entered at phase 0 (a stream's first block forgets them)
            run = ins_compose(run, m[k]);
        }
        carry = ins_compose(carry, total);
    }
}

__global__ __launch_bounds__(256) void inspect_count(const uint8_t* __restrict__ streams, const InsBlock* __restrict__ blocks, uint32_t n_blocks,
                                                      const uint32_t* __restrict__ block_map, const uint8_t* __restrict__ entry,
                                                      const uint16_t* __restrict__ piece_map, InsPartial* __restrict__ partial) {
    const uint32_t lane = lane_id(), blk = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blk >= n_blocks) return;
    const InsBlock B = blocks[blk];
    const uint32_t len = B.len & ~kInsFirst;
    const uint32_t e = (B.len & kInsFirst) ? 0u : (uint32_t)entry[blk];
    // chunk counts, two 16-bit counters to a word (a lane counts at most 256 chunks, a wavefront 16384): INDEX|DIFF, LUMA|RUN, RGB|RGBA
    uint32_t c01 = 0, c23 = 0, c45 = 0, rep = 0, run_px = 0;
    uint32_t blk_first = kInsNoTag, blk_last = kInsNoTag;
    for (uint32_t t = 0; t * kInsTile < len; ++t) {
        const uint32_t at = t * kInsTile + lane * kInsPiece;
        const uint32_t plen = at < len ? (len - at < kInsPiece ? len - at : kInsPiece) : 0u;
        uint32_t d[16];
        ins_load_piece(streams + B.off + at, plen, d);
        uint32_t p = plen ? ((uint32_t)piece_map[(size_t)B.piece_base + t * 64u + lane] >> (3u * e)) & 7u : 0u;
        uint32_t first = kInsNoTag, last = kInsNoTag;                // tag bytes of the piece's first and last chunk
#pragma unroll
        for (uint32_t pos = 0; pos < kInsPiece; ++pos) {
            const uint32_t b = ins_byte(d, pos);
            if (p == pos && pos < plen) {
                const uint32_t k = b >> 6;
                if (b >= kTagRgb) c45 += 1u << ((b & 1u) * 16u);
                else if (k < 2u) c01 += 1u << (k * 16u);
                else c23 += 1u << ((k & 1u) * 16u);
                if (b < kTagRgb && k == 3u) run_px += (b & 63u) + 1u;
                rep += (b < 64u && b == last) ? 1u : 0u;             // INDEX behind INDEX with the same byte (qoi.h:118-119)
                first = first == kInsNoTag ? b : first;
                last = b;
                p = pos + ins_len(b);
            }
        }
        // the pair across the piece's front edge: every piece in front of one that holds a chunk is a full one and holds a chunk itself
        const uint32_t below = from_lane_below(last, blk_last);
        rep += (first < 64u && first == below) ? 1u : 0u;
        if (t == 0u) blk_first = read_lane(first, 0);
        const u64 have = lanes_where(last != kInsNoTag);
        if (have != 0ull) blk_last = read_lane_dyn(last, 63u - (uint32_t)__builtin_clzll(have));
    }
    c01 = wave_sum(c01); c23 = wave_sum(c23); c45 = wave_sum(c45); rep = wave_sum(rep); run_px = wave_sum(run_px);
    if (lane == 0u) {
        InsPartial P;
        P.ops[0] = c01 & 0xFFFFu; P.ops[1] = c01 >> 16; P.ops[2] = c23 & 0xFFFFu; P.ops[3] = c23 >> 16; P.ops[4] = c45 & 0xFFFFu; P.ops[5] = c45 >> 16;
        P.run_px = run_px; P.repeat = rep; P.first = blk_first; P.last = blk_last;
        P.exit = (block_map[blk] >> (3u * e)) & 7u; P.pad = 0u;
        partial[blk] = P;
    }
}

// result and raw are pinned host memory (the context's staging), written in place: 64 + 32 bytes per stream.
__global__ __launch_bounds__(256) void inspect_reduce(const uint8_t* __restrict__ streams, const InsStream* __restrict__ tab, uint32_t n,
                                                       const InsPartial* __restrict__ partial, InsResult* __restrict__ result, uint32_t* __restrict__ raw) {
    const uint32_t lane = lane_id(), s = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= n) return;
    const InsStream S = tab[s];
    const bool read = S.off != ~0ull;
    const uint32_t body = read ? S.size - (uint32_t)(kHeaderBytes + kTrailerBytes) : 0u;
    const uint32_t nblk = (body + kInsBlock - 1u) / kInsBlock;
    uint32_t ops[6] = {0u, 0u, 0u, 0u, 0u, 0u}, rep = 0, run_lo = 0;          // (a lane sums at most 2^31 / 16384 / 64 blocks of at most 2^20 run pixels)
    for (uint32_t b = lane; b < nblk; b += 64u) {
        const InsPartial P = partial[S.first_blk + b];
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) ops[k] += P.ops[k];
        rep += P.repeat; run_lo += P.run_px;
        if (b != 0u && P.first < 64u && P.first == partial[S.first_blk + b - 1u].last) rep += 1u;
    }
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) ops[k] = wave_sum(ops[k]);
    rep = wave_sum(rep);
    u64 run_px = run_lo;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) run_px += (u64)__shfl_xor((unsigned long long)run_px, o);
    // header and trailer: lanes 0..5 put together a word each
    if (lane < 8u) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t j = lane * 4u + k;
            if (read && j < 22u) w |= (uint32_t)streams[S.off + (j < 14u ? j : S.size - 22u + j)] << (8u * k);
        }
        raw[(size_t)s * 8u + lane] = w;
    }
    if (lane == 0u) {
        InsResult R;
        R.run_pixels = run_px;
        R.pixels = (u64)ops[0] + ops[1] + ops[2] + ops[4] + ops[5] + run_px;
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) R.ops[k] = ops[k];
        R.repeat_index = rep;
        R.walk_end = read ? (uint32_t)kHeaderBytes + body + (nblk ? partial[S.first_blk + nblk - 1u].exit : 0u) : 0u;
        R.flags = 0u; R.reserved[0] = R.reserved[1] = R.reserved[2] = 0u;
        result[s] = R;
    }
}

void launch_inspect(const uint8_t* streams, const InsStream* tab, uint32_t n_streams, const InsBlock* blocks, uint32_t n_blocks,
                    uint32_t* block_map, uint8_t* entry, uint16_t* piece_map, InsPartial* partial, InsResult* result, uint32_t* raw,
                    hipStream_t st, KernelTimer* tm) {
    tm->mark(kT_begin, st);
    if (n_blocks != 0u) {
        const uint32_t grid = (n_blocks + 3u) / 4u;
        hipLaunchKernelGGL(inspect_maps, dim3(grid), dim3(256), 0, st, streams, blocks, n_blocks, block_map, piece_map);
        tm->mark(kT_inspect_maps, st);
        hipLaunchKernelGGL(inspect_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)block_map, n_blocks, entry);
        tm->mark(kT_inspect_scan, st);
        hipLaunchKernelGGL(inspect_count, dim3(grid), dim3(256), 0, st, streams, blocks, n_blocks, (const uint32_t*)block_map, (const uint8_t*)entry,
                           (const uint16_t*)piece_map, partial);
        tm->mark(kT_inspect_count, st);
    }
    hipLaunchKernelGGL(inspect_reduce, dim3((n_streams + 3u) / 4u), dim3(256), 0, st, streams, tab, n_streams, (const InsPartial*)partial, result, raw);
    tm->mark(kT_inspect_reduce, st);
}

}  // namespace qoimi

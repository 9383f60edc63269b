// qoi_pack.hip — streams back to back: the offsets of a pack (pack_offsets), the copy into it (pack_copy), their append forms
// (pack_offsets_append, pack_copy_append: qoimi_encode_packed adds a sub-batch of streams to a pack that earlier launches began) and
// the header gather of qoimi_read_descs (gather_headers).  gfx950, wave64.  The host side: qoi_host_pack.hip (qoi_kernels.h declares the launchers).
#include "qoi_dev.h"

namespace qoimi {

// A stream's length as the pack takes it: a caller's error (negative, longer than the stride) never makes a kernel read outside
// [streams, streams + n * stride).
__device__ __forceinline__ u64 pack_len(int len, u64 stride) { return len <= 0 ? 0ull : ((u64)len < stride ? (u64)len : stride); }

// ---------------------------------------------------------------------------------
// Exclusive scan of the lengths, every start rounded up to `align` (a power of two): every start is a multiple of align, so the
// starts are the exclusive scan of the ROUNDED lengths; off[n] is the end of the last stream, not rounded.  One workgroup, one launch,
// tiles of 8192 lengths (eight consecutive ones per thread: lane-serial, six rounds over the wavefront, then over the 16 wavefronts)
// - the shape of enc_offsets with 64-bit sums.
// ---------------------------------------------------------------------------------
// The append form scans a sub-batch, lens[first .. first + n), into off[first .. first + n]: it is seeded ON THE DEVICE with what the
// launch in front of it left in off[first] - the unrounded end of the pack so far - rounded up (first == 0: with 0), so no length or
// offset travels through the host between two sub-batches.
template <bool kAppend>
__device__ __forceinline__ void pack_offsets_body(const int* __restrict__ lens, uint32_t n, u64 stride, u64 align_mask, u64* off) {
    constexpr uint32_t kPer = 8, kTile = 1024u * kPer;
    __shared__ u64 s_wave[16];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    u64 carry = kAppend ? (off[0] + align_mask) & ~align_mask : 0ull;     // (read by every thread in front of the first barrier, written behind it)
    for (uint32_t base = 0; base < n; base += kTile) {
        const uint32_t e0 = base + tid * kPer;
        u64 raw[kPer], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            raw[k] = e0 + k < n ? pack_len(lens[e0 + k], stride) : 0ull;
            mine += (raw[k] + align_mask) & ~align_mask;
        }
        u64 incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const u64 up = (u64)__shfl_up((unsigned long long)incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) { const u64 s = s_wave[k]; before += k < wave ? s : 0ull; total += s; }
        __syncthreads();                                       // s_wave is rewritten by the next tile
        u64 run = carry + before + incl - mine;
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            if (e0 + k < n) off[e0 + k] = run;
            if (e0 + k + 1u == n) off[n] = run + raw[k];
            run += (raw[k] + align_mask) & ~align_mask;
        }
        carry += total;
    }
}
__global__ __launch_bounds__(1024) void pack_offsets(const int* __restrict__ lens, uint32_t n, u64 stride, u64 align_mask, u64* __restrict__ off) {
    pack_offsets_body<false>(lens, n, stride, align_mask, off);
}
__global__ __launch_bounds__(1024) void pack_offsets_append(const int* __restrict__ lens, uint32_t first, uint32_t n, u64 stride, u64 align_mask, u64* off) {
    if (first == 0u) pack_offsets_body<false>(lens, n, stride, align_mask, off);
    else pack_offsets_body<true>(lens + first, n, stride, align_mask, off + first);
}

// ---------------------------------------------------------------------------------
// The copy.  Work is cut by DESTINATION bytes: tiles of kPackTile bytes of the pack (16-byte granules of the destination ADDRESS), a
// workgroup takes a contiguous range of tiles, so it looks its first stream up once (binary search in off) and steps on from tile to
// tile; a tile inside one stream - the usual case for streams of megabytes - costs no search at all, a tile that holds hundreds of
// streams one short search per lane between the tile's first and last stream.  A lane writes whole granules: a granule that lies in
// one stream is one 16-byte store, its 16 source bytes - at any alignment - the aligned dwords that hold them, turned with v_alignbyte
// (four dwords, a fifth only where the source is not dword aligned: the dword that holds the granule's last byte, never the one behind
// it); a granule at a stream's head or tail, in a gap or across several short streams goes byte by byte.  Gap bytes are not written,
// a stream that does not end at or below `cap` is not written at all.
// Loads are non-temporal (a stream is read once), stores plain (what comes next reads the pack).
// ---------------------------------------------------------------------------------
constexpr uint32_t kPackThreads = 256, kPackPer = kPackTile / 16u / kPackThreads;       // (kPackTile: qoi_kernels.h)
// The append form (qoimi_encode_packed) copies the streams [first, e) of a sub-batch behind what earlier launches put into the pack: its range
// of the destination is [off[first], min(off[e], cap)), searches stay inside [first, e], stream j is read at streams + (j - first) * stride
// or, for a call of mixed shapes, at streams + src_off[j].  The granule that holds off[first] may hold the tail of the previous sub-batch's
// last stream: the 16-byte store is taken only by granules that lie wholly inside ONE stream of this sub-batch, the byte path never touches
// a byte below off[first].  kAppend == false is the copy of qoimi_pack_streams as it always was (first 0, e n, source j * stride).
template <bool kAppend>
__device__ __forceinline__ void pack_copy_body(const uint8_t* __restrict__ streams, u64 stride, const u64* __restrict__ src_off, const int* __restrict__ lens,
                                               uint32_t first_arg, uint32_t e, const u64* __restrict__ off, uint8_t* __restrict__ packed, u64 cap) {
    const uint32_t first = kAppend ? first_arg : 0u;
    const u64 dm = (u64)(reinterpret_cast<uintptr_t>(packed) & 15u);         // positions below are packed offsets + dm: granules of the destination address
    const u64 begin = kAppend ? off[first] : 0ull;
    const u64 end_all = off[e] < cap ? off[e] : cap;
    if (end_all <= begin) return;
    const u64 t_first = kAppend ? (begin + dm) / kPackTile : 0ull;
    const u64 tiles = (end_all + dm + kPackTile - 1u) / kPackTile - t_first;
    const u64 per_wg = (tiles + gridDim.x - 1u) / gridDim.x;
    const u64 t_lo = t_first + (u64)blockIdx.x * per_wg, t_hi = t_lo + per_wg < t_first + tiles ? t_lo + per_wg : t_first + tiles;
    if (t_lo >= t_hi) return;
    auto source = [&](uint32_t s) -> u64 { return !kAppend ? (u64)s * stride : (src_off ? src_off[s] : (u64)(s - first) * stride); };
    // largest s in [lo, hi] with off[s] + dm <= x (off[lo] + dm <= x is the caller's)
    auto find = [&](uint32_t lo, uint32_t hi, u64 x) {
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            if (off[mid] + dm <= x) lo = mid; else hi = mid - 1u;
        }
        return lo;
    };
    uint32_t s0 = find(first, e - 1u, t_lo * kPackTile < begin + dm ? begin + dm : t_lo * kPackTile);
    for (u64 t = t_lo; t < t_hi; ++t) {
        const u64 tb = t * kPackTile, te = tb + kPackTile;
        const uint32_t s1 = (s0 + 1u >= e || off[s0 + 1u] + dm >= te) ? s0 : find(s0 + 1u, e - 1u, te - 1u);
        const bool one = s0 == s1;
        const u64 start0 = off[s0], len0 = pack_len(lens[s0], stride);
        uint32_t w[kPackPer][5]; uint32_t sh[kPackPer]; bool whole[kPackPer];
        // what a granule's lane knows of it: its first stream, that stream's start and length
        uint32_t gs[kPackPer]; u64 gstart[kPackPer], glen[kPackPer];
#pragma unroll
        for (uint32_t k = 0; k < kPackPer; ++k) {
            const u64 v = tb + (u64)(k * kPackThreads + threadIdx.x) * 16u;          // the granule's first byte
            whole[k] = false; sh[k] = 0u; gs[k] = s0; gstart[k] = start0; glen[k] = len0;
            if (!one && v >= begin + dm) { gs[k] = find(s0, s1, v); gstart[k] = off[gs[k]]; glen[k] = pack_len(lens[gs[k]], stride); }
            if (v < begin + dm || v - dm >= end_all) continue;                       // (a granule that begins below the range: byte by byte, below)
            const u64 rel = v - dm - gstart[k];
            whole[k] = rel + 16u <= glen[k] && gstart[k] + glen[k] <= cap;
            if (whole[k]) {
                const uint8_t* src = streams + source(gs[k]) + rel;
                const uint32_t m = (uint32_t)reinterpret_cast<uintptr_t>(src) & 3u;
                const uint32_t* a = reinterpret_cast<const uint32_t*>(src - m);
                w[k][0] = __builtin_nontemporal_load(&a[0]); w[k][1] = __builtin_nontemporal_load(&a[1]);
                w[k][2] = __builtin_nontemporal_load(&a[2]); w[k][3] = __builtin_nontemporal_load(&a[3]);
                w[k][4] = m ? __builtin_nontemporal_load(&a[4]) : 0u;
                sh[k] = m;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kPackPer; ++k) {
            const u64 v = tb + (u64)(k * kPackThreads + threadIdx.x) * 16u;
            if (whole[k]) {
                uint4 o;
                o.x = __builtin_amdgcn_alignbyte(w[k][1], w[k][0], sh[k]); o.y = __builtin_amdgcn_alignbyte(w[k][2], w[k][1], sh[k]);
                o.z = __builtin_amdgcn_alignbyte(w[k][3], w[k][2], sh[k]); o.w = __builtin_amdgcn_alignbyte(w[k][4], w[k][3], sh[k]);
                *reinterpret_cast<uint4*>(packed + (v - dm)) = o;
                continue;
            }
            if (v + 16u <= begin + dm || (v >= dm && v - dm >= end_all)) continue;
            // head / tail / gap / several short streams in one granule: byte by byte, stepping on from stream to stream
            uint32_t s = gs[k]; u64 st = gstart[k], ln = glen[k];
            for (uint32_t b = 0; b < 16u; ++b) {
                if (v + b < begin + dm) continue;
                const u64 x = v + b - dm;
                if (x >= end_all) break;
                while (s < s1 && x >= off[s + 1u]) { ++s; st = off[s]; ln = pack_len(lens[s], stride); }
                if (x - st < ln && st + ln <= cap) packed[x] = __builtin_nontemporal_load(&streams[source(s) + (x - st)]);
            }
        }
        s0 = s1;
    }
}
__global__ __launch_bounds__(kPackThreads) void pack_copy(const uint8_t* __restrict__ streams, u64 stride, const int* __restrict__ lens, uint32_t n,
                                                           const u64* __restrict__ off, uint8_t* __restrict__ packed, u64 cap) {
    pack_copy_body<false>(streams, stride, nullptr, lens, 0u, n, off, packed, cap);
}
__global__ __launch_bounds__(kPackThreads) void pack_copy_append(const uint8_t* __restrict__ streams, u64 stride, const u64* __restrict__ src_off,
                                                                  const int* __restrict__ lens, uint32_t first, uint32_t m,
                                                                  const u64* __restrict__ off, uint8_t* __restrict__ packed, u64 cap) {
    pack_copy_body<true>(streams, stride, src_off, lens, first, first + m, off, packed, cap);
}

// ---------------------------------------------------------------------------------
// qoimi_read_descs: the 14 header bytes of every stream (any alignment) into a 16-byte slot each.  offs and out are pinned host memory
// (the context's staging); offs[i] == ~0: a stream too short to hold a header, nothing is read.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_headers(const uint8_t* __restrict__ streams, const u64* __restrict__ offs, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 o = offs[i];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (o != ~0ull)
        for (uint32_t b = 0; b < (uint32_t)kHeaderBytes; ++b) w[b >> 2] |= (uint32_t)streams[o + b] << (8u * (b & 3u));
    *reinterpret_cast<uint4*>(out + 4u * (size_t)i) = make_uint4(w[0], w[1], w[2], w[3]);
}

void launch_pack_streams(const uint8_t* streams, size_t stride, const int* lens, uint32_t n, unsigned align, uint8_t* packed, size_t cap, u64* off,
                         uint32_t grid, hipStream_t st, KernelTimer* tm) {
    tm->mark(kT_begin, st);
    hipLaunchKernelGGL(pack_offsets, dim3(1), dim3(1024), 0, st, lens, n, (u64)stride, (u64)align - 1u, off);
    tm->mark(kT_pack_offsets, st);
    if (cap != 0) {
        hipLaunchKernelGGL(pack_copy, dim3(grid), dim3(kPackThreads), 0, st, streams, (u64)stride, lens, n, (const u64*)off, packed, (u64)cap);
        tm->mark(kT_pack_copy, st);
    }
}

// One sub-batch of qoimi_encode_packed: streams [first, first + m) of the call, strided in the staging arena, behind what is in the pack.
// grid: the host's upper bound of the sub-batch's tiles (workgroups without a tile return at once).
void launch_pack_append(const uint8_t* staging, size_t stride, const u64* src_off, const int* lens, uint32_t first, uint32_t m, unsigned align,
                        uint8_t* packed, size_t cap, u64* off, uint32_t grid, hipStream_t st, KernelTimer* tm) {
    tm->mark(kT_begin, st);
    hipLaunchKernelGGL(pack_offsets_append, dim3(1), dim3(1024), 0, st, lens, first, m, (u64)stride, (u64)align - 1u, off);
    tm->mark(kT_pack_offsets_append, st);
    if (cap != 0) {
        hipLaunchKernelGGL(pack_copy_append, dim3(grid), dim3(kPackThreads), 0, st, staging, (u64)stride, src_off, lens, first, m, (const u64*)off, packed, (u64)cap);
        tm->mark(kT_pack_copy_append, st);
    }
}

void launch_gather_headers(const uint8_t* streams, const u64* offs, uint32_t n, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(gather_headers, dim3((n + 255u) / 256u), dim3(256), 0, st, streams, offs, n, out);
}

}  // namespace qoimi

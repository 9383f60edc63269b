// qoi_ctx.h — what the host files of the C-ABI shim (qoi_host*.hip) share: the error path, the context and its arenas, the header
// rules, and the few lines every entry point begins with.  Host only; no kernel file includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

// The library is built with -fvisibility=hidden: what the header declares is the whole exported surface (tests/test_abi.py
// reads it back with nm -D).
#pragma GCC visibility push(default)
#include "../../include/qoi_mi355x.h"
#pragma GCC visibility pop
#include "qoi_kernels.h"
#include "qoi_stage_plan.h"   // the plans of the calls that work through bounded staging: host arithmetic alone, tested without a GPU

using namespace qoimi;

// ------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------
namespace qoimi { int fail(int code, const std::string& msg); }   // leaves msg as the calling thread's qoimi_last_error (qoi_host.hip) and returns code
#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? QOIMI_E_NOMEM                             \
                        : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice || e_ == hipErrorInsufficientDriver) ? QOIMI_E_NO_GPU \
                        : QOIMI_E_INTERNAL,                                                    \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)

// Every entry point works on its context's device and leaves the calling thread's current device as it found it
// (a caller may hold several GPUs, e.g. under torch).
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
        else if (prev < 0) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// ------------------------------------------------------------------------------------
// context: device + growable workspace arenas
// ------------------------------------------------------------------------------------
struct Arena {
    void* base = nullptr;
    size_t cap = 0;
    unsigned gen = 0;              // allocations so far (what a caller that remembers "I zeroed this part" compares)
    int reserve(size_t bytes) {
        if (bytes <= cap) return QOIMI_OK;
        if (base) { (void)hipFree(base); base = nullptr; cap = 0; }
        // (a quarter more than asked for, so that calls of slowly growing batches do not reallocate every time - but no more than 256 MiB:
        // the decode arena of the 1024-frame 4K shard is 45 GB, its margin was another 11)
        const size_t slack = bytes / 4 < ((size_t)256 << 20) ? bytes / 4 : ((size_t)256 << 20);
        size_t want = bytes + slack + (1u << 20);
        HIP_TRY(hipMalloc(&base, want));
        cap = want; ++gen;
        return QOIMI_OK;
    }
    void release() { if (base) (void)hipFree(base); base = nullptr; cap = 0; }
};

// Pinned host staging: grown to what is asked for plus a page, never shrunk; what it held is not kept.
struct PinBuf {
    void* buf = nullptr; size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return QOIMI_OK;
        release();
        HIP_TRY(hipHostMalloc(&buf, bytes + 4096));
        cap = bytes + 4096;
        return QOIMI_OK;
    }
    void release() { if (buf) (void)hipHostFree(buf); buf = nullptr; cap = 0; }
};

// An arena of exactly what is asked for plus a page (the staging of qoimi_verify_images: the caller states its size).
static int reserve_exact(Arena& a, size_t bytes) {
    if (bytes <= a.cap) return QOIMI_OK;
    a.release();
    HIP_TRY(hipMalloc(&a.base, bytes + 4096u));
    a.cap = bytes + 4096u; ++a.gen;
    return QOIMI_OK;
}

struct Carver {   // hands out 256-byte aligned pieces of an arena
    uint8_t* base; size_t off = 0;
    explicit Carver(void* b) : base((uint8_t*)b) {}
    template <class T> T* take(size_t count) {
        off = (off + 255u) & ~(size_t)255u;
        T* p = base ? (T*)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

struct qoimi_ctx {
    int device = 0;
    int n_cus = 256;            // compute units of the device (the grid of the pack's copy)
    Arena enc_ws, dec_ws;       // kernel workspaces
    Arena enc_stage;            // qoimi_encode_packed: the strided streams of one sub-batch (and the source offsets of a mixed-shape call) on their way into the pack;
                                // qoimi_encode_tiles: the same, every stream behind the gathered pixels of its tile, and the tile table
    long long tile_stats[4] = {0, 0, 0, 0};    // the last qoimi_encode_tiles call: sub-batches, launches of tile_gather (of tile_select in the label modes), bytes of staging planned, images referenced
    Arena insp_ws;              // tables, maps and partial counts of qoimi_inspect_streams (its own: a decode call finds dec_ws as it left it)
    Arena cmp_ws;               // image table and result table of qoimi_compare_images / qoimi_verify_images; the table (and results) of run_staged and of the band assembly
    Arena ver_stage;            // qoimi_verify_images and every call of run_staged (qoi_staged.h: thumbnails, crops, resized, bilinear, warped, pixel statistics, the seek index build): the decoded pixels of one sub-batch (sized to the plan's largest sub-batch plus a page: no slack)
    long long thumb_stats[4] = {0, 0, 0, 0};   // the last qoimi_decode_thumbnails call: sub-batches decoded, launches of thumb_reduce, bytes of staging planned, 0
    long long crop_stats[4] = {0, 0, 0, 0};    // the last qoimi_decode_crops call: sub-batches decoded, launches of crop_gather, bytes of staging planned, images decoded
    long long resize_stats[4] = {0, 0, 0, 0};  // the last qoimi_decode_resized call: sub-batches decoded, launches of resize_filter, bytes of staging planned, images decoded
    long long warp_stats[4] = {0, 0, 0, 0};   // the last qoimi_decode_warped call: sub-batches decoded, launches of warp_gather, bytes of staging planned, images decoded
    long long tensor_stats[4] = {0, 0, 0, 0};   // the last qoimi_decode_tensors or qoimi_decode_warped_tensors call: sub-batches decoded, launches of its tensor kernel, bytes of staging planned, images decoded
    long long bilinear_stats[4] = {0, 0, 0, 0};   // the last qoimi_decode_bilinear call: sub-batches decoded, launches of bilinear_filter, bytes of staging planned, images decoded
    Arena band_arena;           // the four *_indexed calls (qoi_host_seek.hip: stage_bands): the band streams of one call (the sum of their sizes, each rounded up to 16, plus a page)
    long long seek_stats[4] = {0, 0, 0, 0};    // sub-batches decoded by the last qoimi_build_seek_index; of the last qoimi_make_band_streams / *_indexed call: band streams assembled, bytes of the band arena planned, stream bytes copied
    long long pixel_stats[4] = {0, 0, 0, 0};   // the last qoimi_pixel_stats call: sub-batches decoded, launches of stats_reduce, bytes of staging planned, images decoded
    PinBuf cmp_pin;             // pinned staging of the tables and results of qoimi_compare_images, qoimi_verify_images, run_staged and the band assembly
                                // (their own: the decode calls inside them reuse pin at once)
    Arena dec_scan;             // look-back words of dec_scan_entry (calls of a few images): tagged with dec_epoch, zeroed when allocated / when the tag wraps
    uint32_t dec_epoch = 0;     // number of the last such call (16 bits are compared)
    struct { void* at = nullptr; unsigned gen = 0; bool valid = false; } dec_hdr_zero;   // the counter header the last decode call's dec_fill left zeroed (arena base + generation)
    void* dec_tail_stream = nullptr; bool dec_tail_open = false;   // a decode call returned on its pinned result words while its last launch was still retiring on this stream
    Arena io_a, io_b, io_c;     // staging for the host-pointer (drop-in) path
    uint32_t* host_word = nullptr;   // pinned words for read-backs
    hipStream_t own_stream = nullptr; // private non-blocking stream: self-test at creation, the drop-in entry points' work
    PinBuf pin;                 // pinned staging for small host->device tables
    long long dec_stats[4] = {0, 0, 0, 0};
    uint32_t seg_bytes = 0;     // decode segment size; 0: chosen per call from the batch's stream bytes
    uint32_t* last_enc_err = nullptr;   // device flag of the most recent encode launch
    uint32_t* last_enc_err2 = nullptr;  // ... of the other channel group of a qoimi_encode_images call that held 3- and 4-channel images
    PinBuf enc_pin; hipEvent_t enc_pin_ev = nullptr;   // pinned staging of qoimi_encode_images' tables (its own: the call is
                                        // asynchronous, decode calls reuse pin at once) and the event behind the last copies out of it
    bool xchg_ordered = false;          // result of the LDS exchange-order self-test (enc_slabs PROBE 1)
    long long enc_calls = 0;            // encode calls so far: the self-test is repeated every enc_recheck_every of them
    long long enc_calls_at_check = 0;   // ... as of the launch of the repeat in flight (or of the last one)
    long long enc_calls_last_passed = 0;   // ... as of the launch of the last repeat that PASSED (0: the test at creation)
    long long enc_recheck_every = 256, enc_suspect_calls = 0;   // env QOIMI_ENC_RECHECK_EVERY
    bool recheck_pending = false;       // a repeated self-test is in flight on own_stream, result in host_word[8]
    bool recheck_failed_unreported = false;   // a repeat failed: the next qoimi_encode_status reports it (once)
    bool test_force_recheck_fail = false;     // env QOIMI_TEST_FORCE_RECHECK_FAIL (tests): every repeat counts as failed
    int enc_ticket = 1, enc_set_slabs = 0, enc_warm = 1;   // tuning / test knobs (env QOIMI_ENC_*)
    bool dropin = false;                // the context of a thread's qoi_encode / qoi_decode calls (thread_ctx)
    int enc_tree_ticket = -1;           // -1: 1 for qoimi_encode_batch, 0 inside the drop-in qoi_encode.  1: tree placement hands its units out by one ticket per workgroup (start order: no assumption about the dispatcher); 0 (QOIMI_ENC_TREE_TICKET=0,
                                        // and always inside the drop-in qoi_encode, which encodes again by itself): by workgroup index, 4 us less per 4K frame
    int dec_tr_scan = 0;                // env QOIMI_DEC_TR_SCAN=1 (experiment, measured SLOWER: 46.6 us against 24.5 + 20.3 on a lone 4K frame, profiles/r06_s15): dec_scan_entry's
                                        // work as the epilogue of the two-lane transcoder instead of a launch of its own
    bool dec_few_longruns = false;      // the context's last call of up to four images on the single-pass path met 1024 long QOI_OP_RUNs or more: the next one takes run descriptors
    bool dec_few_syncfail = false;      // the context's last call of up to four images held segments its transcoder could not synchronise: see decode_some
    int dec_fused_adapt = 1;            // env QOIMI_DEC_FUSED_ADAPT=0: such calls try the single-pass path every time
    bool dec_nonflat_repair = false;    // the context's last call of more than four images (flat ones aside) needed a repair round: see choose_seg_bytes
    int dec_class_split = 1;            // env QOIMI_DEC_CLASS_SPLIT=0: a call that mixes flat images with others is one pass over all of them (round 5)
    int dec_small_seg = 1;              // env QOIMI_DEC_SMALL_SEG=0: calls of a few images never below 128-byte segments
    int dec_conv = 1;                   // env QOIMI_DEC_CONV=0: refinement passes run to their count (1: they stop at a fixed point, DecParams::conv)
    int dec_s3_ride = 0;                // env QOIMI_DEC_S3_RIDE=1 (experiment, measured: 21.6 -> 20.7 us for the two levels on a lone 4K frame, profiles/r06_s14): the per-image
                                        // level of the state chain rides on the group level's launch (last arrivers) instead of dec_chain_state_l2p's own launch
    int dec_split_max = 512;            // env QOIMI_DEC_SPLIT_MAX: the largest segment of a call of a few images that takes two transcoder lanes (128 / 256 / 512 / 1024: a 5120 x 2880 photograph 211 / 200 / 199 / 198 us, a 4K noise frame 208 / 208 / 197 / 199, 8192^2 510 / 519 / 544 / 546 - it takes 1 KiB - profiles/r06_s44_split_max.txt)
    int dec_split = 1;                  // env QOIMI_DEC_SPLIT=0: one transcoder lane per segment in those calls too
    int dec_fused = 1;                  // env QOIMI_DEC_FUSED=0: calls of a few images take the three-level chains of the batch path instead of the single-pass look-back kernels
    uint32_t test_spin_bound = 0;       // env QOIMI_TEST_SPIN_BOUND (tests): polls before a placement wait gives up
    bool tight_buffer = false;          // env QOIMI_ENCODE_TIGHT_BUFFER=1 (read once, at creation): qoi_encode sizes its result by the thread's previous stream instead of
                                        // returning the reference's worst-case allocation (qoi.h:374-379)
    int enc_gen_slabs = 0;              // env QOIMI_ENC_GEN_SLABS (1..16): slabs per set of the pass over flagged images; 0: kEncGenSetSlabs, twice that for
                                        // calls of 3 x 65536 slabs and more (8 / 12 / 16 slabs, 1024 frames: constant 7.69 / 7.34 / 6.75 ms, uiflat 20.62 / 20.49 / 20.34,
                                        // 512 sprites 8.86 / 8.70 / 8.76 - profiles/r05_s22_enc_gen_slabs16.txt; a single frame has too few sets for that)
    int enc_gen_small_div = 0;          // env QOIMI_ENC_GEN_GRID_DIV (0: 32)
    int enc_gen_grid_div = 1;           // (32 / 4 / 1: uiflat 21.3 / 21.2 / 20.4 ms, sprite_alpha 11.0 / 11.1 / 10.1 per 512, profiles/r05_s14_enc_grid.txt) env QOIMI_ENC_GEN_GRID_HOT: the pass over flagged images runs with 1/N of its units when the previous batch held flagged images
    int enc_uni = -1;                   // one encode pass, sets whose look-back window does not do take the state look-back one by one.  -1: for calls of a few
                                        // images (tree placement) behind a call that met flat stretches (host_word[14]); env QOIMI_ENC_UNI=1 always / 0 never
    int enc_prezero = 1;                // env QOIMI_ENC_PREZERO=0: calls of a few images zero their records with hipMemsetAsync every time (see enc_sets: zero_next)
    struct { void* ptr = nullptr; size_t bytes = 0; unsigned gen = 0; long long seq = -1; bool valid = false; } prezero;   // the region the last such call zeroed for its successor
    long long enc_ws_seq = 0;           // calls that laid out the encode workspace so far (a zeroed region is good for the very next one only)
    int enc_parity = 0;                 // which of the two regions the next call of a few images takes
    int enc_all_g2 = 1;                 // env QOIMI_ENC_ALL_G2=0: a batch behind a batch of flagged images only still runs its first pass (with a sixteenth of its workgroups)
    int enc_g2 = 1;                     // env QOIMI_ENC_G2=0: flagged images (flat content) go through the summary passes instead of the state look-back (ENTRY 2)
    uint32_t enc_epoch = 0;             // encode call number: the tag of the state look-back's granules
    void* g2_zeroed_at = nullptr; size_t g2_zeroed_bytes = 0; unsigned g2_zeroed_gen = 0;     // where those granules were last zeroed
    int enc_adapt = 1;                  // env QOIMI_ENC_ADAPT=0: the set size ignores what the previous call's streams looked like
    uint32_t enc_hint_images = 0;       // images of the batch call whose count of flagged images stands in host_word[13]
    uint32_t enc_hint_npx = 0;          // pixels per image of the batch call whose first stream length stands in host_word[12] (0: none)
    bool enc_heavy_before = false, enc_flagged_before = false;   // what the batch BEFORE the previous one looked like: a hint acts only when two batches in a row agree
    struct { const void* px; size_t ps; qoi_desc desc; int n; void* out; size_t os; int* len; void* st; bool valid = false; } last_enc;   // the last qoimi_encode_batch (qoimi_encode_status re-encodes it order-free if a wait gave up)
    int enc_spread = 1;                 // env QOIMI_ENC_SPREAD: the wavefronts of a workgroup take their tickets from consecutive images (0: all four from one image)
    int enc_pipe = 0;                   // env QOIMI_ENC_PIPE=1 (experiment, with QOIMI_ENC_PERSIST): next set's loads ahead of the current set's placement
    int enc_persist = 0;                // env QOIMI_ENC_PERSIST: workgroups of the first encode pass (0: one per unit)
    int enc_lookback = -1;              // 1: sets place their bytes themselves (decoupled look-back); 2: the same by the tree of byte counts; 0: order-free (scratch slots + enc_offsets + enc_compact); -1: by the call's shape
    std::string enc_debug_dump;         // env QOIMI_ENC_DEBUG_DUMP: file that receives the entry-state arrays of every encode call
    std::string dec_debug_dump;         // env QOIMI_DEC_DEBUG_DUMP: file that receives the per-segment arrays (granule counts, parse records, pixel offsets) of every decode call
    int dec_refine = 1;                 // 0: rounds after a failed check re-speculate from scratch (no alpha hints)
    int dec_fine = 1;                   // 0: lane-per-segment P1/P2 even where the 128-byte piece kernels apply
    int dec_p3_plain = 1, dec_inner = 8, dec_inner1 = 3;   // env QOIMI_P3_PLAIN, QOIMI_DEC_INNER, QOIMI_DEC_INNER1 (read once, at creation)
                                                           // (dec_inner 4 / 8 / 16 on 1024 UI frames: 3 / 2 / 2 rounds in 19.4 / 18.6 / 23.2 ms, profiles/r05_s9_dec_uiflat_inner.txt)
    int dec_l2_wgs = 1;          // dec_chain_state_l2m: 0 never, 1 for calls of up to four images of 128 groups or more, 2 for every call of up to four images (env QOIMI_DEC_L2M, tests)
    int dec_flat_seg = 1;        // 0: calls of flat images take the segment size of the general cost model (env QOIMI_DEC_FLAT_SEG, A/B)
    int dec_run_desc = 2;        // env QOIMI_DEC_RUN_DESC - 0: every long run is written lane by lane; 1: run descriptors for flat images; 2: and a descriptor per long QOI_OP_RUN chunk of the other images
    int dec_max_rounds = kMaxSpecRounds;   // speculation rounds before the sequential last resort (env QOIMI_DEC_MAX_ROUNDS, tests)
    size_t last_drop_len = 0;           // length of the last stream the drop-in qoi_encode returned on this context (page populate-ahead)
    long long enc_retries = 0;          // calls qoimi_encode_status encoded again order-free after a placement wait gave up
    long long dec_seq_images = 0;       // images finished by dec_sequential since the context was created
    size_t dec_rec_cap = (size_t)16 << 30;   // largest record arena: a call whose streams need more is decoded in sub-batches (set from the device's memory at creation)
    KernelTimer timer;                  // optional per-kernel HIP-event timing
    double prof_ms[kT_count] = {0};     // accumulated kernel milliseconds since profiling was (re)enabled
    long long prof_calls[kT_count] = {0};
};

static const size_t kPixelCap = 400000000u;   // QOI_PIXELS_MAX, qoi.h:332

static bool desc_ok(const qoi_desc* d) {       // qoi.h:366-369 / 514-518
    return d && d->width != 0 && d->height != 0 && d->channels >= 3 && d->channels <= 4 &&
           d->colorspace <= 1 && d->height < kPixelCap / d->width;
}

// The output channel count a decoding call takes: 0 (each image's own), 3 or 4.  QOIMI_OK, or the failure.
static int check_out_channels(int channels) {
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    return QOIMI_OK;
}

// The workgroups of a launch whose workgroups walk `tiles` tiles between them: one per tile, eight per compute unit at the most.
static uint32_t grid_bound(const qoimi_ctx* c, uint64_t tiles) {
    const uint32_t most = (uint32_t)c->n_cus * 8u;
    return tiles < most ? (uint32_t)tiles : most;
}

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// The 14 header bytes of a stream by the rules of qoi.h:505-521: *desc is filled whatever they hold; true if a decoder accepts them.
static bool parse_header(const uint8_t* bytes, qoi_desc* desc) {
    const bool magic_ok = memcmp(bytes, "qoif", 4) == 0;
    desc->width = be32(bytes + 4);                                        // filled before validation, qoi.h:507-511
    desc->height = be32(bytes + 8);
    desc->channels = bytes[12];
    desc->colorspace = bytes[13];
    return desc_ok(desc) && magic_ok;                                     // qoi.h:513-521
}

// fold the recorded events into the accumulators (the stream must be idle)
static void timer_collect(qoimi_ctx* c) {
    {
        KernelTimer& t = c->timer;
        int open_total = -1;                           // index of the kT_begin a kT_enc_total / kT_dec_total mark closes
        for (int i = 0; i < t.n; ++i) {
            if (t.tag[i] == kT_begin) { if (open_total < 0) open_total = i; continue; }
            float ms = 0;
            if (t.tag[i] == kT_enc_total || t.tag[i] == kT_dec_total) {
                if (open_total >= 0 && hipEventElapsedTime(&ms, t.ev[open_total], t.ev[i]) == hipSuccess) { c->prof_ms[t.tag[i]] += ms; c->prof_calls[t.tag[i]] += 1; }
                open_total = -1;
                continue;
            }
            if (i > 0 && hipEventElapsedTime(&ms, t.ev[i - 1], t.ev[i]) == hipSuccess) { c->prof_ms[t.tag[i]] += ms; c->prof_calls[t.tag[i]] += 1; }
        }
        t.n = 0;
    }
}

// ---- what entry points begin with (forced inline: a call that needs none of it pays a compare, as when these lines stood in every entry point) ----
// The previous decode call of this context may have returned on its pinned result words while its last launch was still retiring (see
// decode_some).  On the same stream the work that follows is ordered behind it; a caller that changes streams gets the wait here.
static __forceinline__ int wait_decode_tail(qoimi_ctx* c, void* stream) {
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    return QOIMI_OK;
}

// room for the marks of one more call's launches: when the timer is nearly full, the stream is waited for and the events are folded
static __forceinline__ int timer_room(qoimi_ctx* c, hipStream_t st) {
    if (c->timer.n > KernelTimer::kMax - 32) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
    return QOIMI_OK;
}

// The repeat of the LDS-order self-test (launched by qoimi_encode_batch on the context's private stream): its result, once it is there.
// report: the failure is also left as the thread's last error.
static __forceinline__ void enc_poll_recheck(qoimi_ctx* c, bool report) {
    if (!c->recheck_pending || hipStreamQuery(c->own_stream) != hipSuccess) return;
    c->recheck_pending = false;
    if (c->host_word[8] != 0u || c->test_force_recheck_fail) {
        // Never observed.  The context switches to the order-free probe for good and THIS call is encoded with it (its own
        // stream is sound, the call does not fail); what cannot be undone is reported: every call since the launch of the last
        // repeat that PASSED is suspect - the ones before the failed repeat was launched and the ones made while it ran
        // (enc_calls still excludes the call at hand) - and the next qoimi_encode_status returns QOIMI_E_INTERNAL once.
        c->xchg_ordered = false;
        c->enc_suspect_calls += c->enc_calls - c->enc_calls_last_passed;
        c->enc_calls_last_passed = c->enc_calls;
        c->recheck_failed_unreported = true;
        if (report) (void)fail(QOIMI_E_INTERNAL, "the LDS exchange-order self-test failed on repetition: streams encoded since the last passed check are suspect (qoimi_encode_suspect_calls); this context now uses the order-free probe");
    } else c->enc_calls_last_passed = c->enc_calls_at_check;
}

// The tables of the inspect passes (qoi_inspect.hip) for n streams: a stream shorter than 22 bytes is not read, a block is up to kInsBlock
// bytes of ONE stream's body, its pieces are numbered through the call.
static inline void ins_fill_tables(const size_t* stream_offsets, const int* sizes, size_t n, InsStream* h_tab, InsBlock* h_blk) {
    const int kMin = kHeaderBytes + kTrailerBytes;
    uint32_t b = 0, pc = 0;
    for (size_t i = 0; i < n; ++i) {
        h_tab[i].off = sizes[i] >= kMin ? (u64)stream_offsets[i] : ~0ull;
        h_tab[i].size = (uint32_t)sizes[i]; h_tab[i].first_blk = b;
        if (sizes[i] <= kMin) continue;
        const uint32_t body = (uint32_t)(sizes[i] - kMin);
        for (uint32_t at = 0; at < body; at += kInsBlock) {
            const uint32_t len = body - at < kInsBlock ? body - at : kInsBlock;
            h_blk[b].off = (u64)stream_offsets[i] + (u64)kHeaderBytes + at;
            h_blk[b].len = len | (at == 0 ? kInsFirst : 0u);
            h_blk[b].piece_base = pc;
            ++b; pc += (len + kInsPiece - 1u) / kInsPiece;
        }
    }
}

// a call's four counters (a NULL context: zeros)
static inline void copy_stats(const long long* from, long long out[4]) { for (int i = 0; i < 4; ++i) out[i] = from ? from[i] : 0; }

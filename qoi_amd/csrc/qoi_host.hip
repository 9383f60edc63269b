// qoi_host.hip — C-ABI shim of libqoi_mi355x.so (include/qoi_mi355x.h).
//
// Part 1 mirrors the reference's public functions (qoi.h:252,265,278,289): identical
// argument validation, malloc()-owned results, NULL / 0 on failure.  Part 2 is the
// additive device-resident batch API.  There is NO CPU codec in this library: every
// pixel/stream byte is produced by the gfx950 kernels, and all entry points fail when
// no GPU is usable.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <mutex>
#include <algorithm>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

// The library is built with -fvisibility=hidden: what the header declares is the whole exported surface (tests/test_abi.py
// reads it back with nm -D).
#pragma GCC visibility push(default)
#include "../../include/qoi_mi355x.h"
#pragma GCC visibility pop
#include "qoi_decode_core.h"
#include "qoi_kernels.h"
#include "qoi_stage_plan.h"   // the plans of the calls that work through bounded staging: host arithmetic alone, tested without a GPU
#include "qoi_pack.hip"        // the pack kernels and their launchers: part of this translation unit (no build lists the file itself)
#include "qoi_inspect.hip"     // ... and the kernels of qoimi_inspect_streams, the same way
#include "qoi_compare.hip"     // ... and those of qoimi_compare_images / qoimi_verify_images
#include "qoi_thumb.hip"       // ... and the box reduction of qoimi_decode_thumbnails
#include "qoi_crop.hip"        // ... and the gather of qoimi_decode_crops
#include "qoi_resize.hip"      // ... and the area filter of qoimi_decode_resized
#include "qoi_stats.hip"       // ... and the reduction of qoimi_pixel_stats

using namespace qoimi;

// ------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------
static thread_local std::string t_error;
static int fail(int code, const std::string& msg) { t_error = msg; return code; }
#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? QOIMI_E_NOMEM                             \
                        : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice || e_ == hipErrorInsufficientDriver) ? QOIMI_E_NO_GPU \
                        : QOIMI_E_INTERNAL,                                                    \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)

extern "C" const char* qoimi_last_error(void) { return t_error.c_str(); }

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
extern "C" const char* qoimi_version(void) { return "qoi_mi355x 0.1 gfx950"; }

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
    Arena enc_stage;            // qoimi_encode_packed: the strided streams of one sub-batch (and the source offsets of a mixed-shape call) on their way into the pack
    Arena insp_ws;              // tables, maps and partial counts of qoimi_inspect_streams (its own: a decode call finds dec_ws as it left it)
    Arena cmp_ws;               // image table and result table of qoimi_compare_images / qoimi_verify_images
    Arena ver_stage;            // qoimi_verify_images / qoimi_decode_thumbnails / qoimi_decode_crops / qoimi_decode_resized / qoimi_pixel_stats: the decoded pixels of one sub-batch (sized to the plan's largest sub-batch plus a page: no slack)
    long long thumb_stats[4] = {0, 0, 0, 0};   // the last qoimi_decode_thumbnails call: sub-batches decoded, launches of thumb_reduce, bytes of staging planned, 0
    long long crop_stats[4] = {0, 0, 0, 0};    // the last qoimi_decode_crops call: sub-batches decoded, launches of crop_gather, bytes of staging planned, images decoded
    long long resize_stats[4] = {0, 0, 0, 0};  // the last qoimi_decode_resized call: sub-batches decoded, launches of resize_filter, bytes of staging planned, images decoded
    long long pixel_stats[4] = {0, 0, 0, 0};   // the last qoimi_pixel_stats call: sub-batches decoded, launches of stats_reduce, bytes of staging planned, images decoded
    void* cmp_pin_buf = nullptr; size_t cmp_pin_cap = 0;   // pinned staging of those two calls' tables and results (their own: the decode calls inside
                                // qoimi_verify_images reuse pin_buf at once)
    Arena dec_scan;             // look-back words of dec_scan_entry (calls of a few images): tagged with dec_epoch, zeroed when allocated / when the tag wraps
    uint32_t dec_epoch = 0;     // number of the last such call (16 bits are compared)
    struct { void* at = nullptr; unsigned gen = 0; bool valid = false; } dec_hdr_zero;
    void* dec_tail_stream = nullptr; bool dec_tail_open = false;   // a decode call returned on its pinned result words while its last launch was still retiring on this stream   // the counter header the last decode call's dec_fill left zeroed (arena base + generation)
    Arena io_a, io_b, io_c;     // staging for the host-pointer (drop-in) path
    uint32_t* host_word = nullptr;   // pinned words for read-backs
    hipStream_t own_stream = nullptr; // private non-blocking stream: self-test at creation, the drop-in entry points' work
    void* pin_buf = nullptr; size_t pin_cap = 0;   // pinned staging for small host->device tables
    long long dec_stats[4] = {0, 0, 0, 0};
    uint32_t seg_bytes = 0;     // decode segment size; 0: chosen per call from the batch's stream bytes
    uint32_t* last_enc_err = nullptr;   // device flag of the most recent encode launch
    uint32_t* last_enc_err2 = nullptr;  // ... of the other channel group of a qoimi_encode_images call that held 3- and 4-channel images
    void* enc_pin_buf = nullptr; size_t enc_pin_cap = 0; hipEvent_t enc_pin_ev = nullptr;   // pinned staging of qoimi_encode_images' tables (its own: the call is
                                        // asynchronous, decode calls reuse pin_buf at once) and the event behind the last copies out of it
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

extern "C" size_t qoimi_encode_bound(const qoi_desc* desc) {
    if (!desc_ok(desc)) return 0;
    return (size_t)desc->width * desc->height * (desc->channels + 1u) + kHeaderBytes + kTrailerBytes;
}

extern "C" int qoimi_ctx_create(int device, qoimi_ctx** out) {
    if (!out) return fail(QOIMI_E_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(QOIMI_E_NO_GPU, "no such GPU device");
    DeviceGuard guard(device);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(QOIMI_E_NO_GPU, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    qoimi_ctx* c = new qoimi_ctx();
    c->device = device;
    if (prop.multiProcessorCount > 0) c->n_cus = prop.multiProcessorCount;
    {   // record arena of a decode call: up to a sixth of the device's memory (48 GiB on a 288 GB MI355X: the 1024-frame shard of
        // BASELINE configs[4] in one piece, 45.1 GB of workspace = 4.3 x its stream bytes at 36.4 ms), never less than 1 GiB.  A caller
        // short of device memory caps it (QOIMI_DEC_REC_CAP_MB): 24 GiB = two sub-batches, 27.4 GB = 2.6 x the stream bytes at 36.8 ms
        // (+1 %: every kernel's tail twice), 16 GiB = three, 18.3 GB at 37.1 ms (profiles/r05_s17_dec_cap.txt, r05_s27_dec_cap_wall.txt).
        // The default was 24 GiB for sessions 24-34 of round 5: 172.8 Gpx/s (median of six runs on five boxes) against 176 in one piece.
        size_t cap = (size_t)prop.totalGlobalMem / 6u;
        if (cap > ((size_t)48 << 30)) cap = (size_t)48 << 30;
        if (cap < ((size_t)1 << 30)) cap = (size_t)1 << 30;
        c->dec_rec_cap = cap;
    }
    if (hipHostMalloc((void**)&c->host_word, 256) != hipSuccess) { delete c; return fail(QOIMI_E_NOMEM, "hipHostMalloc failed"); }
    // Measure (do not assume) the LDS conflict order the fast colour-table probe relies on.
    {
        hipStream_t pst = nullptr;
        if (hipStreamCreateWithFlags(&pst, hipStreamNonBlocking) != hipSuccess) { (void)hipHostFree(c->host_word); delete c; return fail(QOIMI_E_NO_GPU, "hipStreamCreate failed"); }
        c->own_stream = pst;           // also the stream of the drop-in entry points (one context per calling thread)
        c->xchg_ordered = run_lds_order_selftest(pst) == 0;
    }
    c->host_word[12] = 0u; c->host_word[13] = 0u; c->host_word[14] = 0u; c->host_word[15] = 0u;
    // Documented settings: the order-independent colour-table probe from the start; the tight result buffer of qoi_encode.
    if (const char* e = getenv("QOIMI_ENC_PROBE")) { if (atoi(e) == 0) c->xchg_ordered = false; }
    if (const char* e = getenv("QOIMI_ENCODE_TIGHT_BUFFER")) c->tight_buffer = atoi(e) != 0;
    // Everything else in the environment is a measurement / test knob and is looked at only under QOIMI_TUNING=1 (tests/conftest.py and
    // tools/measure set it): an inherited QOIMI_* variable cannot change kernels, segment sizes or placement of a production process.
    const char* tune = getenv("QOIMI_TUNING");
    if (tune && atoi(tune) != 0) {
        auto knob = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
        auto flag = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e) != 0; };
        if (const char* e = getenv("QOIMI_ENC_RECHECK_EVERY")) { long v = atol(e); if (v >= 1) c->enc_recheck_every = v; }
        knob("QOIMI_ENC_TICKET", c->enc_ticket); knob("QOIMI_ENC_SET_SLABS", c->enc_set_slabs); knob("QOIMI_ENC_WARM", c->enc_warm);
        knob("QOIMI_ENC_LOOKBACK", c->enc_lookback);
        if (const char* e = getenv("QOIMI_ENC_DEBUG_DUMP")) c->enc_debug_dump = e;
        if (const char* e = getenv("QOIMI_DEC_DEBUG_DUMP")) c->dec_debug_dump = e;
        flag("QOIMI_ENC_SPREAD", c->enc_spread); flag("QOIMI_ENC_TREE_TICKET", c->enc_tree_ticket); flag("QOIMI_ENC_ADAPT", c->enc_adapt);
        flag("QOIMI_ENC_G2", c->enc_g2); flag("QOIMI_ENC_ALL_G2", c->enc_all_g2); flag("QOIMI_ENC_PREZERO", c->enc_prezero); flag("QOIMI_ENC_UNI", c->enc_uni);
        flag("QOIMI_ENC_PIPE", c->enc_pipe);
        if (const char* e = getenv("QOIMI_ENC_GEN_GRID_DIV")) { const int v = atoi(e); if (v >= 1) c->enc_gen_small_div = v; }
        if (const char* e = getenv("QOIMI_ENC_GEN_GRID_HOT")) { const int v = atoi(e); if (v >= 1) c->enc_gen_grid_div = v; }
        if (const char* e = getenv("QOIMI_ENC_GEN_SLABS")) { const int v = atoi(e); if (v >= 1 && v <= (int)kEncMaxSetSlabs) c->enc_gen_slabs = v; }
        if (const char* e = getenv("QOIMI_ENC_PERSIST")) { const int v = atoi(e); if (v >= 0) c->enc_persist = v; }
        knob("QOIMI_DEC_FINE", c->dec_fine); knob("QOIMI_DEC_REFINE", c->dec_refine); knob("QOIMI_P3_PLAIN", c->dec_p3_plain);
        if (const char* e = getenv("QOIMI_DEC_INNER")) { const int v = atoi(e); if (v >= 0 && v <= 64) c->dec_inner = v; }
        if (const char* e = getenv("QOIMI_DEC_INNER1")) { const int v = atoi(e); if (v >= 0 && v <= 64) c->dec_inner1 = v; }
        knob("QOIMI_DEC_L2M", c->dec_l2_wgs); knob("QOIMI_DEC_RUN_DESC", c->dec_run_desc); knob("QOIMI_DEC_FLAT_SEG", c->dec_flat_seg);
        knob("QOIMI_DEC_FUSED", c->dec_fused); knob("QOIMI_DEC_SPLIT", c->dec_split); knob("QOIMI_DEC_S3_RIDE", c->dec_s3_ride); knob("QOIMI_DEC_TR_SCAN", c->dec_tr_scan); knob("QOIMI_DEC_CONV", c->dec_conv); knob("QOIMI_DEC_SMALL_SEG", c->dec_small_seg); knob("QOIMI_DEC_CLASS_SPLIT", c->dec_class_split); knob("QOIMI_DEC_FUSED_ADAPT", c->dec_fused_adapt);
        if (const char* e = getenv("QOIMI_DEC_SPLIT_MAX")) { const int v = atoi(e); if (v >= 64 && v <= 4096) c->dec_split_max = v; }
        if (const char* e = getenv("QOIMI_DEC_MAX_ROUNDS")) { int v = atoi(e); if (v >= 1) c->dec_max_rounds = v; }
        if (const char* e = getenv("QOIMI_DEC_REC_CAP_MB")) { long v = atol(e); if (v >= 1) c->dec_rec_cap = (size_t)v << 20; }
        if (const char* e = getenv("QOIMI_SEG_BYTES")) { long v = atol(e); if (v >= 64 && v <= (1 << 20)) c->seg_bytes = (uint32_t)v; }
    }
#ifdef QOIMI_TEST_HOOKS
    // failure injection, compiled into the test flavour of the library only (make TEST_HOOKS=1 -> libqoi_mi355x_test.so)
    if (const char* e = getenv("QOIMI_TEST_FORCE_RECHECK_FAIL")) c->test_force_recheck_fail = atoi(e) != 0;
    if (const char* e = getenv("QOIMI_TEST_SPIN_BOUND")) { const long v = atol(e); if (v >= 1) c->test_spin_bound = (uint32_t)v; }
#endif
    *out = c;
    return QOIMI_OK;
}

extern "C" void qoimi_ctx_destroy(qoimi_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    (void)hipDeviceSynchronize();       // calls still in flight write to the arenas and to the pinned words freed below
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    c->enc_ws.release(); c->enc_stage.release(); c->dec_ws.release(); c->insp_ws.release(); c->cmp_ws.release(); c->ver_stage.release(); c->dec_scan.release(); c->io_a.release(); c->io_b.release(); c->io_c.release();
    if (c->host_word) (void)hipHostFree(c->host_word);
    if (c->pin_buf) (void)hipHostFree(c->pin_buf);
    if (c->enc_pin_buf) (void)hipHostFree(c->enc_pin_buf);
    if (c->cmp_pin_buf) (void)hipHostFree(c->cmp_pin_buf);
    if (c->enc_pin_ev) (void)hipEventDestroy(c->enc_pin_ev);
    delete c;
}

extern "C" int qoimi_set_decode_record_cap(qoimi_ctx* c, size_t bytes, int release) {
    if (!c || bytes < ((size_t)1 << 20)) return fail(QOIMI_E_ARG, "record cap: NULL context or less than 1 MiB");
    c->dec_rec_cap = bytes;
    if (release) {
        DeviceGuard guard(c->device);
        (void)hipDeviceSynchronize();
        c->dec_ws.release();
    }
    return QOIMI_OK;
}

// Per-kernel timing with HIP events on the launch stream.  on=1 resets the accumulators.
extern "C" int qoimi_set_profiling(qoimi_ctx* c, int on) {
    if (!c) return fail(QOIMI_E_ARG, "ctx is NULL");
    DeviceGuard guard(c->device);
    if (on && !c->timer.created) {
        for (int i = 0; i < KernelTimer::kMax; ++i) HIP_TRY(hipEventCreate(&c->timer.ev[i]));
        c->timer.created = true;
    }
    c->timer.on = on != 0;
    c->timer.n = 0;
    if (on) for (int i = 0; i < kT_count; ++i) { c->prof_ms[i] = 0; c->prof_calls[i] = 0; }
    return QOIMI_OK;
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

// Synchronises `stream`, then copies accumulated milliseconds and launch counts per kernel
// (index = position in qoimi_kernel_name).  Returns the number of kernels.
extern "C" int qoimi_get_profile(qoimi_ctx* c, void* stream, double* ms, long long* calls, int cap) {
    if (!c) return fail(QOIMI_E_ARG, "ctx is NULL");
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    timer_collect(c);
    for (int i = 0; i < kT_count && i < cap; ++i) { if (ms) ms[i] = c->prof_ms[i]; if (calls) calls[i] = c->prof_calls[i]; }
    return kT_count;
}

extern "C" const char* qoimi_kernel_name(int i) {
    static const char* names[kT_count] = {"", "enc_slab_summary", "enc_scan_groups", "enc_scan_images", "enc_slabs", "enc_slabs_generic", "enc_offsets", "enc_compact",
        "dec_parse", "dec_chain_parse", "dec_transcode", "dec_chain_slots", "dec_summarize", "dec_chain_state",
        "dec_segments", "dec_prepare_restart", "dec_fill", "dec_expand_runs", "pack_offsets", "pack_copy",
        "inspect_maps", "inspect_scan", "inspect_count", "inspect_reduce", "pack_offsets_append", "pack_copy_append", "encode_total", "decode_total", "cmp_pixels", "cmp_first"};
    return (i >= 0 && i < kT_count) ? names[i] : "";
}

extern "C" long long qoimi_encode_suspect_calls(qoimi_ctx* c) { return c ? c->enc_suspect_calls : 0; }
extern "C" long long qoimi_encode_retries(qoimi_ctx* c) { return c ? c->enc_retries : 0; }
extern "C" int qoimi_set_encode_small_call_order(qoimi_ctx* c, int by_workgroup_index) {
    if (!c) return fail(QOIMI_E_ARG, "ctx is NULL");
    c->enc_tree_ticket = by_workgroup_index ? 0 : 1;
    return QOIMI_OK;
}

// device memory the context holds: [0] encode workspace (and the staging of qoimi_encode_packed), [1] decode workspace (and the tables of
// qoimi_inspect_streams, the tables and the staging of qoimi_compare_images / qoimi_verify_images / qoimi_decode_thumbnails / qoimi_decode_crops / qoimi_decode_resized), [2] staging of the
// host-pointer entry points
extern "C" void qoimi_workspace_bytes(qoimi_ctx* c, size_t out[3]) {
    out[0] = c ? c->enc_ws.cap + c->enc_stage.cap : 0; out[1] = c ? c->dec_ws.cap + c->insp_ws.cap + c->cmp_ws.cap + c->ver_stage.cap : 0;
    out[2] = c ? c->io_a.cap + c->io_b.cap + c->io_c.cap : 0;
}

extern "C" void qoimi_decode_stats(qoimi_ctx* c, long long out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = c ? c->dec_stats[i] : 0;
}

// ------------------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------------------
extern "C" int qoimi_encode_batch(qoimi_ctx* c, const void* d_pixels, size_t pixel_stride,
                                  const qoi_desc* desc, int n_images,
                                  void* d_streams, size_t stream_stride, int* d_stream_len,
                                  void* stream) {
    if (!c || !d_pixels || !d_streams || !d_stream_len || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (!desc_ok(desc)) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:364-372 rules)");
    const size_t npx = (size_t)desc->width * desc->height;
    if (pixel_stride < npx * desc->channels) return fail(QOIMI_E_ARG, "pixel_stride smaller than one image");
    if (stream_stride < qoimi_encode_bound(desc)) return fail(QOIMI_E_ARG, "stream_stride smaller than qoimi_encode_bound");
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;

    EncParams p;
    memset(&p, 0, sizeof p);
    p.pixels = (const uint8_t*)d_pixels; p.pixel_stride = pixel_stride;
    p.npx = (uint32_t)npx; p.n_images = (uint32_t)n_images;
    p.spi = (uint32_t)((npx + kEncSlabPx - 1) / kEncSlabPx);
    p.gpi = (p.spi + 63u) / 64u;
    p.width = desc->width; p.height = desc->height; p.channels = desc->channels; p.colorspace = desc->colorspace;
    // The ordered-exchange probe rests on a measured hardware property (qoi_encode.hip): measure it again as the context
    // lives on.  The repeat runs on the context's private stream; its result is looked at by the next call.
    if (c->recheck_pending && hipStreamQuery(c->own_stream) == hipSuccess) {
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
            (void)fail(QOIMI_E_INTERNAL, "the LDS exchange-order self-test failed on repetition: streams encoded since the last passed check are suspect (qoimi_encode_suspect_calls); this context now uses the order-free probe");
        } else {
            c->enc_calls_last_passed = c->enc_calls_at_check;
        }
    }
    ++c->enc_calls;
    if (c->xchg_ordered && !c->recheck_pending && c->enc_calls - c->enc_calls_at_check >= c->enc_recheck_every && c->io_c.reserve(256) == QOIMI_OK) {
        c->enc_calls_at_check = c->enc_calls;
        uint32_t* d_flag = (uint32_t*)c->io_c.base + 32;
        launch_lds_order_selftest(d_flag, c->own_stream);
        if (hipMemcpyAsync(&c->host_word[8], d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->own_stream) == hipSuccess) c->recheck_pending = true;
    }
    p.probe_xchg = c->xchg_ordered ? 1 : 0;
    p.use_ticket = c->enc_ticket ? 1 : 0;
    p.warm = c->enc_warm ? 1 : 0;
    p.persist = (uint32_t)c->enc_persist;
    bool all_flagged_before = false;
    p.pipe = (uint32_t)c->enc_pipe;
    p.spread = (uint32_t)c->enc_spread;
    // Slabs per set and placement - functions of the call's shape only; QOIMI_ENC_SET_SLABS / QOIMI_ENC_LOOKBACK force them; every
    // combination gives the same bytes.
    // A wavefront carries the colour table and its staged bytes from slab to slab, so the entry-state replay and the placement are
    // paid once per set - as long as the sets still fill the 256 CUs x 24 wavefronts several times.
    // Look-back (1): a set finds its place in the stream by decoupled look-back over the earlier sets of its image and writes its
    // bytes once, straight from the LDS (sets of more than ~1.4 bytes per pixel spill to a scratch slot and move that part
    // themselves).  The inclusive prefixes travel 64 sets per poll (~1 us) through the sets of an image that finish at about the same
    // time - the ~6000 resident wavefronts divided by the number of images.  With a batch that is a few sets; with ONE image it is
    // all of them (a 4K frame: 71-131 us against 45 order-free), and its ticket counter serves every wavefront in turn.
    // Tree (2, round 4; encode_set): calls of fewer than 8 images.  Every set adds three windows of byte counts - its group's, its
    // block's group totals, the image's block totals - nothing travels from set to set, the sets go by workgroup index.  One frame,
    // tree against the best of the other two forms (profiles/r04_s12_single_placement.txt): 640 x 360 20.2 us / 22.8, 1280 x 720
    // 21.9 / 26.8, 1920 x 1080 27.2 / 27.6, 2560 x 1440 32.0 / 31.4, 3840 x 2160 39.9 / 42.6, 5120 x 2880 50.3 / 57.0.
    // Order-free (0): every set parks its bytes in a scratch slot, enc_offsets scans the sizes with a whole workgroup, enc_compact
    // places them (two more launches, a round trip through scratch).  No set ever waits: what very large images take (16384 x
    // 16384: 552 us against 653 by the tree - 6000 sets in flight, each a few microseconds in its slot waiting for the totals).
    {
        const size_t total_slabs = (size_t)n_images * p.spi;
        uint32_t r = total_slabs >= 3u * 65536u ? 3u : (total_slabs >= 16384u ? 2u : 1u);
        int place = c->enc_lookback >= 0 ? (c->enc_lookback > 2 ? 1 : c->enc_lookback) : (n_images >= 8 ? 1 : 2);
        if (place == 2 && c->enc_lookback < 0) {
            const uint32_t rt = total_slabs < 1500u ? 1u : (total_slabs < 6000u ? 2u : 3u);       // measured above
            if ((p.spi + rt - 1u) / rt > kEncTreeMaxSets) place = 0; else r = rt;
        }
        // Look-back batches: three slabs per set is the size for ~1.2 bytes per pixel - above ~1.4 a set outgrows its 6.3 KB staging
        // buffer and sends what it has through a scratch slot (a second trip through memory for those bytes).  Two slabs stay staged
        // up to 3 bytes per pixel (photo_hard, 2.1 B/px, 128 frames: 3.00 ms at three slabs, 2.77 at two, 3.86 at one;
        // photographs of 1.2 B/px lose 10 % at two).  What the content looks like is taken from the previous batch call of the context:
        // the length of its first stream, copied to a pinned word behind that call (read here without a wait: a stale or missing
        // value only picks the other set size, the streams are the same bytes either way).
        // (round 6: only when the TWO batches before this one were both that heavy.  Photographs behind a batch of 2.1 B/px lost 23 % to the
        // two-slab sets their predecessor had earned, bench.py "alternating", profiles/r06_s8; a workload that alternates now never takes a
        // hint, one that stays with its content takes it from its third batch on)
        if (c->enc_adapt && place == 1 && n_images >= 8) {
            const bool heavy = c->enc_hint_npx != 0u && c->host_word[12] != 0u && (double)c->host_word[12] > 1.4 * (double)c->enc_hint_npx;
            if (r == 3u && heavy && c->enc_heavy_before) r = 2u;
            c->enc_heavy_before = heavy;
        }
        if (c->enc_set_slabs > 0) r = (uint32_t)c->enc_set_slabs;
        if (r > kEncMaxSetSlabs) r = kEncMaxSetSlabs;
        p.set_slabs = r;
        p.set_px = r * kEncSlabPx;
        p.sets_per_image = (p.spi + r - 1u) / r;
        p.set_stride = r * kEncSlabWorst + 16u;
        if (place == 2 && p.sets_per_image > 64u * 64u * 64u) place = 0;            // (three levels of 64; the generic pass has fewer sets)
        p.lookback = (uint8_t)place;
        // Tree: units by workgroup index (a wait is for lower-numbered sets, which the dispatcher started earlier - true of one launch
        // on an idle device; two launches from different streams could in principle hold each other's predecessors out: the waits are
        // bounded - 2^15 polls, tens of milliseconds, where a set's predecessors finish within microseconds - a tripped bound ends every
        // wait of the launch and the call is encoded again order-free by qoi_encode / qoimi_encode_status).  That form is what the
        // drop-in qoi_encode takes (it reads the error word and encodes again by itself).  qoimi_encode_batch (round 6: the default)
        // hands the units out by one ticket per workgroup - START order, no assumption about the dispatcher, so a caller that only
        // synchronises its stream never reads a truncated stream - 4 us more per 4K frame (46.8 against 42.6 us, 720p 23.8 against
        // 21.5: profiles/r05_s1_single_ticket.txt).
        if (place == 2) { p.spread = 0; p.use_ticket = (c->enc_tree_ticket >= 0 ? c->enc_tree_ticket != 0 : !c->dropin) ? 1 : 0; }
    }
    const int place = p.lookback;
    const bool lookback = place != 0;
    p.spin_bound = (place == 2 && !p.use_ticket) ? (1u << 15) : (1u << 22);
    if (c->test_spin_bound) p.spin_bound = c->test_spin_bound;            // tests: make a wait give up
    const size_t T = (size_t)p.n_images * p.spi, G = (size_t)p.n_images * p.gpi, S = (size_t)p.n_images * p.sets_per_image;
    if (T > 0xFFFFFFF0ull) return fail(QOIMI_E_ARG, "batch too large (slab index overflows 32 bits)");
    // Scratch.  Order-free: every set parks its bytes in a slot of its own until the placement passes run (few large images:
    // tens of megabytes).  Look-back: only sets that outgrow their LDS staging buffer (more than ~1.5 bytes per pixel) hold scratch,
    // from their first spill to their copy-out - a pool of kEncPoolSlots slots (more than the wavefronts in flight; fewer for calls
    // of fewer sets), handed out on the device (pool_take).  The 1024-frame 4K shard: 0.67 GB (slots of sixteen slabs) instead of 42.5 GB.
    p.pool = lookback ? 1 : 0;
    p.gen_slabs = c->enc_gen_slabs > 0 ? (uint32_t)c->enc_gen_slabs : ((size_t)n_images * p.spi >= 3u * 65536u ? 2u * kEncGenSetSlabs : kEncGenSetSlabs);
    p.gen_grid_div = (c->enc_adapt && n_images >= 8 && c->host_word[13] != 0u) ? (uint32_t)c->enc_gen_grid_div : 0u;
    p.gen_small_div = (uint32_t)c->enc_gen_small_div;
    // The previous batch held flagged images ONLY (flat content: host_word[13] counts them): this call's first pass will most likely find
    // an image's first flat stretch within microseconds and every other set of the image has nothing to do but to see the flag - one
    // workgroup per four sets is 345 000 workgroups that start and end for 512 4K frames, 0.5 ms of dispatch.  A sixteenth of them, each
    // looking at sixteen units, sees the same flags (photographs pay 7-9 % with several sets per wavefront: the hint is gone after one call).
    if (c->enc_adapt && place == 1 && n_images >= 8) {
        const bool flagged = c->enc_hint_images != 0u && c->host_word[13] >= c->enc_hint_images;
        all_flagged_before = flagged && c->enc_flagged_before;                  // (two batches in a row, as the set size above)
        c->enc_flagged_before = flagged;
    }
    if (all_flagged_before && p.persist == 0u) p.persist = 0xFFFFFFFFu;            // resolved below, once the units are known
    // ... or not at all (QOIMI_ENC_ALL_G2, default on): the pass over flagged images takes EVERY image of this call, and counts the images in
    // which some set had to walk the groups in front of its tail - the same statistic, so a batch of photographs behind flat batches
    // runs once through that pass (sixteen-slab sets, every set through the pool) and hands the next batch back to the two passes.
    p.all_g2 = (all_flagged_before && c->enc_all_g2) ? 1u : 0u;
    const size_t S_gen = (size_t)p.n_images * ((p.spi + p.gen_slabs - 1u) / p.gen_slabs);
    if (lookback) {
        size_t slots = (S + 63u) & ~(size_t)63u;
        p.pool_slots = (uint32_t)(slots < kEncPoolSlots ? slots : kEncPoolSlots);
        const uint32_t r_max = p.set_slabs > p.gen_slabs ? p.set_slabs : p.gen_slabs;     // the generic pass draws on the same pool
        p.set_stride = r_max * kEncSlabWorst + 16u;
    }

    size_t g2_bytes = 0;
    // calls of a few images: two regions of records / tickets / flags / pool map, used in turn - the first launch of a call zeroes the region
    // of the next (enc_sets: zero_next), which then skips its hipMemsetAsync if it is the very next user of the workspace and lays out alike
    const long long ws_seq = ++c->enc_ws_seq;
    const auto zeroed_before = c->prezero;
    c->prezero.valid = false;
    const bool pingpong = place == 2 && c->enc_prezero && p.warm && p.probe_xchg;
    uint8_t* zero_other = nullptr; size_t zero_len = 0;
    // one of the last eight small calls the DEVICE has started met flat stretches (host_word[14]: number of the last call that did,
    // [15]: of the last call started; the calls of a pipeline are set up long before their predecessors run - read once: the device may be writing)
    const uint32_t hint = *(volatile uint32_t*)&c->host_word[14], started = *(volatile uint32_t*)&c->host_word[15];
    const bool hot = hint != 0u && (((started - hint) & 0x1FFFFFFFu) < 8u || ((hint - started) & 0x1FFFFFFFu) < 8u);
    for (int pass = 0; pass < 2; ++pass) {      // pass 0 measures, pass 1 carves
        Carver w(pass ? c->enc_ws.base : nullptr);
        p.status = w.take<u64>(S); p.ticket = w.take<uint32_t>((size_t)n_images); p.err = w.take<uint32_t>(1);
        p.need_generic = w.take<uint32_t>((size_t)n_images); p.any_generic = w.take<uint32_t>(1);
        p.status_gen = w.take<u64>(lookback ? S_gen : 0); p.ticket_gen = w.take<uint32_t>(lookback ? (size_t)n_images : 0);
        {   // tree placement: totals of the groups of 64 sets and of the blocks of 64 groups, for the first pass and for the generic one
            const size_t n1 = (p.sets_per_image + 63u) / 64u, n2 = (n1 + 63u) / 64u;
            const size_t sg1 = (S_gen / (size_t)n_images + 63u) / 64u, sg2 = (sg1 + 63u) / 64u;
            const size_t on = place == 2 ? (size_t)n_images : 0;
            p.tree1 = w.take<u64>(on * n1); p.tree2 = w.take<u64>(on * n2);
            p.tree1_gen = w.take<u64>(on * sg1); p.tree2_gen = w.take<u64>(on * sg2);
        }
        p.pool_map = w.take<u64>(lookback ? (size_t)(p.pool_slots / 64u) * kEncPoolMapStride : 0);
        const size_t zero_bytes = w.off;
        // flagged images (flat content): by state look-back over their sets (ENTRY 2: 520 bytes per set of eight slabs, tagged with the
        // call's number instead of being zeroed) - or, for order-free calls and the order-independent probe, by the summary passes
        // (per slab 2 x (256 B table + 8 B valid + 4 B position): 4.3 GB for the 1024-frame 4K shard)
        const bool g2 = lookback && p.probe_xchg && p.warm && c->enc_g2;
        // One pass or two: a frame of photographic content is 2 us faster through the two-pass kernel, which never needs its second pass
        // (35.3 against 37.1 us per 4K frame); a frame with flat stretches saves the second launch and the first pass's wasted walk with
        // the one-pass kernel (4K: constant 110 -> 93 us, UI 156 -> 111, soft-alpha sprite 126 -> 69; profiles/r05_s16_single_uni.txt).
        // Calls of a few images take the one pass when one of the last eight such calls the device has started met a flat stretch: its first
        // such set left the call's number in a pinned word (leave_hint).  Batches keep two passes (1024 photographs 13.4 against 12.3 ms in one pass).
        p.uni = (g2 && (c->enc_uni > 0 || (c->enc_uni < 0 && c->enc_adapt && place == 2 && hot))) ? 1u : 0u;
        p.host_hint = place == 2 ? &c->host_word[14] : nullptr;
        const size_t g2_sets = p.uni ? S : S_gen;              // (one pass: a record per set of that pass)
        p.g2_rec = w.take<u64>(g2 ? g2_sets * 65u : 0);
        g2_bytes = g2 ? g2_sets * 65u * sizeof(u64) : 0;
        if (!g2) p.g2_rec = nullptr;
        const size_t Tt = g2 ? 0 : T, Gt = g2 ? 0 : G;
        p.sum_tab = w.take<uint32_t>(Tt * 64); p.sum_valid = w.take<u64>(Tt); p.sum_le = w.take<int>(Tt);
        p.ent_tab = w.take<uint32_t>(Tt * 64); p.ent_valid = w.take<u64>(Tt); p.ent_le = w.take<int>(Tt);
        p.grp_tab = w.take<uint32_t>(Gt * 64); p.grp_valid = w.take<u64>(Gt); p.grp_le = w.take<int>(Gt);
        p.gent_tab = w.take<uint32_t>(Gt * 64); p.gent_le = w.take<int>(Gt);
        p.set_size = w.take<uint32_t>(lookback ? 0 : S); p.set_off = w.take<uint32_t>(lookback ? 0 : S);
        p.scratch = w.take<uint8_t>(lookback ? ((size_t)p.pool_slots + 1u) * p.set_stride : S * p.set_stride);
        uint8_t* const alt = w.take<uint8_t>(pingpong ? zero_bytes : 0);          // the second region (256-byte aligned like the first)
        if (!pass) { int rc = c->enc_ws.reserve(w.off + 256); if (rc) return rc; }
        else {
            uint8_t* mine = (uint8_t*)c->enc_ws.base;
            if (pingpong) {
                zero_other = alt; zero_len = zero_bytes;
                if (c->enc_parity) {                       // this call's turn on the second region: everything carved from the first moves over
                    const ptrdiff_t d = alt - mine;
                    auto over = [d](auto*& q) { q = reinterpret_cast<std::remove_reference_t<decltype(q)>>(reinterpret_cast<uint8_t*>(q) + d); };
                    over(p.status); over(p.ticket); over(p.err); over(p.need_generic); over(p.any_generic); over(p.status_gen); over(p.ticket_gen);
                    over(p.tree1); over(p.tree2); over(p.tree1_gen); over(p.tree2_gen); over(p.pool_map);
                    zero_other = mine; mine = alt;
                }
                c->enc_parity ^= 1;
                p.zero_next = reinterpret_cast<uint32_t*>(zero_other); p.zero_next_dwords = (uint32_t)(zero_bytes / 4u);
            }
            const bool zeroed = pingpong && zeroed_before.valid && zeroed_before.seq + 1 == ws_seq && zeroed_before.ptr == (void*)mine &&
                                zeroed_before.bytes == zero_bytes && zeroed_before.gen == c->enc_ws.gen;
            if (!zeroed) HIP_TRY(hipMemsetAsync(mine, 0, zero_bytes, st));   // look-back records, tickets, flags, pool map
            // the state look-back's granules are told apart by the call's number; zeroed only when they come to lie somewhere new
            // (another arena, another shape of call) or the number wraps
            c->enc_epoch = (c->enc_epoch + 1u) & 0x1FFFFFFFu;
            if (g2_bytes && (c->g2_zeroed_at != (void*)p.g2_rec || c->g2_zeroed_bytes != g2_bytes || c->g2_zeroed_gen != c->enc_ws.gen || c->enc_epoch == 0u)) {
                HIP_TRY(hipMemsetAsync(p.g2_rec, 0, g2_bytes, st));
                c->g2_zeroed_at = (void*)p.g2_rec; c->g2_zeroed_bytes = g2_bytes; c->g2_zeroed_gen = c->enc_ws.gen;
                if (c->enc_epoch == 0u) c->enc_epoch = 1u;
            }
            p.epoch = c->enc_epoch;
        }
    }
    // (a call that lays the workspace out WITHOUT state granules writes scratch, tables or summaries where an earlier call's granules lay:
    // the next call with granules must zero them again, whatever it finds at the same address)
    if (!g2_bytes) c->g2_zeroed_at = nullptr;
    p.out = (uint8_t*)d_streams; p.out_stride = stream_stride; p.out_len = d_stream_len;
    c->last_enc_err = p.err; c->last_enc_err2 = nullptr;
    if (c->timer.n > KernelTimer::kMax - 32) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
    // (Running the placement passes of one sub-batch on a second stream beside the slab passes of the next was tried in round
    // 2: 4.996 vs 4.986 ms per 256 4K frames - the two kernels time-slice the CUs, nothing overlaps.)
    c->timer.mark(kT_begin, st);
    launch_encode(p, st, &c->timer);
    c->timer.mark(kT_enc_total, st);
    if (pingpong && zero_other) { c->prezero.ptr = zero_other; c->prezero.bytes = zero_len; c->prezero.gen = c->enc_ws.gen; c->prezero.seq = ws_seq; c->prezero.valid = true; }
    if (c->enc_adapt && place == 1) {                       // what this batch's streams look like, for the next call's set size (see above)
        if (hipMemcpyAsync(&c->host_word[12], d_stream_len, sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess) c->enc_hint_npx = p.npx;
        if (hipMemcpyAsync(&c->host_word[13], p.any_generic, sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess) c->enc_hint_images = (uint32_t)n_images;    // ... and how many flagged (flat) images it held: the grids of the next call's passes
    }
    c->last_enc.px = d_pixels; c->last_enc.ps = pixel_stride; c->last_enc.desc = *desc; c->last_enc.n = n_images;
    c->last_enc.out = d_streams; c->last_enc.os = stream_stride; c->last_enc.len = d_stream_len; c->last_enc.st = stream; c->last_enc.valid = true;
    if (const char* dump = c->enc_debug_dump.empty() ? nullptr : c->enc_debug_dump.c_str()) {          // diagnostics: the entry-state arrays of this call, raw
        (void)hipStreamSynchronize(st);
        if (FILE* fo = fopen(dump, "wb")) {
            auto put = [&](const void* d, size_t bytes) { std::vector<uint8_t> h(bytes); (void)hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost); fwrite(h.data(), 1, bytes, fo); };
            const uint64_t hdr[4] = {T, G, (uint64_t)p.spi, (uint64_t)p.gpi};
            fwrite(hdr, 8, 4, fo);
            put(p.sum_tab, T * 256); put(p.sum_valid, T * 8); put(p.ent_tab, T * 256); put(p.ent_valid, T * 8);
            put(p.grp_tab, G * 256); put(p.grp_valid, G * 8); put(p.gent_tab, G * 256);
            fclose(fo);
        }
    }
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

// Differently shaped images in one call (qoibench.c:491-555 walks a directory): per-image descriptors and offsets.  The images are
// grouped by channel count (the kernels are compiled per count) and every group is placed order-free - each set parks its bytes in a
// scratch slot of its own, enc_offsets + enc_compact move them - so no set waits for another and any mix of sizes will do.
extern "C" int qoimi_encode_images(qoimi_ctx* c, const void* d_pixels, const size_t* pixel_offsets, const qoi_desc* descs, int n_images,
                                   void* d_streams, const size_t* stream_offsets, int* d_stream_len, void* stream) {
    if (!c || !d_pixels || !pixel_offsets || !descs || !d_streams || !stream_offsets || !d_stream_len || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    for (int i = 0; i < n_images; ++i) if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:364-372 rules)");
    DeviceGuard guard(c->device);
    ++c->enc_ws_seq; c->prezero.valid = false;               // (the encode workspace is laid out anew below: nothing a batch call zeroed ahead survives)
    c->g2_zeroed_at = nullptr;                               // ... nor the state granules of an earlier batch call
    hipStream_t st = (hipStream_t)stream;
    if (c->recheck_pending && hipStreamQuery(c->own_stream) == hipSuccess) {                  // (the repeat of the LDS-order self-test: see qoimi_encode_batch)
        c->recheck_pending = false;
        if (c->host_word[8] != 0u || c->test_force_recheck_fail) {
            c->xchg_ordered = false;
            c->enc_suspect_calls += c->enc_calls - c->enc_calls_last_passed;
            c->enc_calls_last_passed = c->enc_calls;
            c->recheck_failed_unreported = true;
        } else c->enc_calls_last_passed = c->enc_calls_at_check;
    }
    ++c->enc_calls;
    c->last_enc.valid = false;
    c->last_enc_err = nullptr; c->last_enc_err2 = nullptr;
    // the table of a channel group travels through pinned staging; both groups' tables and workspaces live side by side in the
    // arena (the second group's launches follow the first's on the stream and must not overwrite what those still read)
    size_t ws_off = 0;
    for (int pass = 0; pass < 2; ++pass) {               // pass 0 measures the arena (both groups), pass 1 carves and launches
        ws_off = 0;
        size_t pin_off = 0;
        for (uint32_t ch = 3; ch <= 4; ++ch) {
            std::vector<EncImage> tab;
            std::vector<int> who;
            uint64_t slabs = 0, groups = 0, units = 0;
            for (int i = 0; i < n_images; ++i) {
                if (descs[i].channels != ch) continue;
                EncImage e; memset(&e, 0, sizeof e);
                e.pixel_off = pixel_offsets[i]; e.out_off = stream_offsets[i];
                e.npx = descs[i].width * descs[i].height;
                e.spi = (e.npx + kEncSlabPx - 1u) / kEncSlabPx; e.gpi = (e.spi + 63u) / 64u;
                e.width = descs[i].width; e.height = descs[i].height; e.colorspace = descs[i].colorspace;
                e.slab_base = (uint32_t)slabs; e.grp_base = (uint32_t)groups;
                slabs += e.spi; groups += e.gpi;
                e.len_index = (uint32_t)i;
                tab.push_back(e); who.push_back(i);
            }
            if (tab.empty()) continue;
            if (slabs > 0xFFFFFFF0ull) return fail(QOIMI_E_ARG, "batch too large (slab index overflows 32 bits)");
            const uint32_t n = (uint32_t)tab.size();
            const uint32_t r = c->enc_set_slabs > 0 ? (uint32_t)(c->enc_set_slabs > (int)kEncMaxSetSlabs ? kEncMaxSetSlabs : c->enc_set_slabs)
                                                     : (slabs >= 3u * 65536u ? 3u : (slabs >= 16384u ? 2u : 1u));
            uint64_t sets = 0;
            for (EncImage& e : tab) { e.sets = (e.spi + r - 1u) / r; e.set_base = (uint32_t)sets; e.unit_base = (uint32_t)units; sets += e.sets; units += (e.sets + 3u) / 4u; }
            EncImage tail; memset(&tail, 0, sizeof tail);
            tail.set_base = (uint32_t)sets; tail.slab_base = (uint32_t)slabs; tail.grp_base = (uint32_t)groups; tail.unit_base = (uint32_t)units;
            tab.push_back(tail);
            EncParams p; memset(&p, 0, sizeof p);
            p.pixels = (const uint8_t*)d_pixels; p.out = (uint8_t*)d_streams; p.n_images = n; p.channels = (uint8_t)ch;
            p.set_slabs = r; p.set_px = r * kEncSlabPx; p.set_stride = r * kEncSlabWorst + 16u;
            p.probe_xchg = c->xchg_ordered ? 1 : 0; p.use_ticket = 0; p.warm = c->enc_warm ? 1 : 0; p.lookback = 0; p.pool = 0; p.spin_bound = 1u << 22; p.gen_slabs = kEncGenSetSlabs;
            const size_t T = (size_t)slabs, G = (size_t)groups, S = (size_t)sets;
            Carver w(pass ? (uint8_t*)c->enc_ws.base + ws_off : nullptr);
            if (!pass) w.base = nullptr;
            p.status = w.take<u64>(0); p.ticket = w.take<uint32_t>(n); p.err = w.take<uint32_t>(1);
            p.need_generic = w.take<uint32_t>(n); p.any_generic = w.take<uint32_t>(1);
            const size_t zero_bytes = w.off;
            EncImage* d_tab = w.take<EncImage>(tab.size());
            p.sum_tab = w.take<uint32_t>(T * 64); p.sum_valid = w.take<u64>(T); p.sum_le = w.take<int>(T);
            p.ent_tab = w.take<uint32_t>(T * 64); p.ent_valid = w.take<u64>(T); p.ent_le = w.take<int>(T);
            p.grp_tab = w.take<uint32_t>(G * 64); p.grp_valid = w.take<u64>(G); p.grp_le = w.take<int>(G);
            p.gent_tab = w.take<uint32_t>(G * 64); p.gent_le = w.take<int>(G);
            p.set_size = w.take<uint32_t>(S); p.set_off = w.take<uint32_t>(S);
            p.scratch = w.take<uint8_t>(S * p.set_stride);
            const size_t used = (w.off + 255u) & ~(size_t)255u;
            if (pass) {
                const size_t tbytes = tab.size() * sizeof(EncImage);
                if (hipMemsetAsync((uint8_t*)c->enc_ws.base + ws_off, 0, zero_bytes, st) != hipSuccess) return fail(QOIMI_E_INTERNAL, "hipMemsetAsync failed");
                memcpy((uint8_t*)c->enc_pin_buf + pin_off, tab.data(), tbytes);
                HIP_TRY(hipMemcpyAsync(d_tab, (uint8_t*)c->enc_pin_buf + pin_off, tbytes, hipMemcpyHostToDevice, st));
                HIP_TRY(hipEventRecord(c->enc_pin_ev, st));
                p.img_tab = d_tab; p.out_len = d_stream_len;           // (written at EncImage::len_index: the caller's image number)
                launch_encode_mixed(p, (uint32_t)units, (uint32_t)slabs, (uint32_t)groups, (uint32_t)sets, st, &c->timer);
                c->last_enc_err2 = c->last_enc_err; c->last_enc_err = p.err;       // (qoimi_encode_status looks at both channel groups)
            }
            ws_off += used;
            pin_off += (tab.size() * sizeof(EncImage) + 255u) & ~(size_t)255u;
        }
        if (!pass) {
            int rc = c->enc_ws.reserve(ws_off + 256); if (rc) return rc;
            // The staging of the previous call's tables may still be read by its copies - on whatever stream that call ran: wait for the
            // event recorded behind them (not for the stream: the call stays asynchronous) before the buffer is overwritten or freed.
            const size_t need = (size_t)(n_images + 2) * sizeof(EncImage) + 1024u;
            if (!c->enc_pin_ev) HIP_TRY(hipEventCreateWithFlags(&c->enc_pin_ev, hipEventDisableTiming));
            else HIP_TRY(hipEventSynchronize(c->enc_pin_ev));
            if (need > c->enc_pin_cap) {
                if (c->enc_pin_buf) (void)hipHostFree(c->enc_pin_buf);
                c->enc_pin_buf = nullptr; c->enc_pin_cap = 0;
                HIP_TRY(hipHostMalloc(&c->enc_pin_buf, need + 4096));
                c->enc_pin_cap = need + 4096;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

// Synchronise `stream` and report whether the last encode on this context tripped a
// device-side liveness bound (look-back spin limit).  Never expected; outputs of such a
// call must be discarded.
extern "C" int qoimi_encode_status(qoimi_ctx* c, void* stream) {
    if (!c) return fail(QOIMI_E_ARG, "ctx is NULL");
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (c->last_enc.valid && c->last_enc.st != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->last_enc.st));   // the stream the call was made on
    if (c->recheck_failed_unreported) {
        c->recheck_failed_unreported = false;
        return fail(QOIMI_E_INTERNAL, "the LDS exchange-order self-test failed on repetition: " + std::to_string(c->enc_suspect_calls) +
                    " earlier encode calls of this context are suspect (qoimi_encode_suspect_calls); the context now uses the order-free probe");
    }
    if (!c->last_enc_err) return QOIMI_OK;
    uint32_t err = 0, err2 = 0;
    HIP_TRY(hipMemcpy(&err, c->last_enc_err, sizeof err, hipMemcpyDeviceToHost));
    if (c->last_enc_err2) { HIP_TRY(hipMemcpy(&err2, c->last_enc_err2, sizeof err2, hipMemcpyDeviceToHost)); err |= err2; }
    if (err && c->last_enc.valid && c->enc_lookback != 0) {
        // A placement wait gave up (never observed: the sets a wait is for are resident or done unless another stream's launch holds
        // them out) or the scratch pool ran dry: the call is encoded again ORDER-FREE - no set waits for another, every set has a
        // scratch slot of its own - from the caller's buffers, which it has not read yet (it is asking for the status first), on the
        // stream the call was made on (the one this function waits for next, whatever `stream` is).
        const int forced = c->enc_lookback;
        c->enc_lookback = 0;
        c->last_enc.valid = false;
        const auto again = c->last_enc;
        const int rc = qoimi_encode_batch(c, again.px, again.ps, &again.desc, again.n, again.out, again.os, again.len, again.st);
        c->enc_lookback = forced;
        if (rc != QOIMI_OK) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)again.st));
        HIP_TRY(hipMemcpy(&err, c->last_enc_err, sizeof err, hipMemcpyDeviceToHost));
        c->enc_retries += 1;
    }
    if (err) return fail(QOIMI_E_INTERNAL, (err & 2u) ? "encode scratch pool exhausted" : "encode look-back exceeded its spin bound");
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------
// segment size of a decode call (see the cost model below)
static uint32_t choose_seg_bytes(const qoimi_ctx* c, const int* sizes, const qoi_desc* descs, int n_images, bool honour_forced = true) {
    uint32_t B = honour_forced ? c->seg_bytes : 0u;         // (QOIMI_SEG_BYTES)
    if (B == 0 && c->dec_run_desc && c->dec_flat_seg) {
        // A call of FLAT images only (run descriptors): a lane's walk over its segment no longer writes the segment's pixels, it costs
        // its chunks alone - larger segments mean fewer entry states (780 bytes per segment whatever its size), fewer chances to miss
        // (a round per miss) and the same work.  The largest size that still gives 128 K lanes (1024 UI frames, 292 MB of streams: 512 /
        // 1024 / 2048 bytes = 10 / 5 / 3 rounds in 22.0 / 18.9 / 19.1 ms, profiles/r05_s6_dec_span.txt; 4096: P3 and P4 run short of lanes).
        bool all_flat = true;
        uint64_t bytes = 0;
        for (int i = 0; i < n_images && all_flat; ++i) {
            all_flat = sizes[i] > 22 && descs[i].width != 0 && dec_image_is_flat((uint32_t)sizes[i] - 8u, (uint32_t)((uint64_t)descs[i].width * descs[i].height));
            bytes += (uint64_t)(sizes[i] > 0 ? sizes[i] : 0);
        }
        // (round 6: not below 512 bytes - 128 UI frames, 36 MB of streams, took 256 and with it rounds that re-open nearly everything: the
        // stall rule sent them to the sequential pass, 147 ms where 512-byte segments take 5.2, profiles/r06_s9_uiflat_mid_batch.txt; a call
        // with streams for a quarter of those lanes still takes 512, smaller ones the general model)
        if (all_flat) {
            for (uint32_t cand = 4096u; cand >= 512u; cand >>= 1)
                if (bytes / cand >= 131072u) { B = cand; break; }
            if (B == 0 && bytes / 512u >= 32768u) B = 512u;
        }
    }
    if (B == 0) {
        // One lane decodes one segment.  Two costs pull in opposite directions (constants measured on MI355X):
        //   * a lane walks its segment serially, ~0.6 us per chunk-step over the four passes, and the two
        //     table-bound passes hold ~98 K lanes at a time: t_walk ~ B/1.2 * 0.6 us * ceil(lanes / 98304)
        //   * the per-image chains (S1/S2/S3 level 2) walk the image's 64-segment groups, ~0.5 us per group over
        //     the three chains, 16 wavefronts per image in two sweeps plus a 16-step hand-over:
        //     t_chain ~ (groups / 8 + 16) * 0.5 us with groups = largest stream / B / 64
        // Small batches therefore get small segments (more lanes), a single large image not too small ones.
        // Large batches end at 4 KiB: the 520-byte symbolic summary and the two 260-byte entry states per segment are then an
        // eighth of the stream (256 x 4K photographs: decode 10.3 ms at 2 KiB, 9.9 at 4 KiB - P3 -10 %, S3 halved; at 8 KiB the
        // transcoder's 64 lanes read 512 KiB apart and lose 15 %).
        uint64_t bytes = 0, largest = 0;
        for (int i = 0; i < n_images; ++i) {
            const uint64_t sz = (uint64_t)(sizes[i] > 0 ? sizes[i] : 0);
            bytes += sz; if (sz > largest) largest = sz;
        }
        double best = 1e30;
        for (uint32_t cand = 128; cand <= 4096u; cand <<= 1) {
            const double lanes = (double)bytes / cand;
            const double rounds = lanes <= 98304.0 ? 1.0 : lanes / 98304.0;
            double t = (cand / 1.2) * 0.6 * rounds + ((double)largest / cand / 64.0 / 8.0 + 16.0) * 0.5;
            if (n_images > 4) {
                // Batches (round 6, fitted to 8 .. 256 4K frames of photographs and sprites at every size, profiles/r06_s31_batch_by_seg.txt):
                // the passes run at the chip's throughput, ~5 us per MB of streams, plus the per-segment state - (1 + 140 / B) - and end
                // with the longest lane's walk, which grows with the segment: ~0.3 us per byte (photographs 0.1, sprites with long runs
                // 0.65); a call behind one that needed repair rounds counts 1.3 (a round's passes serve few segments: each is as long as
                // one walk).  sqrt(bytes): 512 bytes for 8 photographs, 1 KiB for 32, 2 KiB for 128 .. 256, 4 KiB from ~3.6 GB of streams.
                // (The model above it ties all sizes once the chip is full and took the largest: 32 sprite frames 5.5 ms at 4 KiB, 3.9 at 1 KiB.)
                const double kappa = c->dec_nonflat_repair ? 1.3 : 0.3;
                t = (double)bytes * 5e-6 * (1.0 + 140.0 / cand) + kappa * cand + ((double)largest / cand / 64.0 / 8.0 + 16.0) * 0.5;
            }
            if (t < best) { best = t; B = cand; }
        }
        // Calls of a few images whose streams are small: the chip is not full at 128 bytes (a 1080p photograph: 20 K segments, 320
        // wavefronts for 1024 SIMDs), a pass is as long as one lane's walk - shorter segments, two transcoder lanes each, as long as
        // the call stays below ~48 K segments (1280 x 720: 111 -> 100 us at 64 bytes, 1080p 120 -> 114, 1440p 132 -> 128 at 96; a 4K
        // photograph keeps 128: 168 us at 112, profiles/r06_s22_single_small_seg.txt).  No piece parse below 128 bytes: a call whose
        // transcoder cannot synchronise every segment takes the full five-phase parse.
        if (B == 128u && n_images <= 4 && c->dec_fused && c->dec_fine && c->dec_split && c->dec_small_seg && !c->dec_few_syncfail) {
            const uint64_t want = (bytes / 49152u + 15u) / 16u * 16u;
            B = want < 64u ? 64u : want < 128u ? (uint32_t)want : 128u;
        }
        // A call that MIXES flat images with others (a directory of screenshots and photographs, bench.py "mixed_directory"): the flat
        // ones' streams are a few hundred KB - a few dozen lanes at the 4 KiB the photographs' bytes ask for - and the symbolic pass walks
        // them several times (refinement passes): 4.8 of that leg's 9.3 ms.  Not above 1 KiB then (photographs lose a few per cent, 4 x
        // the lanes for the flat images' passes).
        if (B > 1024u && c->dec_run_desc)
            for (int i = 0; i < n_images; ++i)
                if (sizes[i] > 22 && descs[i].width != 0 && dec_image_is_flat((uint32_t)sizes[i] - 8u, (uint32_t)((uint64_t)descs[i].width * descs[i].height))) { B = 1024u; break; }
    }
    return B;
}

// one sub-batch: everything of qoimi_decode_batch for images whose record arena fits dec_rec_cap
static int decode_some(qoimi_ctx* c, const void* d_streams, const size_t* stream_offs, size_t stream_limit,
                       const int* sizes, const qoi_desc* descs, int n_images, int channels,
                       void* d_pixels, const size_t* pixel_offs, size_t pixel_limit, void* stream, uint32_t B, long long stats[4]) {
    // image i of this sub-call: its stream at d_streams + stream_offs[i], its pixels at d_pixels + pixel_offs[i]; stream_limit / pixel_limit: the
    // strides of qoimi_decode_batch, which no stream / image may exceed (qoimi_decode_images: no limit); all arrays are the sub-call's own
    int och = 0;
    std::vector<DecImage> imgs((size_t)n_images);
    uint64_t total = 0, total_g = 0, flat_total = 0;
    // Calls of a few images take the single-pass look-back kernel for pixel offsets and speculated slots (dec_scan_entry: one launch
    // where the three-level chains take ten); every image then begins on a multiple of kScanSegs segments.  Needs dec_transcode<0> (the
    // 128-byte piece parse's segment sizes) and falls back to the chains by itself where that pass cannot synchronise every segment.
    // (segments below 128 bytes, any multiple of 16 from 64 on: two transcoder lanes per segment; no piece parse for those - a call whose
    // transcoder cannot synchronise every segment takes the full five-phase parse)
    const bool small_seg = B >= 64u && B < 128u && B % 16u == 0u && c->dec_split;
    // (the context's previous call of a few images could not synchronise every segment - sprites with many alpha levels, noise - and paid for the
    // attempt: a wait, the parse, everything again through the chains.  The next such call takes the chains at once - and run descriptors for
    // long runs, a launch more on a path that no longer counts them; a call that synchronises everything switches back.  A lone 4K sprite
    // frame: 587 -> 404 us, profiles/r06_s34_single_kinds.txt; since the second sync run-up of dec_transcode<0> only streams built against the synchronisation get here)
    const bool skip_fused = n_images <= 4 && c->dec_few_syncfail && c->dec_fused_adapt;
    const bool fused_layout = c->dec_fused && !skip_fused && n_images <= 4 && c->dec_fine &&
                              (small_seg || (B % 128u == 0u && B / 128u >= 1u && B / 128u <= 64u && ((B / 128u) & (B / 128u - 1u)) == 0u));
    for (int i = 0; i < n_images; ++i) {
        if (sizes[i] < kHeaderBytes + kTrailerBytes) return fail(QOIMI_E_ARG, "stream shorter than 22 bytes (qoi.h:500)");
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:513-521 rules)");
        const int o = channels ? channels : descs[i].channels;
        if (och && o != och) return fail(QOIMI_E_ARG, "all images of a batch must share the output channel count");
        och = o;
        const size_t npx = (size_t)descs[i].width * descs[i].height;
        if (npx * (size_t)o > pixel_limit) return fail(QOIMI_E_ARG, "pixel_stride smaller than a decoded image");
        if ((size_t)sizes[i] > stream_limit) return fail(QOIMI_E_ARG, "stream longer than stream_stride");
        DecImage& im = imgs[(size_t)i];
        memset(&im, 0, sizeof im);
        im.stream_off = stream_offs[i];
        im.pixel_off = pixel_offs[i];
        im.chunks_end = (uint32_t)(sizes[i] - kTrailerBytes);
        im.npx = (uint32_t)npx;
        if (fused_layout) { total = (total + kScanSegs - 1u) / kScanSegs * kScanSegs; total_g = total / 64u; }
        im.seg_base = (uint32_t)total;
        im.nseg = (im.chunks_end - kHeaderBytes + B - 1u) / B;
        im.grp_base = (uint32_t)total_g;
        im.ngrp = (im.nseg + 63u) / 64u;
        im.desc_base = kNoRunDesc;
        if (c->dec_run_desc && im.nseg != 0u && dec_image_is_flat(im.chunks_end, im.npx)) { im.desc_base = (uint32_t)flat_total; flat_total += im.nseg; }
        total += im.nseg;
        total_g += im.ngrp;
    }
    if (fused_layout) { total = (total + kScanSegs - 1u) / kScanSegs * kScanSegs; total_g = total / 64u; }
    if (total > 0xFFFFFFF0ull) return fail(QOIMI_E_ARG, "batch too large (segment index overflows 32 bits)");
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    // The previous call of this context may have returned on its pinned result words while its dec_fill was still retiring (it zeroes the
    // counter header last).  On the same stream this call's work is ordered behind it; a caller that changes streams gets the wait here.
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    c->dec_tail_open = false;

    DecParams p;
    memset(&p, 0, sizeof p);
    bool fused = fused_layout && total != 0;
    p.streams = (const uint8_t*)d_streams; p.n_images = (uint32_t)n_images;
    p.total_segs = (uint32_t)total; p.total_grps = (uint32_t)total_g; p.seg_bytes = B;
    p.rec_rows = rec_rows_of(B);
    if (fused && B <= (uint32_t)c->dec_split_max && c->dec_split) {          // two transcoder lanes per segment (dec_transcode<0, .., SPLIT>): rows for two halves
        p.tr_split = 1u; p.tr_rows_half = rec_rows_of(B / 2u); p.rec_rows = 2u * p.tr_rows_half;
        p.tr_scan = c->dec_tr_scan ? 1u : 0u;
    }
    p.flat_segs = (uint32_t)flat_total;
    p.desc_cap = (p.tr_split ? 2u * rec_max_records(B / 2u) : rec_max_records(B)) / 2u + 2u;              // a run ends with the record behind it: every second record at most
    // descriptors for the long runs of the other images as well - not for calls of a few images without a flat one (one more launch
    // on a path that counts them)
    // (... nor for a call of a few images unless the context's previous one met long runs by the thousand - a sprite's transparent bands: its P4 is
    // then as long as the lane that writes a band 16 bytes at a time, 257 us for a 4K frame against 112 with descriptors)
    p.desc_all = (c->dec_run_desc >= 2 && (n_images > 4 || flat_total != 0 || skip_fused || c->dec_few_longruns)) ? 1u : 0u;
    p.sync_all = 0;
    p.p3_plain = (uint32_t)c->dec_p3_plain;
    p.refine_inner = (uint32_t)c->dec_inner;
    {   // extra first-round passes only if the call holds a flat image at all
        bool any_flat = false;
        for (int i = 0; i < n_images && !any_flat; ++i) any_flat = sizes[i] > 22 && dec_image_is_flat((uint32_t)sizes[i] - 8u, descs[i].width * descs[i].height);
        p.first_inner = any_flat ? (uint32_t)c->dec_inner1 : 0u;
    }
    p.pixels = (uint8_t*)d_pixels;
    const size_t Q = total + 1;   // +1: check of segment q reads entry[q+1]
    {   // P1/P2 on 128-byte pieces when a segment is 1, 2, 4 ... 64 of them
        const uint32_t g = B / 128u;
        const bool ok = B % 128u == 0u && g >= 1u && g <= 64u && (g & (g - 1u)) == 0u && c->dec_fine;
        p.fine_per_seg = ok ? g : 0u;
        p.fine_shift = 0;
        while (ok && (1u << p.fine_shift) < g) ++p.fine_shift;
        if ((uint64_t)total * (p.fine_per_seg ? p.fine_per_seg : 1u) > 0xFFFFFF00ull) return fail(QOIMI_E_ARG, "batch too large (piece index overflows 32 bits)");
        p.sync_all = p.fine_per_seg ? 0u : 1u;     // no piece parse for this segment size: full parse, then transcode from S1's phases
    }
    {   // a few large images: the per-image level of the state chain as several workgroups per image (dec_chain_state_l2m)
        uint64_t most = 0;
        for (const DecImage& im : imgs) most = im.ngrp > most ? im.ngrp : most;
        p.l2_wgs = (c->dec_l2_wgs && n_images <= 4 && (most >= 128u || c->dec_l2_wgs == 2)) ? 8u : 1u;                    // (4 images x 8 flags fit the counter header)
    }
    for (int pass = 0; pass < 2; ++pass) {
        Carver w(pass ? c->dec_ws.base : nullptr);
        p.pending = w.take<uint32_t>(4); p.redo_segs = p.pending ? p.pending + 1 : nullptr; p.sync_fails = p.pending ? p.pending + 2 : nullptr;
        p.run_queue_n = p.pending ? p.pending + 3 : nullptr;
        p.l2_ticket = p.pending ? p.pending + 8 : nullptr; p.l2_flag = p.pending ? p.pending + 16 : nullptr;       // words 8..11 and 16..47 of the zeroed 256-byte header
        p.conv = (p.pending && c->dec_conv) ? p.pending + 48 : nullptr;                                      // words 48..63: refinement passes that changed something (DecParams::conv)
        p.images = w.take<DecImage>((size_t)n_images);
        p.first_bad = w.take<uint32_t>((size_t)n_images);
        p.parse = w.take<ParseRec>(Q); p.entry_phase = w.take<uint8_t>(Q); p.px_off = w.take<uint32_t>(Q);
        p.slot_rec = w.take<SlotRec>(Q); p.slot_in = w.take<uint8_t>(Q); p.alpha_in = w.take<uint8_t>(Q);
        p.summary = w.take<u64>(Q * 65); p.entry = w.take<uint32_t>(Q * 65); p.fix = w.take<uint32_t>(Q * 65);
        const size_t NG = total_g + 1;
        p.grp_parse = w.take<ParseRec>(NG); p.grp_phase = w.take<uint8_t>(NG); p.grp_off = w.take<uint32_t>(NG);
        p.grp_slot = w.take<SlotRec>(NG); p.grp_slot_in = w.take<uint8_t>(NG); p.grp_alpha_in = w.take<uint8_t>(NG);
        p.grp_summary = w.take<u64>(NG * 65); p.grp_entry = w.take<uint32_t>(NG * 65);
        p.l2_sum = w.take<u64>((size_t)n_images * p.l2_wgs * 65);
        // calls of a few images: four wavefronts per group in the state chain (quarter summaries), prefixes instead of a chain of workgroups
        // at the per-image level
        const bool few = n_images <= 4 && c->dec_fused != 0;
        p.qtr_summary = w.take<u64>(few ? NG * 4u * 65u : 0);
        p.grp_prefix = w.take<u64>(few ? NG * 65u : 0); p.share_prefix = w.take<u64>(few ? (size_t)n_images * 8u * 16u * 65u : 0);
        if (few && p.l2_wgs < 8u) p.l2_sum = w.take<u64>((size_t)n_images * 8u * 65u);                  // (l2_sum above was sized for l2_wgs workgroups)
        p.s3_ctr = w.take<uint32_t>(few ? (size_t)n_images * 8u * 17u : 0); p.share_sum = w.take<u64>(few ? (size_t)n_images * 8u * 16u * 65u : 0);
        if (!few || !c->dec_s3_ride) { p.s3_ctr = nullptr; }
        if (!few) { p.qtr_summary = nullptr; p.grp_prefix = nullptr; p.share_prefix = nullptr; p.share_sum = nullptr; }
        p.rec_gran = w.take<uint32_t>(Q);
        p.run_cnt = w.take<uint32_t>((flat_total || p.desc_all) ? Q : 0);
        p.run_queue = w.take<uint32_t>((flat_total || p.desc_all) ? Q : 0);
        p.run_desc = w.take<uint4>((size_t)flat_total * p.desc_cap);
        p.sync_fail = w.take<uint8_t>(Q);
        p.recs = w.take<uint32_t>(((Q + 63u) / 64u) * p.rec_rows * 256u);
        if (!pass) { int rc = c->dec_ws.reserve(w.off + 256); if (rc) return rc; }
    }
    if (fused) {
        const size_t words = (size_t)(total / (kScanSegs / 2u)) + 64u;      // (a word per 128 segments where the scan rides on the two-lane transcoder)
        const unsigned gen = c->dec_scan.gen;
        if (c->dec_scan.reserve(words * sizeof(u64)) != QOIMI_OK) { fused = false; p.tr_split = 0u; p.tr_scan = 0u; }          // (no memory for a few KB: the chains will do)
        else {
            c->dec_epoch = (c->dec_epoch + 1u) & 0xFFFFu;
            if (gen != c->dec_scan.gen || c->dec_epoch == 0u) {                           // a new arena, or the tag wraps: no word may carry a tag from before
                HIP_TRY(hipMemsetAsync(c->dec_scan.base, 0, c->dec_scan.cap, st));
                if (c->dec_epoch == 0u) c->dec_epoch = 1u;
            }
            p.fused = 1u; p.epoch = c->dec_epoch; p.scan_status = (u64*)c->dec_scan.base; p.scan_ticket = p.pending + 5;
            p.host_result = &c->host_word[20];
        }
    }
    // Calls of a few images whose predecessor on this context left the counter header zeroed (its dec_fill, see there): the table rides in
    // dec_transcode<0>'s kernel arguments - no copy at all in front of the first kernel.
    const bool hdr_clean = c->dec_hdr_zero.valid && c->dec_hdr_zero.at == (void*)p.pending && c->dec_hdr_zero.gen == c->dec_ws.gen;
    c->dec_hdr_zero.valid = false;
    if (fused && hdr_clean && n_images <= 4) {
        p.tab_in_args = 1u;
        for (int i = 0; i < n_images; ++i) p.tab4[i] = imgs[(size_t)i];
    } else
    {   // image table through pinned staging: no synchronisation (every decode call ends with one, so the staging buffer is free
        // again when the next call fills it).  The four counter words in front of it (pending, redo_segs, sync_fails: the
        // arena's first 256 bytes, the table follows them) travel zeroed in the same copy: no memset launches in round one.
        static_assert(sizeof(DecImage) % 8 == 0, "image table entries keep their alignment behind the counter words");
        const size_t bytes = 256u + imgs.size() * sizeof(DecImage);
        if ((uint8_t*)p.images != (uint8_t*)p.pending + 256u) return fail(QOIMI_E_INTERNAL, "decode workspace layout changed");
        if (bytes > c->pin_cap) {
            if (c->pin_buf) (void)hipHostFree(c->pin_buf);
            c->pin_buf = nullptr; c->pin_cap = 0;
            HIP_TRY(hipHostMalloc(&c->pin_buf, bytes + 4096));
            c->pin_cap = bytes + 4096;
        }
        memset(c->pin_buf, 0, 256);
        memcpy((uint8_t*)c->pin_buf + 256, imgs.data(), bytes - 256u);
        HIP_TRY(hipMemcpyAsync(p.pending, c->pin_buf, bytes, hipMemcpyHostToDevice, st));
    }

    if (fused) launch_decode_fused_front(p, st, &c->timer);
    else launch_decode_parse(p, st, &c->timer);
    long long rounds = 0, stats_seq = 0;
    // A round that re-opens nearly as many segments as the one before it is not getting anywhere (a stream built against the
    // speculation: one verified segment per image and round): two such rounds in a row and the rest goes to the sequential
    // pass at once instead of after dec_max_rounds relaunches over everything (redo_segs accumulates over the rounds).
    uint32_t redo_cum = 0, open_prev = 0xFFFFFFFFu; int stalled = 0;
    for (;;) {
        if (rounds > 0) HIP_TRY(hipMemsetAsync(p.pending, 0, sizeof(uint32_t), st));
        if (rounds > 0 && p.conv) HIP_TRY(hipMemsetAsync(p.conv, 0, 16 * sizeof(uint32_t), st));
        p.l2_tag_base = (uint32_t)rounds * 65536u + 1u;            // (a round launches S3 1 + first_inner / refine_inner times: far fewer than 65536)
        // the first round of a call of a few images: dec_fill leaves the round's counters in pinned host words (no copy back)
        p.tail_fused = (p.fused && rounds == 0) ? 1u : 0u;
        launch_decode_round(p, och, rounds > 0 && c->dec_refine, st, &c->timer);
        ++rounds;
        // pixels the chunks never reach (cheap; redone if the round has to be repeated) - before the read-back,
        // so that the one synchronisation per round also ends the call
        launch_decode_fill(p, och, st, &c->timer);
        c->timer.mark(kT_dec_total, st);
        if (!p.total_segs) { HIP_TRY(hipStreamSynchronize(st)); break; }
        if (p.tail_fused) {
            // dec_fill's first wavefront writes the round's counters into pinned words when everything in front of it - every pixel of the
            // call: dec_segments_rec has ended - is done.  Where no image needs filling (word 23) the call may return on seeing them: the
            // rest of that launch writes nothing.  A few microseconds earlier than the stream's completion signal; after 2 ms of looking (or
            // with per-kernel timing on) the stream is waited for as ever.
            volatile uint32_t* const hw = c->host_word;
            bool seen = false;
            if (!c->timer.on) {
                for (uint32_t spin = 0; spin < 400000u; ++spin) {
                    if (hw[24] == p.epoch) { seen = true; break; }
                    __builtin_ia32_pause();
                }
            }
            if (!seen || hw[23] != 0u) HIP_TRY(hipStreamSynchronize(st));
            else { c->dec_tail_open = true; c->dec_tail_stream = stream; }
            c->host_word[0] = c->host_word[20]; c->host_word[1] = c->host_word[21]; c->host_word[2] = c->host_word[22];
            c->dec_few_longruns = c->host_word[25] >= 1024u;
            // (that dec_fill left the header zeroed; good for the next call if nothing else of this call touches it: no further round)
            c->dec_hdr_zero.at = (void*)p.pending; c->dec_hdr_zero.gen = c->dec_ws.gen; c->dec_hdr_zero.valid = c->host_word[0] == 0u && c->host_word[2] == 0u;
        } else {
            HIP_TRY(hipMemcpyAsync(c->host_word, p.pending, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        timer_collect(c);
        if (p.fused && c->host_word[2] != 0u) {
            // dec_transcode<0> could not synchronise every segment (runs of equally long multi-byte chunks: noise): dec_scan_entry and
            // everything behind it returned at once.  The five-phase parse, the three-level chains and the round again, on the records
            // that stand (the flagged segments are transcoded by dec_transcode<1>).
            p.fused = 0u; fused = false; p.tr_scan = 0u;         // (tr_scan off: the kernels of the chains must not return on sync_fails)
            rounds = 0;
            if (p.fine_per_seg) launch_decode_parse_rest(p, st, &c->timer);
            else launch_decode_parse(p, st, &c->timer);           // (segment sizes without the piece parse: every segment again; sync_fails stands - the call's statistics)
            if (p.conv) HIP_TRY(hipMemsetAsync(p.conv, 0, 16 * sizeof(uint32_t), st));
            continue;
        }
        p.fused = 0u; p.tr_scan = 0u;                       // (rounds after a failed check are the three-level ones, from the image's first bad segment)
        if (c->host_word[0] == 0) break;
        {
            const uint32_t open_now = c->host_word[1] - redo_cum;
            redo_cum = c->host_word[1];
            // (a round that closes less than a 64th of what was open; round 5 asked for a 16th and sent UI frames at small segments - slow
            // but steady, a few per cent per round - to the sequential pass: 30 x the time of the rounds they still needed)
            stalled = (rounds >= 4 && (uint64_t)open_now * 64u > (uint64_t)open_prev * 63u) ? stalled + 1 : 0;
            open_prev = open_now;
        }
        if (rounds >= c->dec_max_rounds || stalled >= 2) {
            // bounded: whatever is still open is finished by the linear sequential pass (see dec_sequential)
            launch_decode_sequential(p, och, st, &c->timer);
            launch_decode_fill(p, och, st, &c->timer);
            c->timer.mark(kT_dec_total, st);
            HIP_TRY(hipStreamSynchronize(st));
            stats_seq = (long long)c->host_word[0];
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    timer_collect(c);
    if (const char* dump = c->dec_debug_dump.empty() ? nullptr : c->dec_debug_dump.c_str()) {                // diagnostics: per-segment arrays of this call, raw
        (void)hipStreamSynchronize(st);
        if (FILE* fo = fopen(dump, "wb")) {
            auto put = [&](const void* d, size_t bytes) { std::vector<uint8_t> h(bytes); (void)hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost); fwrite(h.data(), 1, bytes, fo); };
            const uint64_t hdr[4] = {total, (uint64_t)p.tr_split, (uint64_t)p.rec_rows, (uint64_t)B};
            fwrite(hdr, 8, 4, fo);
            put(p.rec_gran, total * 4); put(p.parse, total * sizeof(ParseRec)); put(p.px_off, total * 4); put(p.sync_fail, total);
            fclose(fo);
        }
    }
    stats[0] = rounds;
    stats[1] = p.total_segs ? c->host_word[1] : 0;
    stats[2] = (long long)total;
    stats[3] = p.total_segs ? c->host_word[2] : 0;
    c->dec_seq_images += stats_seq;
    if (n_images <= 4 && p.total_segs) c->dec_few_syncfail = c->host_word[2] != 0u;
    return QOIMI_OK;
}

// Everything of a decode call behind its argument checks: images at per-image offsets (ascending stream offsets: see qoimi_decode_images).
static int decode_offsets(qoimi_ctx* c, const void* d_streams, const size_t* stream_offs, size_t stream_limit,
                          const int* sizes, const qoi_desc* descs, int n_images, int channels,
                          void* d_pixels, const size_t* pixel_offs, size_t pixel_limit, void* stream) {
    // The chunk records take four bytes per stream byte (worst case) while a call is in flight.  Calls whose streams would
    // need more than dec_rec_cap are decoded as consecutive sub-batches of whole images through the same workspace.
    const uint64_t cap_stream = (uint64_t)(c->dec_rec_cap / 4u) - (uint64_t)(c->dec_rec_cap / 4u) / 64u;
    long long acc[4] = {0, 0, 0, 0};
    auto sub_batches = [&](const int* sz_v, const qoi_desc* ds_v, const size_t* so_v, const size_t* po_v, int n_all, uint32_t B) -> int {
        for (int first = 0; first < n_all;) {
            uint64_t bytes = 0;
            int n = 0;
            while (first + n < n_all) {
                const uint64_t sz = (uint64_t)(sz_v[first + n] > 0 ? sz_v[first + n] : 0) + B;
                if (n > 0 && bytes + sz > cap_stream) break;
                bytes += sz; ++n;
            }
            long long st3[4] = {0, 0, 0, 0};
            const int rc = decode_some(c, d_streams, so_v + first, stream_limit, sz_v + first, ds_v + first, n, channels, d_pixels, po_v + first, pixel_limit, stream, B, st3);
            if (rc != QOIMI_OK) return rc;
            acc[0] = st3[0] > acc[0] ? st3[0] : acc[0]; acc[1] += st3[1]; acc[2] += st3[2]; acc[3] += st3[3];
            first += n;
        }
        return QOIMI_OK;
    };
    // A call that MIXES flat images (UI frames, constant frames: streams of a few hundred KB) with others - a directory of screenshots and
    // photographs - is decoded CLASS BY CLASS: the flat images' passes (a few refinement passes in front of their P4, the P4 that leaves run
    // descriptors) are as long as one lane's walk over one segment, and the segment size the other images' bytes ask for made each of them
    // ~270 us for a few hundred lanes (3 of the mixed directory's 5.4 ms, profiles/r06_s28_mixed_timeline.txt).  Each class takes the
    // segment size of its own bytes; an image's place in the caller's buffers travels in the table (DecImage::stream_off / pixel_off).
    int n_flat = 0;
    if (n_images > 4)
        for (int i = 0; i < n_images; ++i)
            n_flat += (sizes[i] > 22 && descs[i].width != 0 && dec_image_is_flat((uint32_t)sizes[i] - 8u, (uint32_t)((uint64_t)descs[i].width * descs[i].height))) ? 1 : 0;
    if (n_flat != 0 && n_flat != n_images && c->dec_run_desc && c->dec_class_split) {
        for (int cls = 0; cls < 2; ++cls) {
            std::vector<int> sz_v; std::vector<qoi_desc> ds_v; std::vector<size_t> so_v, po_v;
            for (int i = 0; i < n_images; ++i) {
                const bool flat = sizes[i] > 22 && descs[i].width != 0 && dec_image_is_flat((uint32_t)sizes[i] - 8u, (uint32_t)((uint64_t)descs[i].width * descs[i].height));
                if ((flat ? 1 : 0) == cls) { sz_v.push_back(sizes[i]); ds_v.push_back(descs[i]); so_v.push_back(stream_offs[i]); po_v.push_back(pixel_offs[i]); }
            }
            const uint32_t B = choose_seg_bytes(c, sz_v.data(), ds_v.data(), (int)sz_v.size(), cls == 0);      // (QOIMI_SEG_BYTES: the other images' size; the flat class keeps its rule)
            const long long before = acc[0];
            acc[0] = 0;
            const int rc = sub_batches(sz_v.data(), ds_v.data(), so_v.data(), po_v.data(), (int)sz_v.size(), B);
            if (rc != QOIMI_OK) return rc;
            if (cls == 0 && sz_v.size() > 4u) c->dec_nonflat_repair = acc[0] > 1;
            acc[0] = acc[0] > before ? acc[0] : before;
        }
    } else {
        const uint32_t B = choose_seg_bytes(c, sizes, descs, n_images);
        const int rc = sub_batches(sizes, descs, stream_offs, pixel_offs, n_images, B);
        if (rc != QOIMI_OK) return rc;
        if (n_images > 4 && n_flat == 0) c->dec_nonflat_repair = acc[0] > 1;
    }
    c->dec_stats[0] = acc[0]; c->dec_stats[1] = acc[1]; c->dec_stats[2] = acc[2]; c->dec_stats[3] = acc[3];
    return QOIMI_OK;
}

// The strided form: image i at i * stride - a caller of the path above.
extern "C" int qoimi_decode_batch(qoimi_ctx* c, const void* d_streams, size_t stream_stride,
                                  const int* sizes, const qoi_desc* descs, int n_images, int channels,
                                  void* d_pixels, size_t pixel_stride, void* stream) {
    if (!c || !d_streams || !sizes || !descs || !d_pixels || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    for (int i = 1; i < n_images && channels == 0; ++i)
        if (descs[i].channels != descs[0].channels) return fail(QOIMI_E_ARG, "all images of a batch must share the output channel count");
    size_t few[8];                                            // (a call of a few images allocates nothing for its offsets)
    std::vector<size_t> many;
    size_t* so = few; size_t* po = few + 4;
    if (n_images > 4) { many.resize(2u * (size_t)n_images); so = many.data(); po = so + n_images; }
    for (int i = 0; i < n_images; ++i) { so[i] = (size_t)i * stream_stride; po[i] = (size_t)i * pixel_stride; }
    // (a lone stream may be longer than its stride: there is nothing behind it)
    return decode_offsets(c, d_streams, so, n_images == 1 ? ~(size_t)0 : stream_stride, sizes, descs, n_images, channels, d_pixels, po, pixel_stride, stream);
}

// Streams and images wherever the caller's offsets put them.  Two things in the kernels are written for ascending addresses: the
// transcoder's stream descriptor (one per wavefront, from its first lane's stream to its last lane's end) and the pixel writer's (based at
// the image of the wavefront's first segment).  The image table is therefore laid out by ascending STREAM offset here - a sorted pack runs
// as qoimi_decode_batch does; a stream that ends behind its successor's end (overlapping input ranges) is out of its wavefront's reach and
// takes the plain-pointer parse (counted in qoimi_decode_stats [3]); an image that lies in front of its wavefront's base is written with
// plain stores (correct, slower).
extern "C" int qoimi_decode_images(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes,
                                   const qoi_desc* descs, int n_images, int channels,
                                   void* d_pixels, const size_t* pixel_offsets, void* stream) {
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !d_pixels || !pixel_offsets || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    // everything the host can see is looked at before anything is launched: a rejected call leaves the caller's buffers as they were
    std::vector<size_t> out_bytes((size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        if (sizes[i] < kHeaderBytes + kTrailerBytes) return fail(QOIMI_E_ARG, "stream shorter than 22 bytes (qoi.h:500)");
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:513-521 rules)");
        if (channels == 0 && descs[i].channels != descs[0].channels) return fail(QOIMI_E_ARG, "all images of a batch must share the output channel count");
        out_bytes[(size_t)i] = (size_t)descs[i].width * descs[i].height * (size_t)(channels ? channels : descs[i].channels);
    }
    std::vector<int> order((size_t)n_images);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return pixel_offsets[a] < pixel_offsets[b]; });
    for (int k = 1; k < n_images; ++k) {
        const int a = order[(size_t)k - 1], b = order[(size_t)k];
        if (pixel_offsets[a] + out_bytes[(size_t)a] > pixel_offsets[b]) return fail(QOIMI_E_ARG, "the output ranges of two images overlap");
    }
    const bool ascending = std::is_sorted(stream_offsets, stream_offsets + n_images);
    if (ascending) return decode_offsets(c, d_streams, stream_offsets, ~(size_t)0, sizes, descs, n_images, channels, d_pixels, pixel_offsets, ~(size_t)0, stream);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return stream_offsets[a] < stream_offsets[b]; });
    std::vector<size_t> so((size_t)n_images), po((size_t)n_images); std::vector<int> sz((size_t)n_images); std::vector<qoi_desc> ds((size_t)n_images);
    for (int k = 0; k < n_images; ++k) { const int i = order[(size_t)k]; so[(size_t)k] = stream_offsets[i]; po[(size_t)k] = pixel_offsets[i]; sz[(size_t)k] = sizes[i]; ds[(size_t)k] = descs[i]; }
    return decode_offsets(c, d_streams, so.data(), ~(size_t)0, sz.data(), ds.data(), n_images, channels, d_pixels, po.data(), ~(size_t)0, stream);
}

// ------------------------------------------------------------------------------------
// packed streams
// ------------------------------------------------------------------------------------
extern "C" int qoimi_pack_streams(qoimi_ctx* c, const void* d_streams, size_t stream_stride, const int* d_stream_len, int n_streams,
                                  unsigned align, void* d_packed, size_t packed_capacity, unsigned long long* d_packed_off, void* stream) {
    if (!c || !d_streams || !d_stream_len || !d_packed_off || n_streams <= 0 || (!d_packed && packed_capacity != 0)) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (align == 0 || align > 256u || (align & (align - 1u)) != 0) return fail(QOIMI_E_ARG, "align must be a power of two, 1..256");
    if (stream_stride == 0 || stream_stride > (size_t)0x7FFFFFFF + 256u) return fail(QOIMI_E_ARG, "stream_stride out of range");
    {
        const uintptr_t s0 = (uintptr_t)d_streams, s1 = s0 + (size_t)n_streams * stream_stride, p0 = (uintptr_t)d_packed, p1 = p0 + packed_capacity;
        if (packed_capacity != 0 && s0 < p1 && p0 < s1) return fail(QOIMI_E_ARG, "source and destination overlap");
    }
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->timer.n > KernelTimer::kMax - 32) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
    launch_pack_streams((const uint8_t*)d_streams, stream_stride, d_stream_len, (uint32_t)n_streams, align, (uint8_t*)d_packed, packed_capacity,
                        (u64*)d_packed_off, (uint32_t)c->n_cus * 8u, st, &c->timer);
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// encode into a pack through bounded staging
// ------------------------------------------------------------------------------------
// (the sub-batch plan: qoi_stage_plan.h: stage_plan)
static int pin_reserve(qoimi_ctx* c, size_t bytes) {
    if (bytes <= c->pin_cap) return QOIMI_OK;
    if (c->pin_buf) (void)hipHostFree(c->pin_buf);
    c->pin_buf = nullptr; c->pin_cap = 0;
    HIP_TRY(hipHostMalloc(&c->pin_buf, bytes + 4096));
    c->pin_cap = bytes + 4096;
    return QOIMI_OK;
}

// Both entry points: descs holds one descriptor (pixel_offsets == nullptr: image i at i * pixel_stride) or n_images of them.  Every sub-batch
// is one call of the encoder as it is into the staging arena, qoimi_encode_status (which waits for it and encodes it again order-free if a
// placement wait gave up: the pack never takes bytes of a sub-batch whose status has not been looked at), then the append scan and copy on the
// caller's stream; the next sub-batch's encoder is ordered behind that copy by the stream.
static int encode_packed(qoimi_ctx* c, const void* d_pixels, size_t pixel_stride, const size_t* pixel_offsets, const qoi_desc* descs, int n_images,
                         unsigned align, void* d_packed, size_t packed_capacity, unsigned long long* d_packed_off, int* d_stream_len,
                         size_t staging_bytes, unsigned long long* packed_off_out, int* stream_len_out, void* stream) {
    const bool mixed = pixel_offsets != nullptr;
    const size_t n = (size_t)n_images;
    std::vector<size_t> slots(n);
    size_t largest = 0;
    for (size_t i = 0; i < n; ++i) {
        slots[i] = up256(qoimi_encode_bound(&descs[mixed ? i : 0]));
        if (slots[i] > largest) largest = slots[i];
    }
    const StagePlan plan = stage_plan(slots, staging_bytes);
    const std::vector<int>& firsts = plan.firsts;
    const std::vector<size_t>& src = plan.at;                // where stream i lies in the staging of its sub-batch
    const size_t need = plan.need;
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    const size_t table_bytes = mixed ? (n * sizeof(u64) + 255u) & ~(size_t)255u : 0;
    { int rc = c->enc_stage.reserve(table_bytes + need); if (rc) return rc; }
    { int rc = pin_reserve(c, (n + 1u) * sizeof(u64) + n * sizeof(int) + 256u); if (rc) return rc; }
    u64* const d_src = mixed ? (u64*)c->enc_stage.base : nullptr;
    uint8_t* const staging = (uint8_t*)c->enc_stage.base + table_bytes;
    if (mixed) {                                             // where stream j lies in the staging of its sub-batch: one table for the whole call
        for (size_t i = 0; i < n; ++i) ((u64*)c->pin_buf)[i] = (u64)src[i];
        HIP_TRY(hipMemcpyAsync(d_src, c->pin_buf, n * sizeof(u64), hipMemcpyHostToDevice, st));
    }
    int rc = QOIMI_OK;
    for (size_t k = 0; k + 1 < firsts.size() && rc == QOIMI_OK; ++k) {
        const int first = firsts[k], m = firsts[k + 1] - first;
        size_t span = 0;
        for (int i = first; i < first + m; ++i) span += slots[(size_t)i];
        rc = mixed ? qoimi_encode_images(c, d_pixels, pixel_offsets + first, descs + first, m, staging, src.data() + first, d_stream_len + first, stream)
                   : qoimi_encode_batch(c, (const uint8_t*)d_pixels + (size_t)first * pixel_stride, pixel_stride, descs, m, staging, largest, d_stream_len + first, stream);
        if (rc == QOIMI_OK) rc = qoimi_encode_status(c, stream);
        if (rc != QOIMI_OK) break;
        if (c->timer.n > KernelTimer::kMax - 32) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
        // (a stream is no longer than its slot and align is at most 256, so the sub-batch takes no more of the pack than `span` bytes:
        // that many tiles, one more for where the range begins in its first tile and one for the destination's own alignment)
        const size_t tiles = span / kPackTile + 3u, most = (size_t)c->n_cus * 8u;
        launch_pack_append(staging, largest, d_src, d_stream_len, (uint32_t)first, (uint32_t)m, align, (uint8_t*)d_packed, packed_capacity,
                           (u64*)d_packed_off, (uint32_t)(tiles < most ? tiles : most), st, &c->timer);
        if (hipGetLastError() != hipSuccess) rc = fail(QOIMI_E_INTERNAL, "launch of the pack's append kernels failed");
    }
    // whatever happened, qoimi_encode_status must not encode "the last call" again: it went into staging
    c->last_enc.valid = false; c->last_enc_err = nullptr; c->last_enc_err2 = nullptr;
    if (rc != QOIMI_OK) { (void)hipStreamSynchronize(st); return rc; }
    u64* const h_off = (u64*)c->pin_buf; int* const h_len = (int*)(h_off + n + 1u);
    HIP_TRY(hipMemcpyAsync(h_off, d_packed_off, (n + 1u) * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_len, d_stream_len, n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (packed_off_out) memcpy(packed_off_out, h_off, (n + 1u) * sizeof(u64));
    if (stream_len_out) memcpy(stream_len_out, h_len, n * sizeof(int));
    return QOIMI_OK;
}

static int encode_packed_args(qoimi_ctx* c, const void* d_pixels, int n_images, unsigned align, void* d_packed, size_t packed_capacity,
                              const void* d_packed_off, const void* d_stream_len) {
    if (!c || !d_pixels || !d_packed_off || !d_stream_len || n_images <= 0 || (!d_packed && packed_capacity != 0)) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (align == 0 || align > 256u || (align & (align - 1u)) != 0) return fail(QOIMI_E_ARG, "align must be a power of two, 1..256");
    return QOIMI_OK;
}

extern "C" int qoimi_encode_packed(qoimi_ctx* c, const void* d_pixels, size_t pixel_stride, const qoi_desc* desc, int n_images,
                                   unsigned align, void* d_packed, size_t packed_capacity, unsigned long long* d_packed_off, int* d_stream_len,
                                   size_t staging_bytes, unsigned long long* packed_off_out, int* stream_len_out, void* stream) {
    if (int rc = encode_packed_args(c, d_pixels, n_images, align, d_packed, packed_capacity, d_packed_off, d_stream_len)) return rc;
    if (!desc_ok(desc)) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:364-372 rules)");
    if (pixel_stride < (size_t)desc->width * desc->height * desc->channels) return fail(QOIMI_E_ARG, "pixel_stride smaller than one image");
    return encode_packed(c, d_pixels, pixel_stride, nullptr, desc, n_images, align, d_packed, packed_capacity, d_packed_off, d_stream_len,
                         staging_bytes, packed_off_out, stream_len_out, stream);
}

extern "C" int qoimi_encode_images_packed(qoimi_ctx* c, const void* d_pixels, const size_t* pixel_offsets, const qoi_desc* descs, int n_images,
                                          unsigned align, void* d_packed, size_t packed_capacity, unsigned long long* d_packed_off, int* d_stream_len,
                                          size_t staging_bytes, unsigned long long* packed_off_out, int* stream_len_out, void* stream) {
    if (int rc = encode_packed_args(c, d_pixels, n_images, align, d_packed, packed_capacity, d_packed_off, d_stream_len)) return rc;
    if (!pixel_offsets || !descs) return fail(QOIMI_E_ARG, "NULL/empty argument");
    for (int i = 0; i < n_images; ++i) if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:364-372 rules)");
    return encode_packed(c, d_pixels, 0, pixel_offsets, descs, n_images, align, d_packed, packed_capacity, d_packed_off, d_stream_len,
                         staging_bytes, packed_off_out, stream_len_out, stream);
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

extern "C" int qoimi_read_descs(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, int n_streams,
                                qoi_desc* descs_out, int* first_bad, void* stream) {
    if (!c || !d_streams || !stream_offsets || !sizes || !descs_out || n_streams <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    // offsets in, header bytes out: both through the context's pinned staging, which the kernel reads and writes in place
    const size_t n = (size_t)n_streams, bytes = n * (sizeof(u64) + 16u) + 256u;
    if (bytes > c->pin_cap) {
        if (c->pin_buf) (void)hipHostFree(c->pin_buf);
        c->pin_buf = nullptr; c->pin_cap = 0;
        HIP_TRY(hipHostMalloc(&c->pin_buf, bytes + 4096));
        c->pin_cap = bytes + 4096;
    }
    u64* offs = (u64*)c->pin_buf;
    uint8_t* hdr = (uint8_t*)c->pin_buf + ((n * sizeof(u64) + 255u) & ~(size_t)255u);
    for (size_t i = 0; i < n; ++i) offs[i] = sizes[i] >= kHeaderBytes + kTrailerBytes ? (u64)stream_offsets[i] : ~0ull;
    launch_gather_headers((const uint8_t*)d_streams, offs, (uint32_t)n_streams, (uint32_t*)hdr, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    int bad = -1;
    for (size_t i = 0; i < n; ++i) {
        bool ok = false;
        if (sizes[i] >= kHeaderBytes + kTrailerBytes) ok = parse_header(hdr + 16u * i, &descs_out[i]);    // (a shorter stream: qoi_decode returns before it touches *desc, qoi.h:497-503)
        if (!ok && bad < 0) bad = (int)i;
    }
    if (first_bad) *first_bad = bad;
    if (bad >= 0) return fail(QOIMI_E_ARG, "stream " + std::to_string(bad) + ": shorter than 22 bytes or header rejected (qoi.h:497-521 rules)");
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// chunk statistics and strict checks (qoi_inspect.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_stream_info) == sizeof(InsResult) && offsetof(qoimi_stream_info, ops) == 16 && offsetof(qoimi_stream_info, repeat_index) == 40 &&
              offsetof(qoimi_stream_info, walk_end) == 44 && offsetof(qoimi_stream_info, flags) == 48 && offsetof(qoimi_stream_info, reserved) == 52,
              "qoimi_stream_info is what inspect_reduce writes");

extern "C" int qoimi_inspect_streams(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, int n_streams,
                                     qoimi_stream_info* infos_out, int* first_flagged, void* stream) {
    if (!c || !stream_offsets || !sizes || !infos_out || n_streams < 0 || (!d_streams && n_streams > 0)) return fail(QOIMI_E_ARG, "NULL/negative argument");
    const size_t n = (size_t)n_streams;
    const int kMin = kHeaderBytes + kTrailerBytes;
    // the block table's size: a block is up to kInsBlock bytes of ONE stream's body
    size_t nb = 0, npieces = 0;
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] < 0) return fail(QOIMI_E_ARG, "stream " + std::to_string(i) + ": negative size");
        if (sizes[i] <= kMin) continue;
        const size_t body = (size_t)(sizes[i] - kMin);
        nb += (body + kInsBlock - 1u) / kInsBlock;
        npieces += (body + kInsPiece - 1u) / kInsPiece;
    }
    if (nb >= 0x7FFFFFFFu || npieces >= 0xFFFFFFFFu) return fail(QOIMI_E_ARG, "more than 2^31 blocks of stream bytes in one call");
    if (first_flagged) *first_flagged = -1;
    if (n == 0) return QOIMI_OK;
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    if (c->timer.n > KernelTimer::kMax - 32) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
    // pinned staging: [stream table][block table] go to the device, [results][header + trailer bytes] are written by inspect_reduce in place
    auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
    const size_t tab_bytes = up(n * sizeof(InsStream)) + up(nb * sizeof(InsBlock));
    const size_t bytes = tab_bytes + up(n * sizeof(InsResult)) + up(n * 32u);
    if (bytes > c->pin_cap) {
        if (c->pin_buf) (void)hipHostFree(c->pin_buf);
        c->pin_buf = nullptr; c->pin_cap = 0;
        HIP_TRY(hipHostMalloc(&c->pin_buf, bytes + 4096));
        c->pin_cap = bytes + 4096;
    }
    uint8_t* pin = (uint8_t*)c->pin_buf;
    InsStream* h_tab = (InsStream*)pin;
    InsBlock* h_blk = (InsBlock*)(pin + up(n * sizeof(InsStream)));
    InsResult* h_res = (InsResult*)(pin + tab_bytes);
    const uint8_t* h_raw = pin + tab_bytes + up(n * sizeof(InsResult));
    {
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
    // device workspace: the tables, a map and an entry phase per block, a map per piece (2 bytes per 64 stream bytes), a partial per block
    Carver sizer(nullptr);
    sizer.take<uint8_t>(tab_bytes); sizer.take<uint32_t>(nb); sizer.take<uint8_t>(nb); sizer.take<uint16_t>(npieces); sizer.take<InsPartial>(nb);
    { const int rc = c->insp_ws.reserve(sizer.off + 256u); if (rc != QOIMI_OK) return rc; }
    Carver cv(c->insp_ws.base);
    uint8_t* d_tab = cv.take<uint8_t>(tab_bytes);
    uint32_t* d_map = cv.take<uint32_t>(nb);
    uint8_t* d_entry = cv.take<uint8_t>(nb);
    uint16_t* d_piece = cv.take<uint16_t>(npieces);
    InsPartial* d_part = cv.take<InsPartial>(nb);
    HIP_TRY(hipMemcpyAsync(d_tab, pin, tab_bytes, hipMemcpyHostToDevice, st));
    launch_inspect((const uint8_t*)d_streams, (const InsStream*)d_tab, (uint32_t)n, (const InsBlock*)(d_tab + up(n * sizeof(InsStream))), (uint32_t)nb,
                   d_map, d_entry, d_piece, d_part, h_res, (uint32_t*)(pin + tab_bytes + up(n * sizeof(InsResult))), st, &c->timer);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    static const uint8_t kEnd[8] = {0, 0, 0, 0, 0, 0, 0, 1};                // qoi.h:339
    int flagged = -1;
    for (size_t i = 0; i < n; ++i) {
        qoimi_stream_info info;
        memset(&info, 0, sizeof(info));
        if (sizes[i] < kMin) info.flags = QOIMI_SI_TOO_SHORT;
        else {
            memcpy(&info, &h_res[i], sizeof(info));
            const uint8_t* raw = h_raw + 32u * i;
            qoi_desc d;
            unsigned f = 0;
            if (!parse_header(raw, &d)) f |= QOIMI_SI_HEADER_BAD;
            else {
                const unsigned long long want = (unsigned long long)d.width * d.height;
                if (info.pixels < want) f |= QOIMI_SI_PIXELS_SHORT;
                if (info.pixels > want) f |= QOIMI_SI_PIXELS_OVER;
            }
            if (info.walk_end > (unsigned)(sizes[i] - kTrailerBytes)) f |= QOIMI_SI_LAST_CHUNK_CUT;
            if (memcmp(raw + kHeaderBytes, kEnd, 8) != 0) f |= QOIMI_SI_NO_END_MARKER;
            if (info.repeat_index != 0) f |= QOIMI_SI_REPEATED_INDEX;
            info.flags = f;
        }
        infos_out[i] = info;
        if (info.flags != 0 && flagged < 0) flagged = (int)i;
    }
    if (first_flagged) *first_flagged = flagged;
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// images against images, streams against their pixels (qoi_compare.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_image_diff) == sizeof(CmpDiff) && offsetof(qoimi_image_diff, first) == 8 && offsetof(qoimi_image_diff, want) == 16 &&
              offsetof(qoimi_image_diff, got) == 20 && offsetof(qoimi_image_diff, flags) == 24 && offsetof(qoimi_image_diff, reserved) == 28,
              "qoimi_image_diff is what cmp_pixels and cmp_first write");
static_assert(QOIMI_DIFF_PIXELS == 1, "cmp_first writes the flag as a number");

static int cmp_pin_reserve(qoimi_ctx* c, size_t bytes) {
    if (bytes <= c->cmp_pin_cap) return QOIMI_OK;
    if (c->cmp_pin_buf) (void)hipHostFree(c->cmp_pin_buf);
    c->cmp_pin_buf = nullptr; c->cmp_pin_cap = 0;
    HIP_TRY(hipHostMalloc(&c->cmp_pin_buf, bytes + 4096));
    c->cmp_pin_cap = bytes + 4096;
    return QOIMI_OK;
}

// Fills entry `e` for an image of npx pixels and returns the tiles it takes.
static uint32_t cmp_entry(CmpImage* e, size_t a_off, size_t b_off, size_t npx, uint32_t first_tile, unsigned ca, unsigned cb, unsigned ra, unsigned rb, uint32_t index) {
    e->a_off = (u64)a_off; e->b_off = (u64)b_off; e->npx = (uint32_t)npx; e->first_tile = first_tile;
    e->chan = ca | (cb << 8) | (ra << 16) | (rb << 24); e->index = index;
    return (uint32_t)((npx + kCmpTilePx - 1u) / kCmpTilePx);
}

// The two kernels over table entries [from, from + m) of the device table (their tiles begin at 0).  With per-kernel timing on, the stream is
// waited for and the events are folded at once: the interval of a launch that follows must not begin at this one's first event.
static int compare_launch(qoimi_ctx* c, const void* d_a, const void* d_b, const CmpImage* d_tab, uint32_t m, uint32_t tiles, CmpDiff* d_diffs, hipStream_t st) {
    if (c->timer.n > KernelTimer::kMax - 32) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
    const uint32_t most = (uint32_t)c->n_cus * 8u;
    launch_compare((const uint8_t*)d_a, (const uint8_t*)d_b, d_tab, m, tiles, d_diffs, tiles < most ? tiles : most, st, &c->timer);
    HIP_TRY(hipGetLastError());
    if (c->timer.on) { HIP_TRY(hipStreamSynchronize(st)); timer_collect(c); }
    return QOIMI_OK;
}

extern "C" int qoimi_compare_images(qoimi_ctx* c, const void* d_a, const size_t* a_offsets, int a_channels,
                                    const void* d_b, const size_t* b_offsets, int b_channels,
                                    const qoi_desc* descs, int n_images, qoimi_image_diff* diffs_out, int* first_diff, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves diffs_out as it was)
    if (!c || !d_a || !d_b || !a_offsets || !b_offsets || !descs || !diffs_out || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if ((a_channels != 0 && a_channels != 3 && a_channels != 4) || (b_channels != 0 && b_channels != 3 && b_channels != 4))
        return fail(QOIMI_E_ARG, "a_channels / b_channels must be 0, 3 or 4");
    const size_t n = (size_t)n_images;
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(i) + " rejected (qoi.h:364-372 rules)");
        tiles += ((uint64_t)descs[i].width * descs[i].height + kCmpTilePx - 1u) / kCmpTilePx;
    }
    if (tiles >= 0x7FFFFFFFull) return fail(QOIMI_E_ARG, "more than 2^31 tiles of pixels in one call");
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    // pinned staging: [image table][results as they start] go to the device in one copy, [results] come back
    const size_t tab_bytes = up256(n * sizeof(CmpImage)), res_bytes = up256(n * sizeof(CmpDiff));
    { const int rc = cmp_pin_reserve(c, tab_bytes + 2u * res_bytes); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(tab_bytes + res_bytes); if (rc != QOIMI_OK) return rc; }
    uint8_t* pin = (uint8_t*)c->cmp_pin_buf;
    CmpImage* h_tab = (CmpImage*)pin;
    CmpDiff* h_init = (CmpDiff*)(pin + tab_bytes);
    CmpDiff* h_res = (CmpDiff*)(pin + tab_bytes + res_bytes);
    uint32_t t = 0;
    for (size_t i = 0; i < n; ++i) {
        const unsigned ca = a_channels ? (unsigned)a_channels : descs[i].channels, cb = b_channels ? (unsigned)b_channels : descs[i].channels;
        t += cmp_entry(&h_tab[i], a_offsets[i], b_offsets[i], (size_t)descs[i].width * descs[i].height, t, ca, cb, ca, cb, (uint32_t)i);
        memset(&h_init[i], 0, sizeof(CmpDiff));
        h_init[i].first = ~0ull;
    }
    uint8_t* dev = (uint8_t*)c->cmp_ws.base;
    HIP_TRY(hipMemcpyAsync(dev, pin, tab_bytes + n * sizeof(CmpDiff), hipMemcpyHostToDevice, st));
    { const int rc = compare_launch(c, d_a, d_b, (const CmpImage*)dev, (uint32_t)n, t, (CmpDiff*)(dev + tab_bytes), st); if (rc != QOIMI_OK) return rc; }
    HIP_TRY(hipMemcpyAsync(h_res, dev + tab_bytes, n * sizeof(CmpDiff), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int lowest = -1;
    for (size_t i = 0; i < n; ++i) {
        memcpy(&diffs_out[i], &h_res[i], sizeof(qoimi_image_diff));
        if (h_res[i].flags != 0u && lowest < 0) lowest = (int)i;
    }
    if (first_diff) *first_diff = lowest;
    return QOIMI_OK;
}

// An arena of exactly what is asked for plus a page (the staging of qoimi_verify_images: the caller states its size).
static int reserve_exact(Arena& a, size_t bytes) {
    if (bytes <= a.cap) return QOIMI_OK;
    a.release();
    HIP_TRY(hipMalloc(&a.base, bytes + 4096u));
    a.cap = bytes + 4096u; ++a.gen;
    return QOIMI_OK;
}

// Streams against their pixels: every sub-batch of the plan is one call of the decoder as it is into the staging arena (the images whose
// header does not match their descriptor left out), then the compare kernels on the caller's stream - the caller's pixels side A, the staging
// side B; the next sub-batch's decoder is ordered behind them by the stream.  The results stay on the device until the last one is done.
extern "C" int qoimi_verify_images(qoimi_ctx* c, const void* d_pixels, const size_t* pixel_offsets, const qoi_desc* descs, int n_images,
                                   const void* d_streams, const size_t* stream_offsets, const int* sizes, size_t staging_bytes,
                                   qoimi_image_diff* diffs_out, int* first_diff, void* stream) {
    if (!c || !d_pixels || !pixel_offsets || !descs || !d_streams || !stream_offsets || !sizes || !diffs_out || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    const size_t n = (size_t)n_images;
    unsigned och = 3;                                          // ONE output channel count for the staging of the whole call
    uint64_t all_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] < 0) return fail(QOIMI_E_ARG, "stream " + std::to_string(i) + ": negative size");
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(i) + " rejected (qoi.h:364-372 rules)");
        if (descs[i].channels == 4) och = 4;
        all_tiles += ((uint64_t)descs[i].width * descs[i].height + kCmpTilePx - 1u) / kCmpTilePx;
    }
    if (all_tiles >= 0x7FFFFFFFull) return fail(QOIMI_E_ARG, "more than 2^31 tiles of pixels in one call");
    // the plan: a function of descs and staging_bytes alone (qoi_amd/packplan.py: plan over width * height * och)
    std::vector<size_t> slots(n);
    for (size_t i = 0; i < n; ++i) slots[i] = up256((size_t)descs[i].width * descs[i].height * och);
    const StagePlan plan = stage_plan(slots, staging_bytes);
    const std::vector<int>& firsts = plan.firsts;
    const std::vector<size_t>& at = plan.at;
    const size_t need = plan.need;
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    // pinned staging: [image table][results as they start] go to the device in one copy, [results] come back; [offsets][header bytes] are
    // read and written in place by gather_headers
    const size_t tab_bytes = up256(n * sizeof(CmpImage)), res_bytes = up256(n * sizeof(CmpDiff)), off_bytes = up256(n * sizeof(u64));
    { const int rc = cmp_pin_reserve(c, tab_bytes + 2u * res_bytes + off_bytes + n * 16u); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(tab_bytes + res_bytes); if (rc != QOIMI_OK) return rc; }
    { const int rc = reserve_exact(c->ver_stage, need); if (rc != QOIMI_OK) return rc; }
    uint8_t* pin = (uint8_t*)c->cmp_pin_buf;
    CmpImage* h_tab = (CmpImage*)pin;
    CmpDiff* h_init = (CmpDiff*)(pin + tab_bytes);
    CmpDiff* h_res = (CmpDiff*)(pin + tab_bytes + res_bytes);
    u64* h_off = (u64*)(pin + tab_bytes + 2u * res_bytes);
    const uint8_t* h_hdr = pin + tab_bytes + 2u * res_bytes + off_bytes;
    // 1. the headers: a stream that is too short, fails the rules of qoimi_read_descs or says something else than descs[i] is not decoded
    const int kMin = kHeaderBytes + kTrailerBytes;
    for (size_t i = 0; i < n; ++i) h_off[i] = sizes[i] >= kMin ? (u64)stream_offsets[i] : ~0ull;
    launch_gather_headers((const uint8_t*)d_streams, h_off, (uint32_t)n, (uint32_t*)h_hdr, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint8_t> header_bad(n);
    for (size_t i = 0; i < n; ++i) {
        qoi_desc d;
        header_bad[i] = !(sizes[i] >= kMin && parse_header(h_hdr + 16u * i, &d) && d.width == descs[i].width && d.height == descs[i].height &&
                          d.channels == descs[i].channels && d.colorspace == descs[i].colorspace);
    }
    // 2. one table for the whole call: the entries of a sub-batch's decoded images stand together, their tiles begin at 0
    struct Sub { uint32_t entry, m, tiles; };
    std::vector<Sub> subs(firsts.size() - 1u);
    uint32_t entries = 0;
    for (size_t k = 0; k + 1 < firsts.size(); ++k) {
        Sub& s = subs[k];
        s.entry = entries; s.tiles = 0;
        for (int i = firsts[k]; i < firsts[k + 1]; ++i) {
            if (header_bad[(size_t)i]) continue;
            const unsigned ch = descs[i].channels;             // a_channels = 0; side B holds och bytes per pixel and stands for a decode at ch
            s.tiles += cmp_entry(&h_tab[entries++], pixel_offsets[i], at[(size_t)i], (size_t)descs[i].width * descs[i].height, s.tiles, ch, och, ch, ch, (uint32_t)i);
        }
        s.m = entries - s.entry;
    }
    for (size_t i = 0; i < n; ++i) { memset(&h_init[i], 0, sizeof(CmpDiff)); h_init[i].first = ~0ull; }
    uint8_t* dev = (uint8_t*)c->cmp_ws.base;
    CmpDiff* d_diffs = (CmpDiff*)(dev + tab_bytes);
    HIP_TRY(hipMemcpyAsync(dev, pin, tab_bytes + n * sizeof(CmpDiff), hipMemcpyHostToDevice, st));
    // 3. sub-batch by sub-batch
    std::vector<size_t> so, po; std::vector<int> sz; std::vector<qoi_desc> ds;
    for (size_t k = 0; k < subs.size(); ++k) {
        if (subs[k].m == 0u) continue;
        so.clear(); po.clear(); sz.clear(); ds.clear();
        for (int i = firsts[k]; i < firsts[k + 1]; ++i) {
            if (header_bad[(size_t)i]) continue;
            so.push_back(stream_offsets[i]); po.push_back(at[(size_t)i]); sz.push_back(sizes[i]); ds.push_back(descs[i]);
        }
        const int rc = qoimi_decode_images(c, d_streams, so.data(), sz.data(), ds.data(), (int)subs[k].m, (int)och, c->ver_stage.base, po.data(), stream);
        if (rc != QOIMI_OK) { (void)hipStreamSynchronize(st); return rc; }
        const int rc2 = compare_launch(c, d_pixels, c->ver_stage.base, (const CmpImage*)dev + subs[k].entry, subs[k].m, subs[k].tiles, d_diffs, st);
        if (rc2 != QOIMI_OK) { (void)hipStreamSynchronize(st); return rc2; }
    }
    // 4. one read-back
    HIP_TRY(hipMemcpyAsync(h_res, d_diffs, n * sizeof(CmpDiff), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int lowest = -1;
    for (size_t i = 0; i < n; ++i) {
        if (header_bad[i]) {
            memset(&diffs_out[i], 0, sizeof(qoimi_image_diff));
            diffs_out[i].first = ~0ull; diffs_out[i].flags = QOIMI_DIFF_HEADER;
        } else memcpy(&diffs_out[i], &h_res[i], sizeof(qoimi_image_diff));
        if (diffs_out[i].flags != 0u && lowest < 0) lowest = (int)i;
    }
    if (first_diff) *first_diff = lowest;
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// decode through staging, then one table-driven kernel per sub-batch: what qoimi_decode_thumbnails, qoimi_decode_crops and
// qoimi_decode_resized share (their plans: qoi_stage_plan.h)
// ------------------------------------------------------------------------------------
// Sub-batch k of the plan into the staging arena: one call of the decoder as it is, at 4 output channels (every staged pixel an aligned
// dword) and with each descriptor's height shortened to the image's rows (the decoder decodes to the descriptor it is given: the prefix of
// the full decode).
static int decode_rows(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs, const RowsPlan& p,
                       const std::vector<uint32_t>& rows, size_t k, void* stream) {
    const int first = p.firsts[k], m = p.firsts[k + 1] - first;
    std::vector<size_t> so; std::vector<int> sz; std::vector<qoi_desc> ds;
    for (int r = first; r < first + m; ++r) {
        const int i = p.refs[(size_t)r];
        qoi_desc d = descs[i];
        d.height = rows[(size_t)i];
        so.push_back(stream_offsets[i]); sz.push_back(sizes[i]); ds.push_back(d);
    }
    return qoimi_decode_images(c, d_streams, so.data(), sz.data(), ds.data(), m, 4, c->ver_stage.base, p.at.data() + first, stream);
}

// What check_items makes of a call's items.  rows[i]: the rows of image i that are decoded, 0: no item names it; out_bytes[j]: the bytes of
// output j; och: the output channel count of the call.
struct CheckedItems { std::vector<uint32_t> rows; std::vector<size_t> out_bytes; unsigned och = 0; };

// The items of qoimi_decode_crops (`noun` "crop"), of qoimi_decode_resized ("item") and of qoimi_pixel_stats ("region"), looked at in the order
// that decides which message a call with several faults gets.  wrong(desc, item): nullptr if the item is fine for an accepted descriptor, else
// what is wrong with it; output(j, item, och): QOIMI_OK, or the failure of item j's output (a call without outputs: always QOIMI_OK).
template <class Item, class Wrong, class Output>
static int check_refs(const std::string& noun, const int* sizes, const qoi_desc* descs, int n_images, int channels, const Item* items, size_t n,
                      Wrong wrong, Output output, CheckedItems& out) {
    std::vector<uint32_t>& rows = out.rows;
    rows.assign((size_t)n_images, 0u);
    unsigned och = (unsigned)channels;
    for (size_t j = 0; j < n; ++j) {
        const Item& r = items[j];
        if (r.image >= (unsigned)n_images) return fail(QOIMI_E_ARG, noun + " " + std::to_string(j) + ": no image " + std::to_string(r.image));
        const size_t i = r.image;
        if (rows[i] == 0u) {                                   // (an image no item names is never looked at)
            if (sizes[i] < kHeaderBytes + kTrailerBytes) return fail(QOIMI_E_ARG, "stream " + std::to_string(i) + " shorter than 22 bytes (qoi.h:500)");
            if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(i) + " rejected (qoi.h:513-521 rules)");
        }
        if (channels == 0) {
            if (och == 0u) och = descs[i].channels;
            else if (descs[i].channels != och) return fail(QOIMI_E_ARG, "all referenced images of a call must share the output channel count");
        }
        if (const char* what = wrong(&descs[i], &r)) return fail(QOIMI_E_ARG, noun + " " + std::to_string(j) + ": " + what);
        if (r.y + r.height > rows[i]) rows[i] = r.y + r.height;
        if (const int rc = output(j, &r, och)) return rc;
    }
    out.och = och;
    return QOIMI_OK;
}

// check_refs for the calls that write an output per item at d_out + out_offsets[j]: bytes_of(item, och, &bytes): false if the output's size
// does not fit a size_t; no output may end behind the address space, no two may overlap.
template <class Item, class Wrong, class Bytes>
static int check_items(const std::string& noun, const int* sizes, const qoi_desc* descs, int n_images, int channels, const Item* items, size_t n,
                       const void* d_out, const size_t* out_offsets, Wrong wrong, Bytes bytes_of, CheckedItems& out) {
    out.out_bytes.resize(n);
    const uintptr_t room = ~(uintptr_t)0 - (uintptr_t)d_out;       // (so that no address of an output wraps, whatever the offsets)
    if (const int rc = check_refs(noun, sizes, descs, n_images, channels, items, n, wrong, [&](size_t j, const Item* r, unsigned och) {
            if (!bytes_of(r, och, &out.out_bytes[j]) || out_offsets[j] > room || out.out_bytes[j] > room - out_offsets[j]) return fail
               (QOIMI_E_ARG, noun + " " + std::to_string(j) + ": the output ends behind the address space");
            return (int)QOIMI_OK;
        }, out)) return rc;
    if (ranges_overlap(out_offsets, out.out_bytes)) return fail(QOIMI_E_ARG, "the output ranges of two " + noun + "s overlap");
    return QOIMI_OK;
}

// Everything behind "the plan is made and the call is accepted".  One table for the whole call, through pinned staging: fill(entry, e) writes
// entry e (of item items.by_ref[e]; the entries of a sub-batch stand together, their tiles begin at 0).  Then, sub-batch by sub-batch, one call
// of the decoder as it is into the staging arena and one launch over the sub-batch's entries on the caller's stream -
// launch(its entries on the device, m, tiles, workgroups, stream), `kernel` in the message if it fails; the next sub-batch's decoder is ordered
// behind it by the stream.  stats: sub-batches decoded, launches, bytes of staging planned, `decoded`.
// extra != 0: that many bytes of results stand behind the table (256-aligned: staged_extra_at) on the device and in the pinned staging;
// begin(pinned bytes, stream) sets them as they start - they go to the device with the table - and may enqueue more; they are copied back
// behind the last launch and are the call's when QOIMI_OK is returned.
static size_t staged_extra_at(size_t n, size_t entry_bytes) { return up256(n * entry_bytes); }

template <class Entry, class Fill, class Launch, class Begin>
static int run_staged(qoimi_ctx* c, long long (&stats)[4], long long decoded, const char* kernel, const void* d_streams, const size_t* stream_offsets,
                      const int* sizes, const qoi_desc* descs, const RowsPlan& plan, const std::vector<uint32_t>& rows, const ItemPlan& items,
                      Fill fill, Launch launch, void* stream, size_t extra, Begin begin) {
    const size_t n = items.by_ref.size();
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    stats[0] = 0; stats[1] = 0; stats[2] = (long long)plan.need; stats[3] = decoded;
    if (c->dec_tail_open && c->dec_tail_stream != stream) HIP_TRY(hipStreamSynchronize((hipStream_t)c->dec_tail_stream));
    const size_t tab_bytes = staged_extra_at(n, sizeof(Entry));
    { const int rc = cmp_pin_reserve(c, tab_bytes + extra); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(tab_bytes + extra); if (rc != QOIMI_OK) return rc; }
    { const int rc = reserve_exact(c->ver_stage, plan.need); if (rc != QOIMI_OK) return rc; }
    Entry* h_tab = (Entry*)c->cmp_pin_buf;
    for (size_t e = 0; e < n; ++e) fill(h_tab[e], e);
    const Entry* d_tab = (const Entry*)c->cmp_ws.base;
    if (extra != 0u) { const int rc = begin((uint8_t*)c->cmp_pin_buf + tab_bytes, st); if (rc != QOIMI_OK) return rc; }
    HIP_TRY(hipMemcpyAsync(c->cmp_ws.base, h_tab, extra != 0u ? tab_bytes + extra : n * sizeof(Entry), hipMemcpyHostToDevice, st));
    const uint32_t most = (uint32_t)c->n_cus * 8u;
    for (size_t k = 0; k < items.subs.size(); ++k) {
        const ItemSub& s = items.subs[k];
        const int rc = decode_rows(c, d_streams, stream_offsets, sizes, descs, plan, rows, k, stream);
        if (rc != QOIMI_OK) { (void)hipStreamSynchronize(st); return rc; }
        stats[0] += 1;
        launch(d_tab + s.entry, s.m, s.tiles, s.tiles < most ? s.tiles : most, st);
        { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(QOIMI_E_INTERNAL, std::string(kernel) + ": " + hipGetErrorString(e)); } }
        stats[1] += 1;
    }
    if (extra != 0u) HIP_TRY(hipMemcpyAsync((uint8_t*)c->cmp_pin_buf + tab_bytes, (const uint8_t*)c->cmp_ws.base + tab_bytes, extra, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return QOIMI_OK;
}

// ... for the calls whose kernels write the caller's device memory and nothing else
template <class Entry, class Fill, class Launch>
static int run_staged(qoimi_ctx* c, long long (&stats)[4], long long decoded, const char* kernel, const void* d_streams, const size_t* stream_offsets,
                      const int* sizes, const qoi_desc* descs, const RowsPlan& plan, const std::vector<uint32_t>& rows, const ItemPlan& items,
                      Fill fill, Launch launch, void* stream) {
    return run_staged<Entry>(c, stats, decoded, kernel, d_streams, stream_offsets, sizes, descs, plan, rows, items, fill, launch, stream, (size_t)0,
                             [](uint8_t*, hipStream_t) { return (int)QOIMI_OK; });
}

// ------------------------------------------------------------------------------------
// thumbnails of a pack (qoi_thumb.hip)
// ------------------------------------------------------------------------------------
static_assert(QOIMI_THUMB_PLAIN == 0 && QOIMI_THUMB_ALPHA_WEIGHTED == 1, "the table's mode bit");

extern "C" size_t qoimi_thumbnail_size(const qoi_desc* desc, unsigned factor, int channels, unsigned* tw, unsigned* th) {
    if (!desc_ok(desc) || factor < 1u || factor > kThumbMaxFactor || (channels != 3 && channels != 4)) return 0;
    const uint32_t x = thumb_extent(desc->width, factor), y = thumb_extent(desc->height, factor);
    if (tw) *tw = x;
    if (th) *th = y;
    return (size_t)x * y * (size_t)channels;
}

extern "C" void qoimi_thumbnail_stats(qoimi_ctx* c, long long out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = c ? c->thumb_stats[i] : 0;
}

// The plan of the gather calls with every image referenced at its full height and item j naming image j (qoi_amd/packplan.py: plan over
// width * height * 4); run_staged with one launch of thumb_reduce per sub-batch.
extern "C" int qoimi_decode_thumbnails(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                       int n_images, int channels, const unsigned* factors, int mode, void* d_thumbs, const size_t* thumb_offsets,
                                       size_t staging_bytes, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !factors || !d_thumbs || !thumb_offsets || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    if (mode != QOIMI_THUMB_PLAIN && mode != QOIMI_THUMB_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_THUMB_PLAIN or QOIMI_THUMB_ALPHA_WEIGHTED");
    const size_t n = (size_t)n_images;
    std::vector<size_t> out_bytes(n);
    std::vector<uint32_t> rows(n), image_of(n);
    std::vector<uint64_t> tiles_of(n);
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] < kHeaderBytes + kTrailerBytes) return fail(QOIMI_E_ARG, "stream " + std::to_string(i) + " shorter than 22 bytes (qoi.h:500)");
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(i) + " rejected (qoi.h:513-521 rules)");
        if (channels == 0 && descs[i].channels != descs[0].channels) return fail(QOIMI_E_ARG, "all images of a call must share the output channel count");
        if (factors[i] < 1u || factors[i] > kThumbMaxFactor) return fail(QOIMI_E_ARG, "factor " + std::to_string(i) + " outside 1..64");
        out_bytes[i] = (size_t)thumb_extent(descs[i].width, factors[i]) * thumb_extent(descs[i].height, factors[i]) * (size_t)(channels ? channels : descs[i].channels);
        rows[i] = descs[i].height; image_of[i] = (uint32_t)i;
        tiles_of[i] = thumb_tiles(descs[i].width, descs[i].height, factors[i]);
    }
    const unsigned och = channels ? (unsigned)channels : descs[0].channels;
    // (unlike check_items, this call has never looked whether an output ends inside the address space)
    if (ranges_overlap(thumb_offsets, out_bytes)) return fail(QOIMI_E_ARG, "the output ranges of two thumbnails overlap");
    const RowsPlan plan = plan_rows(descs, n_images, rows, staging_bytes);
    const ItemPlan items = plan_items(image_of, plan.ref_of, plan.firsts, tiles_of);   // (entry i is image i)
    if (items.overflow) return fail(QOIMI_E_ARG, "more than 2^31 tiles of thumbnail pixels in one sub-batch");
    const uint32_t weighted = (mode == QOIMI_THUMB_ALPHA_WEIGHTED && och == 4u) ? 1u : 0u;   // with 3 output channels the mode is PLAIN
    return run_staged<ThumbImage>(c, c->thumb_stats, 0, "thumb_reduce", d_streams, stream_offsets, sizes, descs, plan, rows, items,
        [&](ThumbImage& e, size_t i) {
            uint32_t lg, cols;
            thumb_split(factors[i], lg, cols);
            e.src_off = (u64)plan.at[i]; e.dst_off = (u64)thumb_offsets[i];
            e.w = descs[i].width; e.h = descs[i].height; e.f = factors[i];
            e.tw = thumb_extent(e.w, e.f); e.th = thumb_extent(e.h, e.f);
            e.first_tile = items.first_tile[i]; e.cfg = lg | (cols << 8) | (och << 16) | (weighted << 24); e.reserved = 0u;
        },
        [&](const ThumbImage* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            launch_thumb((const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_thumbs, grid, st);
        }, stream);
}

// ------------------------------------------------------------------------------------
// rectangles of a pack's images (qoi_crop.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_crop) == 24 && offsetof(qoimi_crop, image) == 0 && offsetof(qoimi_crop, x) == 4 && offsetof(qoimi_crop, y) == 8 &&
              offsetof(qoimi_crop, width) == 12 && offsetof(qoimi_crop, height) == 16 && offsetof(qoimi_crop, flags) == 20, "qoimi_crop layout");
static_assert(QOIMI_CROP_FLIP_X == (int)kCropFlipX && QOIMI_CROP_FLIP_Y == (int)kCropFlipY, "the table's flag bits");

// nullptr if the rectangle is fine for an accepted descriptor, else what is wrong with it
static const char* crop_rect_wrong(const qoi_desc* d, const qoimi_crop* r) {
    if (r->width == 0u || r->height == 0u) return "zero width or height";
    if ((r->flags & ~(unsigned)(QOIMI_CROP_FLIP_X | QOIMI_CROP_FLIP_Y)) != 0u) return "unknown flag bit";
    if ((uint64_t)r->x + r->width > d->width || (uint64_t)r->y + r->height > d->height) return "the rectangle leaves its image";
    return nullptr;
}

// width * height * och (a rectangle inside an image: it always fits)
static bool crop_bytes(const qoimi_crop* r, unsigned och, size_t* bytes) {
    *bytes = (size_t)r->width * r->height * och;
    return true;
}

extern "C" size_t qoimi_crop_size(const qoi_desc* desc, const qoimi_crop* crop, int channels) {
    if (!desc_ok(desc) || !crop || (channels != 3 && channels != 4) || crop_rect_wrong(desc, crop)) return 0;
    return (size_t)crop->width * crop->height * (size_t)channels;
}

extern "C" void qoimi_crop_stats(qoimi_ctx* c, long long out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = c ? c->crop_stats[i] : 0;
}

// The referenced images, in ascending order, are planned into sub-batches over slots of w * rows * 4 bytes, rows the last row any crop of
// the image needs (qoi_amd/crops.py: plan - a function of descs, crops and staging_bytes alone); run_staged with one launch of crop_gather
// over the sub-batch's crops.
extern "C" int qoimi_decode_crops(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                  int n_images, int channels, const qoimi_crop* crops, int n_crops, void* d_out, const size_t* out_offsets,
                                  size_t staging_bytes, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !crops || !d_out || !out_offsets || n_images <= 0 || n_crops <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    const size_t n = (size_t)n_crops;
    CheckedItems ok;
    if (const int rc = check_items("crop", sizes, descs, n_images, channels, crops, n, d_out, out_offsets, crop_rect_wrong, crop_bytes, ok)) return rc;
    const unsigned och = ok.och;
    const RowsPlan plan = plan_rows(descs, n_images, ok.rows, staging_bytes);
    std::vector<uint32_t> image_of(n);
    std::vector<uint64_t> tiles_of(n);
    for (size_t j = 0; j < n; ++j) { image_of[j] = crops[j].image; tiles_of[j] = crop_tiles((uint64_t)(uintptr_t)d_out + out_offsets[j], ok.out_bytes[j]); }
    const ItemPlan items = plan_items(image_of, plan.ref_of, plan.firsts, tiles_of);
    if (items.overflow) return fail(QOIMI_E_ARG, "more than 2^31 tiles of output words in one sub-batch");
    return run_staged<CropEntry>(c, c->crop_stats, (long long)plan.refs.size(), "crop_gather", d_streams, stream_offsets, sizes, descs, plan, ok.rows, items,
        [&](CropEntry& t, size_t e) {
            const size_t j = items.by_ref[e];
            const qoimi_crop& r = crops[j];
            t.src_off = (u64)plan.at[(size_t)plan.ref_of[r.image]]; t.dst_off = (u64)out_offsets[j];
            t.w = descs[r.image].width; t.x = r.x; t.y = r.y; t.cw = r.width; t.ch = r.height;
            t.first_tile = items.first_tile[e]; t.cfg = och | (r.flags << 8); t.reserved = 0u;
        },
        [&](const CropEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            launch_crop((const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, grid, st);
        }, stream);
}

// ------------------------------------------------------------------------------------
// rectangles of a pack's images resampled to fixed sizes (qoi_resize.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_resize) == 32 && offsetof(qoimi_resize, image) == 0 && offsetof(qoimi_resize, x) == 4 && offsetof(qoimi_resize, y) == 8 &&
              offsetof(qoimi_resize, width) == 12 && offsetof(qoimi_resize, height) == 16 && offsetof(qoimi_resize, out_width) == 20 &&
              offsetof(qoimi_resize, out_height) == 24 && offsetof(qoimi_resize, flags) == 28, "qoimi_resize layout");
static_assert(QOIMI_RESIZE_FLIP_X == (int)kResizeFlipX && QOIMI_RESIZE_FLIP_Y == (int)kResizeFlipY, "the table's flag bits");
static_assert(QOIMI_RESIZE_PLAIN == 0 && QOIMI_RESIZE_ALPHA_WEIGHTED == 1, "the table's mode bit");

// nullptr if the item is fine for an accepted descriptor, else what is wrong with it
static const char* resize_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (r->width == 0u || r->height == 0u || r->out_width == 0u || r->out_height == 0u) return "zero width or height";
    if ((r->flags & ~(unsigned)(QOIMI_RESIZE_FLIP_X | QOIMI_RESIZE_FLIP_Y)) != 0u) return "unknown flag bit";
    if ((uint64_t)r->x + r->width > d->width || (uint64_t)r->y + r->height > d->height) return "the rectangle leaves its image";
    if (r->width > (uint64_t)kResizeMaxRatio * r->out_width || r->height > (uint64_t)kResizeMaxRatio * r->out_height) return "reduced by more than 64 in an axis";
    return nullptr;
}

// out_width * out_height * och, false if that does not fit a size_t
static bool resize_bytes(const qoimi_resize* r, unsigned och, size_t* bytes) {
    const uint64_t px = (uint64_t)r->out_width * r->out_height;
    if (px > ~(size_t)0 / och) return false;
    *bytes = (size_t)px * och;
    return true;
}

extern "C" size_t qoimi_resize_size(const qoi_desc* desc, const qoimi_resize* item, int channels) {
    size_t bytes = 0;
    if (!desc_ok(desc) || !item || (channels != 3 && channels != 4) || resize_item_wrong(desc, item) || !resize_bytes(item, (unsigned)channels, &bytes)) return 0;
    return bytes;
}

extern "C" void qoimi_resize_stats(qoimi_ctx* c, long long out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = c ? c->resize_stats[i] : 0;
}

// The plan of qoimi_decode_crops over the items' rectangles (qoi_amd/resize.py: plan); run_staged with one launch of resize_filter over the
// sub-batch's items.
extern "C" int qoimi_decode_resized(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                    int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                    size_t staging_bytes, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    if (mode != QOIMI_RESIZE_PLAIN && mode != QOIMI_RESIZE_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_RESIZE_PLAIN or QOIMI_RESIZE_ALPHA_WEIGHTED");
    const size_t n = (size_t)n_items;
    CheckedItems ok;
    if (const int rc = check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, resize_item_wrong, resize_bytes, ok)) return rc;
    const unsigned och = ok.och;
    const RowsPlan plan = plan_rows(descs, n_images, ok.rows, staging_bytes);
    std::vector<uint32_t> image_of(n);
    std::vector<uint64_t> tiles_of(n);
    for (size_t j = 0; j < n; ++j) { image_of[j] = items[j].image; tiles_of[j] = resize_tiles(items[j].width, items[j].out_width, items[j].out_height); }
    const ItemPlan order = plan_items(image_of, plan.ref_of, plan.firsts, tiles_of);
    if (order.overflow) return fail(QOIMI_E_ARG, "more than 2^31 tiles of output pixels in one sub-batch");
    const uint32_t weighted = (mode == QOIMI_RESIZE_ALPHA_WEIGHTED && och == 4u) ? 1u : 0u;   // with 3 output channels the mode is PLAIN
    return run_staged<ResizeEntry>(c, c->resize_stats, (long long)plan.refs.size(), "resize_filter", d_streams, stream_offsets, sizes, descs, plan, ok.rows, order,
        [&](ResizeEntry& t, size_t e) {
            const size_t j = order.by_ref[e];
            const qoimi_resize& r = items[j];
            uint32_t lg, cols;
            resize_split(r.width, r.out_width, lg, cols);
            t.src_off = (u64)plan.at[(size_t)plan.ref_of[r.image]]; t.dst_off = (u64)out_offsets[j];
            t.w = descs[r.image].width; t.x = r.x; t.y = r.y; t.cw = r.width; t.rh = r.height; t.ow = r.out_width; t.oh = r.out_height;
            t.first_tile = order.first_tile[e]; t.cfg = lg | (cols << 8) | (och << 16) | (weighted << 24) | (r.flags << 28); t.reserved = 0u;
        },
        [&](const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            launch_resize((const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, grid, st);
        }, stream);
}

// ------------------------------------------------------------------------------------
// pixel statistics of rectangles of a pack's images (qoi_stats.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_pixel_stat) == 128 && offsetof(qoimi_pixel_stat, sum) == 8 && offsetof(qoimi_pixel_stat, sum_sq) == 40 &&
              offsetof(qoimi_pixel_stat, min) == 72 && offsetof(qoimi_pixel_stat, max) == 76 && offsetof(qoimi_pixel_stat, first) == 80 &&
              offsetof(qoimi_pixel_stat, flags) == 84 && offsetof(qoimi_pixel_stat, opaque_pixels) == 88 && offsetof(qoimi_pixel_stat, transparent_pixels) == 96 &&
              offsetof(qoimi_pixel_stat, grey_pixels) == 104 && offsetof(qoimi_pixel_stat, reserved) == 112, "qoimi_pixel_stat layout");
static_assert(QOIMI_PS_CONSTANT == (int)kStatsConstant && QOIMI_PS_OPAQUE == (int)kStatsOpaque && QOIMI_PS_TRANSPARENT == (int)kStatsTransparent &&
              QOIMI_PS_GREY == (int)kStatsGrey, "stats_flags gives the flags as numbers");
static_assert(QOIMI_CROP_FLIP_X == (int)kStatsFlipX && QOIMI_CROP_FLIP_Y == (int)kStatsFlipY, "the table's flag bits");

extern "C" void qoimi_pixel_stats_counters(qoimi_ctx* c, long long out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = c ? c->pixel_stats[i] : 0;
}

// The plan of qoimi_decode_crops over the regions (qoi_amd/pixelstats.py: plan); run_staged with one launch of stats_reduce over the
// sub-batch's regions.  The result table stands behind the region table; `first`, the sums and the extremes come back from the device,
// `pixels` and `flags` are made of them here.
extern "C" int qoimi_pixel_stats(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                 int n_images, const qoimi_crop* regions, int n_regions, qoimi_pixel_stat* stats_out, unsigned* d_hist,
                                 size_t staging_bytes, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves stats_out as it was)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !regions || !stats_out || n_images <= 0 || n_regions <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    const size_t n = (size_t)n_regions;
    CheckedItems ok;
    if (const int rc = check_refs("region", sizes, descs, n_images, 4, regions, n, crop_rect_wrong,
                                  [](size_t, const qoimi_crop*, unsigned) { return (int)QOIMI_OK; }, ok)) return rc;
    const RowsPlan plan = plan_rows(descs, n_images, ok.rows, staging_bytes);
    std::vector<uint32_t> image_of(n);
    std::vector<uint64_t> tiles_of(n);
    for (size_t j = 0; j < n; ++j) { image_of[j] = regions[j].image; tiles_of[j] = stats_tiles(regions[j].width, regions[j].height); }
    const ItemPlan items = plan_items(image_of, plan.ref_of, plan.firsts, tiles_of);
    if (items.overflow) return fail(QOIMI_E_ARG, "more than 2^31 tiles of region pixels in one sub-batch");
    const size_t res_at = staged_extra_at(n, sizeof(StatsEntry));
    const int rc = run_staged<StatsEntry>(c, c->pixel_stats, (long long)plan.refs.size(), "stats_reduce", d_streams, stream_offsets, sizes, descs, plan, ok.rows, items,
        [&](StatsEntry& t, size_t e) {
            const size_t j = items.by_ref[e];
            const qoimi_crop& r = regions[j];
            t.src_off = (u64)plan.at[(size_t)plan.ref_of[r.image]];
            t.w = descs[r.image].width; t.x = r.x; t.y = r.y; t.cw = r.width; t.ch = r.height;
            t.first_tile = items.first_tile[e]; t.index = (uint32_t)j; t.cfg = r.flags; t.reserved[0] = 0u; t.reserved[1] = 0u;
        },
        [&](const StatsEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            launch_stats((const uint8_t*)c->ver_stage.base, tab, m, tiles, (StatsAcc*)((uint8_t*)c->cmp_ws.base + res_at), d_hist, grid, st);
        }, stream, n * sizeof(StatsAcc),
        [&](uint8_t* h_res, hipStream_t st) {
            for (size_t j = 0; j < n; ++j) stats_init(((StatsAcc*)h_res)[j]);
            if (d_hist) HIP_TRY(hipMemsetAsync(d_hist, 0, n * kStatsBins * sizeof(unsigned), st));
            return (int)QOIMI_OK;
        });
    if (rc != QOIMI_OK) return rc;
    const StatsAcc* h_res = (const StatsAcc*)((const uint8_t*)c->cmp_pin_buf + res_at);
    for (size_t j = 0; j < n; ++j) {
        const StatsAcc& a = h_res[j];
        qoimi_pixel_stat& o = stats_out[j];
        memset(&o, 0, sizeof(o));
        o.pixels = (unsigned long long)regions[j].width * regions[j].height;
        for (int k = 0; k < 4; ++k) { o.sum[k] = a.sum[k]; o.sum_sq[k] = a.sum_sq[k]; o.min[k] = (unsigned char)a.mn[k]; o.max[k] = (unsigned char)a.mx[k]; }
        o.first = a.first; o.flags = stats_flags(a, o.pixels);
        o.opaque_pixels = a.opaque; o.transparent_pixels = a.transparent; o.grey_pixels = a.grey;
    }
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// synthetic frames
// ------------------------------------------------------------------------------------
extern "C" int qoimi_synth_frames(qoimi_ctx* c, int kind, unsigned seed, unsigned first_frame,
                                  int n_frames, unsigned width, unsigned height,
                                  void* d_pixels, size_t pixel_stride, void* stream) {
    if (!c || !d_pixels || n_frames <= 0 || kind < 0 || kind > 5 || width == 0 || height == 0)
        return fail(QOIMI_E_ARG, "bad argument");
    const size_t npx = (size_t)width * height;
    if (npx >= kPixelCap || pixel_stride < npx * 4 || n_frames > 65535) return fail(QOIMI_E_ARG, "bad frame geometry");
    DeviceGuard guard(c->device);
    SynthParams p;
    p.pixels = (uint8_t*)d_pixels; p.pixel_stride = pixel_stride; p.npx = (uint32_t)npx; p.width = width;
    p.n_frames = (uint32_t)n_frames; p.first_frame = first_frame; p.seed = seed; p.kind = kind;
    launch_synth(p, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

extern "C" int qoimi_hash_streams(qoimi_ctx* c, const void* d_streams, size_t stream_stride, const int* d_stream_len, int n_streams,
                                  unsigned long long* d_hash, void* stream) {
    if (!c || !d_streams || !d_stream_len || !d_hash || n_streams <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    DeviceGuard guard(c->device);
    launch_hash_streams((const uint8_t*)d_streams, stream_stride, d_stream_len, (uint32_t)n_streams, (u64*)d_hash, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// Part 1 — drop-in entry points on host pointers
// ------------------------------------------------------------------------------------
// One context per CALLING THREAD (qoi.h:339,357-362,489-495: the reference keeps no state between calls and is callable
// from any number of threads at once).  Round 1 serialised every call on one global context behind a mutex; now a thread's
// calls run on its own context - own workspace, own non-blocking stream - so concurrent callers overlap their copies and
// kernels on the GPU.  A thread's context goes away with the thread.
// A fresh malloc of tens of megabytes is untouched address space: the copy back from the device would take a page fault every
// 4 KiB (2 ms of a 2.6 ms qoi_decode of a 4K frame, bench.py "dropin_host_pointers").  Ask for huge pages and have the range
// populated in one call instead; where the kernel knows neither, nothing is lost.
static void prefault_pages(void* p, size_t n) {
    if (n < ((size_t)1 << 20)) return;
    const uintptr_t a = ((uintptr_t)p + 4095u) & ~(uintptr_t)4095u, e = ((uintptr_t)p + n) & ~(uintptr_t)4095u;
    if (e <= a) return;
#ifdef MADV_HUGEPAGE
    (void)madvise((void*)a, e - a, MADV_HUGEPAGE);
#endif
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
    (void)madvise((void*)a, e - a, MADV_POPULATE_WRITE);
}

// The helpers that populate qoi_decode's result pages while the stream goes in and the kernels run: TWO parked threads per
// calling thread, started at its first large decode and woken per call (round 2 created and joined two std::threads in every
// call).  Per 4K frame: no populate 2.6 ms, one thread 1.95, two 1.61, three 2.4, four 2.5 - they contend for the address-space lock.
class Prefaulter {
    static constexpr int kThreads = 2;
    std::thread th[kThreads];
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    void* ptr[kThreads] = {nullptr, nullptr};
    size_t len[kThreads] = {0, 0};
    unsigned long long ticket[kThreads] = {0, 0}, done[kThreads] = {0, 0};
    bool started = false, quit = false, no_helpers = false;
    void loop(int i) {
        unsigned long long seen = 0;
        for (;;) {
            void* p; size_t n;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return quit || ticket[i] != seen; });
                if (quit) return;
                seen = ticket[i]; p = ptr[i]; n = len[i];
            }
            prefault_pages(p, n);
            { std::lock_guard<std::mutex> lk(mu); done[i] = seen; }
            cv_done.notify_all();
        }
    }
public:
    // populate [p, p + n) in the background; wait() returns when it is done
    void start(void* p, size_t n) {
        if (!started) {
            if (no_helpers) { prefault_pages(p, n); return; }
            int made = 0;
            try { for (; made < kThreads; ++made) th[made] = std::thread(&Prefaulter::loop, this, made); started = true; }
            catch (...) {
                // no threads to be had: the ones that did start are told to quit and joined, the state stays "no helpers" for good
                // (a second attempt would assign to a joinable std::thread), and this call populates here
                { std::lock_guard<std::mutex> lk(mu); quit = true; }
                cv_work.notify_all();
                for (int i = 0; i < made; ++i) if (th[i].joinable()) th[i].join();
                no_helpers = true;
                prefault_pages(p, n);
                return;
            }
        }
        const size_t part = ((n / kThreads) + 4095u) & ~(size_t)4095u;
        std::lock_guard<std::mutex> lk(mu);
        for (int i = 0; i < kThreads; ++i) {
            const size_t lo = (size_t)i * part;
            ptr[i] = (uint8_t*)p + (lo < n ? lo : n);
            len[i] = lo >= n ? 0 : ((i == kThreads - 1 || lo + part > n) ? n - lo : part);
            ++ticket[i];
        }
        cv_work.notify_all();
    }
    void wait() {
        if (!started) return;
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { for (int i = 0; i < kThreads; ++i) if (done[i] != ticket[i]) return false; return true; });
    }
    ~Prefaulter() {
        if (!started) return;
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv_work.notify_all();
        for (auto& t : th) if (t.joinable()) t.join();
    }
};

struct ThreadCtx {
    qoimi_ctx* c = nullptr;
    bool tried = false;
    Prefaulter pf;
    ~ThreadCtx() { if (c) qoimi_ctx_destroy(c); }
};
static thread_local ThreadCtx t_ctx;
static std::mutex g_mutex;                 // guards the one-time warning only

static qoimi_ctx* thread_ctx() {
    if (!t_ctx.c && !t_ctx.tried) {
        t_ctx.tried = true;
        int dev = 0;
        if (const char* e = getenv("QOIMI_DEVICE")) dev = atoi(e);
        if (qoimi_ctx_create(dev, &t_ctx.c) != QOIMI_OK) {
            std::lock_guard<std::mutex> lock(g_mutex);
            fprintf(stderr, "qoi_mi355x: no usable MI355X (%s); there is no CPU fallback\n", t_error.c_str());
            t_ctx.c = nullptr;
        } else t_ctx.c->dropin = true;
    }
    return t_ctx.c;
}

extern "C" void* qoi_encode(const void* data, const qoi_desc* desc, int* out_len) {
    if (!data || !out_len || !desc_ok(desc)) return NULL;                 // qoi.h:364-372
    qoimi_ctx* c = thread_ctx();
    if (!c) return NULL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->own_stream;
    const size_t npx = (size_t)desc->width * desc->height;
    const size_t in_bytes = npx * desc->channels;
    const size_t bound = qoimi_encode_bound(desc);                        // qoi.h:374-376
    if (c->io_a.reserve(in_bytes + 16) || c->io_b.reserve(bound + 16) || c->io_c.reserve(256)) return NULL;
    void* result = NULL;
    // The result is the reference's allocation (qoi.h:374-379: the worst case, w * h * (channels + 1) + 22 bytes) - a caller written
    // against the reference may count on that capacity.  Only the pages the stream will touch are populated (by the thread's parked
    // helpers, while the pixels go in and the kernels run); the rest of the allocation stays untouched address space.  What it costs:
    // a 4K frame's worst case is 39.6 MiB, above the 32 MiB ceiling of glibc's dynamic mmap threshold, so every call maps fresh
    // zero-filled pages and the caller's free() unmaps them (qoibench's encode-free loop, qoibench.c:446-449: 1.7 ms per call
    // against 0.84 with the tight buffer, profiles/r06_s1_dropin_worst_case.txt).  QOIMI_ENCODE_TIGHT_BUFFER=1 (opt-in, read when the
    // thread's context is created) sizes the buffer by this thread's previous stream instead (+ 1/8; a third of the bound at first; an
    // exact buffer in the rare case the stream turns out longer): it comes back from the allocator's heap with its pages in place.
    const bool worst_case = !c->tight_buffer;
    const size_t guess = worst_case ? bound : (c->last_drop_len ? c->last_drop_len + c->last_drop_len / 8u : bound / 3u);
    size_t ahead = guess < bound ? guess : bound;
    if (ahead < (size_t)kHeaderBytes + kTrailerBytes) ahead = (size_t)kHeaderBytes + kTrailerBytes;
    uint8_t* bytes = (uint8_t*)malloc(ahead);
    if (!bytes) return NULL;
    // The result's pages are populated by the thread's parked helpers WHILE the pixels go in and the kernels run (round 2
    // populated after the kernels: 0.35 ms of a 1.3 ms call).
    const size_t expect = worst_case ? (c->last_drop_len ? c->last_drop_len + c->last_drop_len / 8u : bound / 3u) : ahead;   // pages the stream will touch
    const bool populate = expect >= ((size_t)1 << 20);
    if (populate) t_ctx.pf.start(bytes, expect < ahead ? expect : ahead);
    do {
        // pixels in (the copy engine reads pageable memory at the link's rate on this platform, tools/ubench/host_copy.cpp),
        // kernels, then ONE read-back of length + liveness flag through pinned words, then exactly `len` bytes out
        if (hipMemcpyAsync(c->io_a.base, data, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) break;
        // A placement that waits on other sets (tree, look-back) bounds its spins; should that bound ever trip - never observed - the
        // image is encoded once more by the order-free form, in which no set waits for another.
        bool sound = false;
        for (int attempt = 0; attempt < 2 && !sound; ++attempt) {
            const int forced = c->enc_lookback;
            if (attempt) c->enc_lookback = 0;
            const int rc = qoimi_encode_batch(c, c->io_a.base, in_bytes, desc, 1, c->io_b.base, bound, (int*)c->io_c.base, st);
            c->enc_lookback = forced;
            if (rc != QOIMI_OK) break;
            if (hipMemcpyAsync(&c->host_word[4], c->io_c.base, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) break;
            if (hipMemcpyAsync(&c->host_word[5], c->last_enc_err, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess) break;
            if (hipStreamSynchronize(st) != hipSuccess) break;
            sound = c->host_word[5] == 0;
        }
        const int len = (int)c->host_word[4];
        if (!sound || len < kHeaderBytes + kTrailerBytes || (size_t)len > bound) {
            t_error = "encode kernel reported a liveness failure";
            break;
        }
        if (populate) { t_ctx.pf.wait(); }
        if ((size_t)len > ahead) {                                      // longer than expected: an exact buffer instead
            free(bytes);
            bytes = (uint8_t*)malloc((size_t)len);
            if (!bytes) return NULL;
            prefault_pages(bytes, (size_t)len);
        }
        if (hipMemcpyAsync(bytes, c->io_b.base, (size_t)len, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) break;
        c->last_drop_len = (size_t)len;
        *out_len = len;
        result = bytes;
    } while (0);
    if (!result) { if (populate) t_ctx.pf.wait(); free(bytes); }
    return result;
}

extern "C" void* qoi_decode(const void* data, int size, qoi_desc* desc, int channels) {
    if (!data || !desc || (channels != 0 && channels != 3 && channels != 4) ||
        size < kHeaderBytes + kTrailerBytes) return NULL;                 // qoi.h:497-503
    const uint8_t* bytes = (const uint8_t*)data;
    if (!parse_header(bytes, desc)) return NULL;                          // desc filled before validation, qoi.h:507-521
    const int och = channels ? channels : desc->channels;                 // qoi.h:523-525
    const size_t out_bytes = (size_t)desc->width * desc->height * (size_t)och;

    qoimi_ctx* c = thread_ctx();
    if (!c) return NULL;
    DeviceGuard guard(c->device);
    hipStream_t st = c->own_stream;
    if (c->io_a.reserve((size_t)size + 16) || c->io_b.reserve(out_bytes + 16)) return NULL;
    uint8_t* pixels = (uint8_t*)malloc(out_bytes);                        // qoi.h:527-531
    if (!pixels) return NULL;
    // The pages of the result are populated by the calling thread's two parked helpers while the stream goes in and the
    // kernels run (33 MB take one thread ~1.2 ms - the kernel zeroes them); the two copies alone take 0.79 ms (bench.py
    // dropin_host_pointers).  (Copying back in 4 MiB parts behind the populating threads instead of after them: 4.2 ms -
    // every pageable copy pins its pages under the same lock the populating threads hold.)
    const bool populate = out_bytes >= ((size_t)4 << 20);
    if (populate) t_ctx.pf.start(pixels, out_bytes);
    bool ok = hipMemcpyAsync(c->io_a.base, data, (size_t)size, hipMemcpyHostToDevice, st) == hipSuccess &&
              qoimi_decode_batch(c, c->io_a.base, (size_t)size, &size, desc, 1, channels, c->io_b.base, out_bytes, st) == QOIMI_OK;
    if (populate) t_ctx.pf.wait();
    ok = ok && hipMemcpyAsync(pixels, c->io_b.base, out_bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
    if (!ok) { free(pixels); return NULL; }
    return pixels;
}

// stdio wrappers, same observable behaviour as qoi.h:595-646.  Like the reference (qoi.h:51-58,592: QOI_NO_STDIO), a build with
// -DQOI_NO_STDIO leaves them out (make -C qoi_amd/csrc NO_STDIO=1 -> libqoi_mi355x_nostdio.so).
#ifndef QOI_NO_STDIO
extern "C" int qoi_write(const char* filename, const void* data, const qoi_desc* desc) {
    FILE* f = fopen(filename, "wb");
    if (!f) return 0;
    int size = 0;
    void* encoded = qoi_encode(data, desc, &size);
    if (!encoded) { fclose(f); return 0; }
    fwrite(encoded, 1, (size_t)size, f);
    fflush(f);
    const int err = ferror(f);
    fclose(f);
    free(encoded);
    return err ? 0 : size;
}

extern "C" void* qoi_read(const char* filename, qoi_desc* desc, int channels) {
    FILE* f = fopen(filename, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    if (size <= 0 || size > 0x7FFFFFFFL || fseek(f, 0, SEEK_SET) != 0) { fclose(f); return NULL; }
    void* data = malloc((size_t)size);
    if (!data) { fclose(f); return NULL; }
    const size_t got = fread(data, 1, (size_t)size, f);
    fclose(f);
    void* pixels = (got != (size_t)size) ? NULL : qoi_decode(data, (int)got, desc, channels);
    free(data);
    return pixels;
}
#endif  // QOI_NO_STDIO

// qoi_host.hip — C-ABI shim of libqoi_mi355x.so (include/qoi_mi355x.h): errors, the context, profiling, the getters, and Part 1.
//
// Part 1 (at the end of this file) mirrors the reference's public functions (qoi.h:252,265,278,289): identical
// argument validation, malloc()-owned results, NULL / 0 on failure; it creates a context per calling thread.  Part 2 is the
// additive device-resident batch API, one file per family of calls: qoi_host_encode.hip, qoi_host_decode.hip, qoi_host_pack.hip,
// qoi_host_staged.hip, qoi_host_seek.hip; what they share is qoi_ctx.h.  There is NO CPU codec in this library: every
// pixel/stream byte is produced by the gfx950 kernels, and all entry points fail when
// no GPU is usable.  Every look at the environment happens in this file, where contexts are created.
#include "qoi_ctx.h"

#include <sys/mman.h>

#include <condition_variable>
#include <mutex>
#include <thread>

// ------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------
static thread_local std::string t_error;
int qoimi::fail(int code, const std::string& msg) { t_error = msg; return code; }

extern "C" const char* qoimi_last_error(void) { return t_error.c_str(); }

extern "C" const char* qoimi_version(void) { return "qoi_mi355x 0.1 gfx950"; }

// ------------------------------------------------------------------------------------
// context: device + growable workspace arenas (qoi_ctx.h)
// ------------------------------------------------------------------------------------
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
    c->enc_ws.release(); c->enc_stage.release(); c->dec_ws.release(); c->insp_ws.release(); c->cmp_ws.release(); c->ver_stage.release(); c->band_arena.release(); c->dec_scan.release(); c->io_a.release(); c->io_b.release(); c->io_c.release();
    if (c->host_word) (void)hipHostFree(c->host_word);
    c->pin.release(); c->enc_pin.release(); c->cmp_pin.release();
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

// device memory the context holds: [0] encode workspace (and the staging of qoimi_encode_packed and qoimi_encode_tiles), [1] decode workspace (and the tables of
// qoimi_inspect_streams, the tables and the staging of qoimi_compare_images / qoimi_verify_images / qoimi_decode_thumbnails / qoimi_decode_crops / qoimi_decode_resized, the band arena of qoimi_decode_crops_indexed), [2] staging of the
// host-pointer entry points
extern "C" void qoimi_workspace_bytes(qoimi_ctx* c, size_t out[3]) {
    out[0] = c ? c->enc_ws.cap + c->enc_stage.cap : 0; out[1] = c ? c->dec_ws.cap + c->insp_ws.cap + c->cmp_ws.cap + c->ver_stage.cap + c->band_arena.cap : 0;
    out[2] = c ? c->io_a.cap + c->io_b.cap + c->io_c.cap : 0;
}

extern "C" void qoimi_decode_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->dec_stats : nullptr, out); }
extern "C" void qoimi_thumbnail_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->thumb_stats : nullptr, out); }
extern "C" void qoimi_crop_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->crop_stats : nullptr, out); }
extern "C" void qoimi_resize_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->resize_stats : nullptr, out); }
extern "C" void qoimi_bilinear_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->bilinear_stats : nullptr, out); }
extern "C" void qoimi_warp_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->warp_stats : nullptr, out); }
extern "C" void qoimi_tensor_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->tensor_stats : nullptr, out); }
extern "C" void qoimi_pixel_stats_counters(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->pixel_stats : nullptr, out); }
extern "C" void qoimi_seek_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->seek_stats : nullptr, out); }
extern "C" void qoimi_tile_stats(qoimi_ctx* c, long long out[4]) { copy_stats(c ? c->tile_stats : nullptr, out); }

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
            fprintf(stderr, "qoi_mi355x: no usable MI355X (%s); there is no CPU fallback\n", qoimi_last_error());
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
            (void)fail(QOIMI_E_INTERNAL, "encode kernel reported a liveness failure");
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

// qoi_host_staged.hip — the calls of the C-ABI shim that decode a pack's images into bounded staging and run one table-driven kernel over
// each sub-batch: qoimi_verify_images (and qoimi_compare_images, whose kernels it runs), qoimi_decode_thumbnails, qoimi_decode_crops,
// qoimi_decode_resized, qoimi_decode_bilinear, qoimi_pixel_stats, and the row seek index (qoimi_build_seek_index, qoimi_seek_index_from_pixels - which stages nothing;
// one kernel pair, seekpx_last + seekpx_carry, serves both builds: over the staging arena and over the caller's pixels -,
// qoimi_make_band_streams, qoimi_decode_crops_indexed, qoimi_decode_resized_indexed, qoimi_decode_bilinear_indexed,
// qoimi_pixel_stats_indexed).
#include "qoi_ctx.h"
#include "qoi_thumb_core.h"
#include "qoi_crop_core.h"
#include "qoi_resize_core.h"
#include "qoi_bilinear_core.h"
#include "qoi_stats_core.h"
#include "qoi_seek_core.h"

#include <stddef.h>

// ------------------------------------------------------------------------------------
// images against images, streams against their pixels (qoi_compare.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_image_diff) == sizeof(CmpDiff) && offsetof(qoimi_image_diff, first) == 8 && offsetof(qoimi_image_diff, want) == 16 &&
              offsetof(qoimi_image_diff, got) == 20 && offsetof(qoimi_image_diff, flags) == 24 && offsetof(qoimi_image_diff, reserved) == 28,
              "qoimi_image_diff is what cmp_pixels and cmp_first write");
static_assert(QOIMI_DIFF_PIXELS == 1, "cmp_first writes the flag as a number");

// Fills entry `e` for an image of npx pixels and returns the tiles it takes.
static uint32_t cmp_entry(CmpImage* e, size_t a_off, size_t b_off, size_t npx, uint32_t first_tile, unsigned ca, unsigned cb, unsigned ra, unsigned rb, uint32_t index) {
    e->a_off = (u64)a_off; e->b_off = (u64)b_off; e->npx = (uint32_t)npx; e->first_tile = first_tile;
    e->chan = ca | (cb << 8) | (ra << 16) | (rb << 24); e->index = index;
    return (uint32_t)((npx + kCmpTilePx - 1u) / kCmpTilePx);
}

// The two kernels over table entries [from, from + m) of the device table (their tiles begin at 0).  With per-kernel timing on, the stream is
// waited for and the events are folded at once: the interval of a launch that follows must not begin at this one's first event.
static int compare_launch(qoimi_ctx* c, const void* d_a, const void* d_b, const CmpImage* d_tab, uint32_t m, uint32_t tiles, CmpDiff* d_diffs, hipStream_t st) {
    if (const int rc = timer_room(c, st)) return rc;
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
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    // pinned staging: [image table][results as they start] go to the device in one copy, [results] come back
    const size_t tab_bytes = up256(n * sizeof(CmpImage)), res_bytes = up256(n * sizeof(CmpDiff));
    { const int rc = c->cmp_pin.reserve(tab_bytes + 2u * res_bytes); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(tab_bytes + res_bytes); if (rc != QOIMI_OK) return rc; }
    uint8_t* pin = (uint8_t*)c->cmp_pin.buf;
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
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    // pinned staging: [image table][results as they start] go to the device in one copy, [results] come back; [offsets][header bytes] are
    // read and written in place by gather_headers
    const size_t tab_bytes = up256(n * sizeof(CmpImage)), res_bytes = up256(n * sizeof(CmpDiff)), off_bytes = up256(n * sizeof(u64));
    { const int rc = c->cmp_pin.reserve(tab_bytes + 2u * res_bytes + off_bytes + n * 16u); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(tab_bytes + res_bytes); if (rc != QOIMI_OK) return rc; }
    { const int rc = reserve_exact(c->ver_stage, need); if (rc != QOIMI_OK) return rc; }
    uint8_t* pin = (uint8_t*)c->cmp_pin.buf;
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
// decode through staging, then one table-driven kernel per sub-batch: what qoimi_decode_thumbnails, qoimi_decode_crops,
// qoimi_decode_resized and qoimi_decode_bilinear share (their plans: qoi_stage_plan.h)
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

// The items of qoimi_decode_crops (`noun` "crop"), of qoimi_decode_resized and qoimi_decode_bilinear ("item") and of qoimi_pixel_stats ("region"), looked at in the order
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
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    const size_t tab_bytes = staged_extra_at(n, sizeof(Entry));
    { const int rc = c->cmp_pin.reserve(tab_bytes + extra); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(tab_bytes + extra); if (rc != QOIMI_OK) return rc; }
    { const int rc = reserve_exact(c->ver_stage, plan.need); if (rc != QOIMI_OK) return rc; }
    Entry* h_tab = (Entry*)c->cmp_pin.buf;
    for (size_t e = 0; e < n; ++e) fill(h_tab[e], e);
    const Entry* d_tab = (const Entry*)c->cmp_ws.base;
    if (extra != 0u) { const int rc = begin((uint8_t*)c->cmp_pin.buf + tab_bytes, st); if (rc != QOIMI_OK) return rc; }
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
    if (extra != 0u) HIP_TRY(hipMemcpyAsync((uint8_t*)c->cmp_pin.buf + tab_bytes, (const uint8_t*)c->cmp_ws.base + tab_bytes, extra, hipMemcpyDeviceToHost, st));
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
// rectangles of a pack's images resampled by the antialiased bilinear filter (qoi_bilinear.hip)
// ------------------------------------------------------------------------------------
// nullptr if the item is fine for an accepted descriptor, else what is wrong with it: the checks of resize_item_wrong with the ratio limit of
// 32 and the product limit (qoi_bilinear_core.h: what keeps a weight in 32 bits and the sums in 64)
static const char* bilinear_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (r->width == 0u || r->height == 0u || r->out_width == 0u || r->out_height == 0u) return "zero width or height";
    if ((r->flags & ~(unsigned)(QOIMI_RESIZE_FLIP_X | QOIMI_RESIZE_FLIP_Y)) != 0u) return "unknown flag bit";
    if ((uint64_t)r->x + r->width > d->width || (uint64_t)r->y + r->height > d->height) return "the rectangle leaves its image";
    if (r->width > (uint64_t)kBilinearMaxRatio * r->out_width || r->height > (uint64_t)kBilinearMaxRatio * r->out_height) return "reduced by more than 32 in an axis";
    const uint64_t mx = r->width > r->out_width ? r->width : r->out_width, my = r->height > r->out_height ? r->height : r->out_height;
    if (mx * my >= kBilinearMaxArea) return "max(width, out_width) * max(height, out_height) is 2^30 or more";
    return nullptr;
}

extern "C" size_t qoimi_bilinear_size(const qoi_desc* desc, const qoimi_resize* item, int channels) {
    size_t bytes = 0;
    if (!desc_ok(desc) || !item || (channels != 3 && channels != 4) || bilinear_item_wrong(desc, item) || !resize_bytes(item, (unsigned)channels, &bytes)) return 0;
    return bytes;
}

// The plan of qoimi_decode_crops over the items' rectangles (qoi_amd/bilinear.py: plan); run_staged with one launch of bilinear_filter over the
// sub-batch's items.
extern "C" int qoimi_decode_bilinear(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                     int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                     size_t staging_bytes, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    if (mode != QOIMI_RESIZE_PLAIN && mode != QOIMI_RESIZE_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_RESIZE_PLAIN or QOIMI_RESIZE_ALPHA_WEIGHTED");
    const size_t n = (size_t)n_items;
    CheckedItems ok;
    if (const int rc = check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, bilinear_item_wrong, resize_bytes, ok)) return rc;
    const unsigned och = ok.och;
    const RowsPlan plan = plan_rows(descs, n_images, ok.rows, staging_bytes);
    std::vector<uint32_t> image_of(n);
    std::vector<uint64_t> tiles_of(n);
    for (size_t j = 0; j < n; ++j) { image_of[j] = items[j].image; tiles_of[j] = bilinear_tiles(items[j].width, items[j].out_width, items[j].out_height); }
    const ItemPlan order = plan_items(image_of, plan.ref_of, plan.firsts, tiles_of);
    if (order.overflow) return fail(QOIMI_E_ARG, "more than 2^31 tiles of output pixels in one sub-batch");
    const uint32_t weighted = (mode == QOIMI_RESIZE_ALPHA_WEIGHTED && och == 4u) ? 1u : 0u;   // with 3 output channels the mode is PLAIN
    return run_staged<ResizeEntry>(c, c->bilinear_stats, (long long)plan.refs.size(), "bilinear_filter", d_streams, stream_offsets, sizes, descs, plan, ok.rows, order,
        [&](ResizeEntry& t, size_t e) {
            const size_t j = order.by_ref[e];
            const qoimi_resize& r = items[j];
            uint32_t lg, cols;
            bilinear_split(r.width, r.out_width, lg, cols);
            t.src_off = (u64)plan.at[(size_t)plan.ref_of[r.image]]; t.dst_off = (u64)out_offsets[j];
            t.w = descs[r.image].width; t.x = r.x; t.y = r.y; t.cw = r.width; t.rh = r.height; t.ow = r.out_width; t.oh = r.out_height;
            t.first_tile = order.first_tile[e]; t.cfg = lg | (cols << 8) | (och << 16) | (weighted << 24) | (r.flags << 28); t.reserved = 0u;
        },
        [&](const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            launch_bilinear((const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, grid, st);
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
    const StatsAcc* h_res = (const StatsAcc*)((const uint8_t*)c->cmp_pin.buf + res_at);
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
// the row seek index (qoi_seek.hip; qoi_amd/seekindex.py states all of it)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_seek_point) == sizeof(SeekPoint) && offsetof(qoimi_seek_point, skip) == 4 && offsetof(qoimi_seek_point, prev) == 8 &&
              offsetof(qoimi_seek_point, table) == 16, "qoimi_seek_point is what seekpx_carry writes");
static_assert(sizeof(qoimi_band) == 16 && sizeof(qoimi_band_info) == 24 && offsetof(qoimi_band_info, desc) == 8 && offsetof(qoimi_band_info, pad_rows) == 20,
              "qoimi_band / qoimi_band_info layout");

extern "C" int qoimi_seek_points(const qoi_desc* desc, unsigned interval_rows) {
    if (!desc_ok(desc)) return -1;
    return (int)seek_point_count(desc->width, desc->height, interval_rows);
}

// What the two builds of an index share.  SeekCount: what seek_count makes of a call's images - np[i] points of image i from point_base[i]
// on, refs: the images that have a point, ascending, ref_tiles: the tiles of kSeekTilePx pixels each of them takes; total points; tiles of all
// of refs, blocks and pieces of the inspect passes over refs.
struct SeekCount { std::vector<uint32_t> np, point_base; std::vector<size_t> refs; std::vector<uint64_t> ref_tiles; uint64_t total = 0, tiles = 0; size_t nb = 0, npieces = 0; };

// Fills the entry of an image with np >= 1 points whose pixels stand at `off` of a pixel buffer, ch bytes each, and returns the tiles it takes.
// (interval_rows * w is below 400 000 000: a point lies inside the image.)
static uint32_t seekpx_entry(SeekPxImage& e, size_t off, uint32_t ch, uint32_t interval_rows, uint32_t w, uint32_t np, uint32_t point_base, uint32_t first_tile) {
    e.src_off = (u64)off; e.ipx = interval_rows * w; e.np = np; e.tpi = seek_interval_tiles(e.ipx);
    e.first_tile = first_tile; e.point_base = point_base; e.ch = ch;
    return np * e.tpi;
}

// The checks both builds make per image, in the order that decides which message a call with several faults gets; more(i): nullptr, or what
// else is wrong with image i.
template <class More>
static int seek_count(const int* sizes, const qoi_desc* descs, size_t n, const unsigned* interval_rows, More more, SeekCount& k) {
    const int kMin = kHeaderBytes + kTrailerBytes;
    k.np.resize(n); k.point_base.resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] < kMin) return fail(QOIMI_E_ARG, "stream " + std::to_string(i) + " shorter than 22 bytes (qoi.h:500)");
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(i) + " rejected (qoi.h:513-521 rules)");
        const int64_t cnt = seek_point_count(descs[i].width, descs[i].height, interval_rows[i]);
        if (cnt < 0) return fail(QOIMI_E_ARG, "image " + std::to_string(i) + ": interval_rows * width below 128");
        if (const char* what = more(i)) return fail(QOIMI_E_ARG, "image " + std::to_string(i) + ": " + what);
        k.np[i] = (uint32_t)cnt; k.point_base[i] = (uint32_t)k.total;
        k.total += (uint64_t)cnt;
        if (cnt == 0) continue;
        k.refs.push_back(i);
        k.ref_tiles.push_back((uint64_t)cnt * seek_interval_tiles(interval_rows[i] * descs[i].width));   // (a point lies inside the image: 32 bits)
        k.tiles += k.ref_tiles.back();
        const size_t body = (size_t)(sizes[i] - kMin);
        k.nb += (body + kInsBlock - 1u) / kInsBlock;
        k.npieces += (body + kInsPiece - 1u) / kInsPiece;
    }
    if (k.total >= 0x7FFFFFFFull / 64u) return fail(QOIMI_E_ARG, "more than 2^25 seek points in one call");
    if (k.nb >= 0x7FFFFFFFu || k.npieces >= 0xFFFFFFFFu) return fail(QOIMI_E_ARG, "more than 2^31 blocks of stream bytes in one call");
    return QOIMI_OK;
}

// byte_off and skip of every point (k.total >= 1): one qoimi_inspect_streams over the images that have a point, the block scan and a
// wavefront per point on top of its tables, enqueued on st and NOT waited for.  Pinned staging (c->pin): [stream table][block table][jobs]
// [extra_bytes of the caller's: fill(those bytes) writes them] go to the device in one copy, [results][header + trailer bytes] are written by
// inspect_reduce in place (and not looked at), [room for the points, if with_points].  The workspace is carved the same way: d_extra is the
// caller's table on the device, d_loc what seek_locate finds, d_last a zeroed uint32[64] per point, d_points (with_points) room for the points.
struct SeekLocated { const uint8_t* d_extra; SeekLoc* d_loc; uint32_t* d_last; SeekPoint* d_points; uint8_t* h_points; };

template <class Fill>
static int locate_points(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                         const unsigned* interval_rows, const SeekCount& k, size_t extra_bytes, Fill fill, bool with_points, void* stream, SeekLocated& out) {
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    if (const int rc = timer_room(c, st)) return rc;
    const size_t R = k.refs.size(), nb = k.nb, npieces = k.npieces, total = (size_t)k.total;
    const size_t tab_bytes = up256(R * sizeof(InsStream)) + up256(nb * sizeof(InsBlock)), job_bytes = up256(total * sizeof(SeekJob));
    const size_t in_bytes = tab_bytes + job_bytes + up256(extra_bytes);
    const size_t res_at = in_bytes, raw_at = res_at + up256(R * sizeof(InsResult)), pts_at = raw_at + up256(R * 32u);
    if (const int rc = c->pin.reserve(pts_at + (with_points ? total * sizeof(SeekPoint) : 0u))) return rc;
    uint8_t* pin = (uint8_t*)c->pin.buf;
    InsStream* h_tab = (InsStream*)pin;
    InsBlock* h_blk = (InsBlock*)(pin + up256(R * sizeof(InsStream)));
    SeekJob* h_job = (SeekJob*)(pin + tab_bytes);
    std::vector<size_t> so(R); std::vector<int> sz(R);
    for (size_t r = 0; r < R; ++r) { so[r] = stream_offsets[k.refs[r]]; sz[r] = sizes[k.refs[r]]; }
    ins_fill_tables(so.data(), sz.data(), R, h_tab, h_blk);
    for (size_t r = 0; r < R; ++r) {
        const size_t i = k.refs[r];
        const uint32_t ipx = interval_rows[i] * descs[i].width;          // (below 400 000 000: a point lies inside the image)
        for (uint32_t p = 0; p < k.np[i]; ++p) { SeekJob& j = h_job[k.point_base[i] + p]; j.stream = (uint32_t)r; j.point = k.point_base[i] + p; j.P = (p + 1u) * ipx; j.reserved = 0u; }
    }
    fill(pin + tab_bytes + job_bytes);
    Carver sizer(nullptr);
    sizer.take<uint8_t>(in_bytes); sizer.take<uint32_t>(nb); sizer.take<uint8_t>(nb); sizer.take<uint16_t>(npieces); sizer.take<InsPartial>(nb);
    sizer.take<u64>(nb); sizer.take<SeekLoc>(total); sizer.take<uint32_t>(total * 64u);
    if (with_points) sizer.take<SeekPoint>(total);
    { const int rc = c->insp_ws.reserve(sizer.off + 256u); if (rc != QOIMI_OK) return rc; }
    Carver cv(c->insp_ws.base);
    uint8_t* d_tab = cv.take<uint8_t>(in_bytes);
    uint32_t* d_map = cv.take<uint32_t>(nb);
    uint8_t* d_entry = cv.take<uint8_t>(nb);
    uint16_t* d_piece = cv.take<uint16_t>(npieces);
    InsPartial* d_part = cv.take<InsPartial>(nb);
    u64* d_blk_px = cv.take<u64>(nb);
    out.d_loc = cv.take<SeekLoc>(total);
    out.d_last = cv.take<uint32_t>(total * 64u);
    out.d_points = with_points ? cv.take<SeekPoint>(total) : nullptr;
    out.d_extra = d_tab + tab_bytes + job_bytes;
    out.h_points = with_points ? pin + pts_at : nullptr;
    const InsBlock* d_blk = (const InsBlock*)(d_tab + up256(R * sizeof(InsStream)));
    HIP_TRY(hipMemcpyAsync(d_tab, pin, in_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(out.d_last, 0, total * 64u * sizeof(uint32_t), st));
    launch_inspect((const uint8_t*)d_streams, (const InsStream*)d_tab, (uint32_t)R, d_blk, (uint32_t)nb, d_map, d_entry, d_piece, d_part, (InsResult*)(pin + res_at),
                   (uint32_t*)(pin + raw_at), st, &c->timer);
    launch_seek_locate((const uint8_t*)d_streams, (const InsStream*)d_tab, (uint32_t)R, d_blk, d_part, d_entry, d_piece, d_blk_px,
                       (const SeekJob*)(d_tab + tab_bytes), (uint32_t)total, out.d_loc, st);
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

// locate_points (byte_off, skip); then run_staged over the images that have a point at their full height with seekpx_last + seekpx_carry
// over the staging arena per sub-batch (prev, table), which write the points behind the image table; one copy back.
extern "C" int qoimi_build_seek_index(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                      int n_images, const unsigned* interval_rows, qoimi_seek_point* points_out, size_t staging_bytes, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves points_out as it was)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !interval_rows || !points_out || n_images <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    const size_t n = (size_t)n_images;
    SeekCount k;
    if (const int rc = seek_count(sizes, descs, n, interval_rows, [](size_t) { return (const char*)nullptr; }, k)) return rc;
    const std::vector<uint32_t>& np = k.np; const std::vector<uint32_t>& point_base = k.point_base;
    const uint64_t total = k.total;
    std::vector<uint32_t> rows(n);
    for (size_t i = 0; i < n; ++i) rows[i] = np[i] != 0u ? descs[i].height : 0u;
    const RowsPlan plan = plan_rows(descs, n_images, rows, staging_bytes);   // (plan.refs is k.refs: the images that have a point)
    const size_t R = plan.refs.size();
    const std::vector<uint32_t> image_of(plan.refs.begin(), plan.refs.end());
    const ItemPlan items = plan_items(image_of, plan.ref_of, plan.firsts, k.ref_tiles);   // (entry r is the r-th image that has a point)
    if (items.overflow) return fail(QOIMI_E_ARG, "more than 2^31 tiles of pixels in one sub-batch");
    c->seek_stats[0] = 0;
    if (total == 0u) return QOIMI_OK;
    SeekLocated at;
    {
        DeviceGuard guard(c->device);
        if (const int rc = locate_points(c, d_streams, stream_offsets, sizes, descs, interval_rows, k, 0u, [](uint8_t*) {}, false, stream, at)) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));              // (the decode calls below reuse the pinned staging at once)
        if (c->timer.on) timer_collect(c);
    }
    SeekLoc* d_loc = at.d_loc; uint32_t* d_last = at.d_last;
    const size_t res_at = staged_extra_at(R, sizeof(SeekPxImage));
    long long stats[4];
    const int rc = run_staged<SeekPxImage>(c, stats, (long long)R, "seekpx_last", d_streams, stream_offsets, sizes, descs, plan, rows, items,
        [&](SeekPxImage& t, size_t e) {
            const size_t r = items.by_ref[e], i = (size_t)plan.refs[r];
            (void)seekpx_entry(t, plan.at[r], 4u, interval_rows[i], descs[i].width, np[i], point_base[i], items.first_tile[e]);
        },
        [&](const SeekPxImage* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            launch_seek_tables_px((const uint8_t*)c->ver_stage.base, tab, m, tiles, d_last, d_loc, (SeekPoint*)((uint8_t*)c->cmp_ws.base + res_at), grid, st);
        }, stream, (size_t)total * sizeof(SeekPoint),
        [&](uint8_t* h_points, hipStream_t) { memset(h_points, 0, (size_t)total * sizeof(SeekPoint)); return (int)QOIMI_OK; });
    c->seek_stats[0] = stats[0];
    if (rc != QOIMI_OK) return rc;
    memcpy(points_out, (const uint8_t*)c->cmp_pin.buf + res_at, (size_t)total * sizeof(SeekPoint));
    return QOIMI_OK;
}

// locate_points (byte_off, skip) and, in the same stream order, seekpx_last + seekpx_carry over the caller's pixels in ONE launch each (prev,
// table): no decode, no staging arena.  The image table travels with the inspect tables, the points are written on the device behind them
// and come back in one copy; one wait, at the end.
extern "C" int qoimi_seek_index_from_pixels(qoimi_ctx* c, const void* d_pixels, const size_t* pixel_offsets, const void* d_streams, const size_t* stream_offsets,
                                            const int* sizes, const qoi_desc* descs, int n_images, const unsigned* interval_rows, qoimi_seek_point* points_out,
                                            void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves points_out as it was)
    if (!c || !d_pixels || !pixel_offsets || !d_streams || !stream_offsets || !sizes || !descs || !interval_rows || !points_out || n_images <= 0)
        return fail(QOIMI_E_ARG, "NULL/empty argument");
    const uintptr_t room = ~(uintptr_t)0 - (uintptr_t)d_pixels;          // the last byte of an image may stand at the last address there is
    SeekCount k;
    if (const int rc = seek_count(sizes, descs, (size_t)n_images, interval_rows, [&](size_t i) {
            const size_t bytes = (size_t)descs[i].width * descs[i].height * descs[i].channels;
            return pixel_offsets[i] > room || bytes - 1u > room - pixel_offsets[i] ? "the address of its last byte does not fit in a pointer" : (const char*)nullptr;
        }, k)) return rc;
    if (k.tiles >= 0x7FFFFFFFull) return fail(QOIMI_E_ARG, "more than 2^31 tiles of pixels in one call");
    c->seek_stats[0] = 0;                                      // (no sub-batch is decoded)
    if (k.total == 0u) return QOIMI_OK;
    const size_t R = k.refs.size(), pts_bytes = (size_t)k.total * sizeof(SeekPoint);
    uint32_t t = 0;
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    SeekLocated at;
    if (const int rc = locate_points(c, d_streams, stream_offsets, sizes, descs, interval_rows, k, R * sizeof(SeekPxImage), [&](uint8_t* bytes) {
            SeekPxImage* h_img = (SeekPxImage*)bytes;
            for (size_t r = 0; r < R; ++r) {
                const size_t i = k.refs[r];
                t += seekpx_entry(h_img[r], pixel_offsets[i], descs[i].channels, interval_rows[i], descs[i].width, k.np[i], k.point_base[i], t);
            }
        }, true, stream, at)) return rc;
    const uint32_t most = (uint32_t)c->n_cus * 8u;
    launch_seek_tables_px((const uint8_t*)d_pixels, (const SeekPxImage*)at.d_extra, (uint32_t)R, t, at.d_last, at.d_loc, at.d_points, t < most ? t : most, st);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(QOIMI_E_INTERNAL, std::string("seekpx_last: ") + hipGetErrorString(e)); } }
    HIP_TRY(hipMemcpyAsync(at.h_points, at.d_points, pts_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->timer.on) timer_collect(c);
    memcpy(points_out, at.h_points, pts_bytes);
    return QOIMI_OK;
}

// A band as qoimi_band_plan sees it: what it will be, what stands in front of its tail, the point it starts at (nullptr: row 0) and its
// tail, the bytes [tail_lo, tail_lo + tail_len) of the stream.
struct BandPlan { qoimi_band_info info; SeekPrefix f; const qoimi_seek_point* e; uint32_t tail_lo, tail_len; };

// nullptr if the band is fine, else what is wrong with it
static const char* band_wrong(const qoi_desc* d, int size, unsigned K, const qoimi_seek_point* pts, const qoimi_band* b, BandPlan& out) {
    if (!desc_ok(d)) return "descriptor rejected (qoi.h:513-521 rules)";
    if (size < kHeaderBytes + kTrailerBytes) return "stream shorter than 22 bytes (qoi.h:500)";
    const int64_t np = seek_point_count(d->width, d->height, K);
    if (np < 0) return "interval_rows * width below 128";
    if (b->rows == 0u) return "an empty band";
    if ((uint64_t)b->first_row + b->rows > d->height) return "the band leaves its image";
    if (b->first_row % K != 0u) return "first_row is neither 0 nor a seek row";
    const uint64_t k2 = ((uint64_t)b->first_row + b->rows + K - 1u) / K - 1u;
    if ((b->first_row != 0u || k2 < (uint64_t)np) && !pts) return "no points";
    const qoimi_seek_point* e = b->first_row != 0u ? pts + (b->first_row / K - 1u) : nullptr;
    const qoimi_seek_point* e2 = k2 < (uint64_t)np ? pts + k2 : nullptr;
    for (const qoimi_seek_point* p : {e, e2})
        if (p && (p->byte_off < (unsigned)kHeaderBytes || p->byte_off > (unsigned)(size - kTrailerBytes) || p->skip > kSeekMaxSkip))
            return "a seek point with byte_off outside [14, size - 8] or skip above 61";
    const uint32_t lo = e ? e->byte_off : (uint32_t)kHeaderBytes;
    const uint32_t hi = e2 && e2->byte_off + 13u < (uint32_t)size ? e2->byte_off + 13u : (uint32_t)size;
    if (hi < lo) return "the seek points do not ascend";
    out.f = seek_prefix_plan((const SeekPoint*)e, d->width);
    // (a point of a stream holds prev in prev's own slot, so it has at most 64 loads; 64 table words that all differ from prev are no point)
    if (out.f.n > kSeekMaxLoads) return "a seek point with more than 64 loads (its table does not hold prev)";
    const uint64_t bytes = (uint64_t)seek_prefix_len(out.f) + (hi - lo);
    if (bytes >= 0x7FFFFFFFull) return "a band stream of 2^31 - 1 bytes or more";
    out.e = e; out.tail_lo = lo; out.tail_len = hi - lo;
    out.info.size = bytes; out.info.desc = *d; out.info.desc.height = out.f.pad_rows + b->rows; out.info.pad_rows = out.f.pad_rows;
    return nullptr;
}

extern "C" int qoimi_band_plan(const qoi_desc* desc, int size, unsigned interval_rows, const qoimi_seek_point* points, const qoimi_band* band,
                               qoimi_band_info* out) {
    if (!desc || !band || !out) return fail(QOIMI_E_ARG, "NULL argument");
    BandPlan p;
    if (const char* what = band_wrong(desc, size, interval_rows, points, band, p)) return fail(QOIMI_E_ARG, std::string("band: ") + what);
    *out = p.info;
    return QOIMI_OK;
}

// Band stream j of image image_of[j] at d_out + out_offsets[j]: the heads (header and loads) are written here and travel with the table, one
// launch of band_assemble writes everything; the stream is waited for (the pinned staging belongs to the next call at once).  The ranges have
// been checked.  Leaves the counters of qoimi_seek_stats [1] and [3].
static int assemble_bands(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const std::vector<BandPlan>& plans,
                          const std::vector<uint32_t>& image_of, void* d_out, const size_t* out_offsets, const std::vector<uint32_t>& first_tile,
                          uint32_t tiles, void* stream) {
    const size_t n = plans.size();
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    const size_t tab_bytes = up256(n * sizeof(BandEntry)), bytes = tab_bytes + n * kSeekHeadSlot;
    { const int rc = c->cmp_pin.reserve(bytes); if (rc != QOIMI_OK) return rc; }
    { const int rc = c->cmp_ws.reserve(bytes); if (rc != QOIMI_OK) return rc; }
    BandEntry* h_tab = (BandEntry*)c->cmp_pin.buf;
    uint8_t* h_heads = (uint8_t*)c->cmp_pin.buf + tab_bytes;
    long long copied = 0;
    for (size_t j = 0; j < n; ++j) {
        const BandPlan& p = plans[j];
        BandEntry& t = h_tab[j];
        t.src_off = (u64)stream_offsets[image_of[j]] + p.tail_lo; t.dst_off = (u64)out_offsets[j];
        t.B = (uint32_t)p.info.size; t.head_len = p.f.head_len; t.run_full = p.f.run_full; t.run_last = p.f.run_last;
        t.first_tile = first_tile[j]; t.head_at = (uint32_t)(j * kSeekHeadSlot); t.reserved[0] = 0u; t.reserved[1] = 0u;
        memset(h_heads + j * kSeekHeadSlot, 0, kSeekHeadSlot);
        seek_write_head((const SeekPoint*)p.e, p.info.desc.width, p.info.desc.height, p.info.desc.channels, p.info.desc.colorspace, h_heads + j * kSeekHeadSlot);
        copied += (long long)p.tail_len;
    }
    HIP_TRY(hipMemcpyAsync(c->cmp_ws.base, h_tab, bytes, hipMemcpyHostToDevice, st));
    const uint32_t most = (uint32_t)c->n_cus * 8u;
    launch_band_assemble((const uint8_t*)d_streams, (const BandEntry*)c->cmp_ws.base, (uint32_t)n, tiles, (const uint8_t*)c->cmp_ws.base + tab_bytes,
                         (uint8_t*)d_out, tiles < most ? tiles : most, st);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(QOIMI_E_INTERNAL, std::string("band_assemble: ") + hipGetErrorString(e)); } }
    HIP_TRY(hipStreamSynchronize(st));
    c->seek_stats[1] = (long long)n; c->seek_stats[3] = copied;
    return QOIMI_OK;
}

// The tiles of band streams of plans[j].info.size bytes at base + offsets[j]; false: 2^31 - 1 of them or more
static bool band_tiles(const std::vector<BandPlan>& plans, uintptr_t base, const size_t* offsets, std::vector<uint32_t>& first_tile, uint32_t& tiles) {
    uint64_t t = 0;
    first_tile.resize(plans.size());
    for (size_t j = 0; j < plans.size(); ++j) {
        if (t >= 0x7FFFFFFFull) return false;
        first_tile[j] = (uint32_t)t;
        t += crop_tiles((uint64_t)base + offsets[j], plans[j].info.size);
    }
    tiles = (uint32_t)t;
    return t < 0x7FFFFFFFull;
}

extern "C" int qoimi_make_band_streams(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                       int n_images, const unsigned* interval_rows, const qoimi_seek_point* points, const size_t* point_firsts,
                                       const qoimi_band* bands, int n_bands, void* d_out, const size_t* out_offsets, qoimi_band_info* infos_out, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !interval_rows || !points || !point_firsts || !bands || !d_out || !out_offsets ||
        n_images <= 0 || n_bands <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    const size_t n = (size_t)n_bands;
    if (n > 0xFFFFFFFFu / kSeekHeadSlot) return fail(QOIMI_E_ARG, "more than 12 782 640 bands in one call");     // (a head's place in the table is 32 bits)
    std::vector<BandPlan> plans(n);
    std::vector<uint32_t> image_of(n);
    std::vector<size_t> out_bytes(n);
    const uintptr_t room = ~(uintptr_t)0 - (uintptr_t)d_out;
    // [start, end) of every output (kind 1) and of every stream a band names (kind 0), as addresses: no output may meet anything
    struct Range { uintptr_t lo, hi; int out; };
    std::vector<Range> ranges;
    for (size_t j = 0; j < n; ++j) {
        const qoimi_band& b = bands[j];
        if (b.image >= (unsigned)n_images) return fail(QOIMI_E_ARG, "band " + std::to_string(j) + ": no image " + std::to_string(b.image));
        const size_t i = b.image;
        if (const char* what = band_wrong(&descs[i], sizes[i], interval_rows[i], points + point_firsts[i], &b, plans[j]))
            return fail(QOIMI_E_ARG, "band " + std::to_string(j) + ": " + what);
        image_of[j] = b.image; out_bytes[j] = (size_t)plans[j].info.size;
        if (out_offsets[j] > room || out_bytes[j] > room - out_offsets[j]) return fail(QOIMI_E_ARG, "band " + std::to_string(j) + ": the output ends behind the address space");
        ranges.push_back({(uintptr_t)d_out + out_offsets[j], (uintptr_t)d_out + out_offsets[j] + out_bytes[j], 1});
        ranges.push_back({(uintptr_t)d_streams + stream_offsets[i], (uintptr_t)d_streams + stream_offsets[i] + (size_t)sizes[i], 0});
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    uintptr_t end_any = 0, end_out = 0;                        // the furthest end so far of any range, of an output
    for (const Range& r : ranges) {
        if (r.out ? r.lo < end_any : r.lo < end_out) return fail(QOIMI_E_ARG, "an output range overlaps another or a stream of the call");
        if (r.hi > end_any) end_any = r.hi;
        if (r.out && r.hi > end_out) end_out = r.hi;
    }
    std::vector<uint32_t> first_tile; uint32_t tiles = 0;
    if (!band_tiles(plans, (uintptr_t)d_out, out_offsets, first_tile, tiles)) return fail(QOIMI_E_ARG, "more than 2^31 tiles of output words in one call");
    if (const int rc = assemble_bands(c, d_streams, stream_offsets, plans, image_of, d_out, out_offsets, first_tile, tiles, stream)) return rc;
    c->seek_stats[2] = 0;
    if (infos_out) for (size_t j = 0; j < n; ++j) infos_out[j] = plans[j].info;
    return QOIMI_OK;
}

// What the indexed calls share (qoi_amd/seekindex.py: bands_for_crops).  rows[i] / top[i]: the largest y + height and the smallest y over the
// items of image i (rows[i] == 0: no item names it, the image is not looked at).  Per referenced image, ascending, the band from the last seek
// row at or above top[i] to rows[i]; the band streams are assembled into the context's band arena and described as the inner call takes them:
// at / sz / ds are its stream_offsets / sizes / descs, number[i] is the band of image i and shift[r] what is added to the y of an item of band
// r (pad_rows - first_row, modulo 2^32).  Everything is looked at before anything is launched.
struct BandedCall { std::vector<size_t> at; std::vector<int> sz, number; std::vector<qoi_desc> ds; std::vector<uint32_t> shift; };

static int stage_bands(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs, int n_images,
                       const std::vector<uint32_t>& rows, const std::vector<uint32_t>& top, const unsigned* interval_rows, const qoimi_seek_point* points,
                       const size_t* point_firsts, void* stream, BandedCall& out) {
    std::vector<BandPlan> plans;
    std::vector<uint32_t> image_of;
    out.number.assign((size_t)n_images, -1);
    size_t arena = 0;
    for (int i = 0; i < n_images; ++i) {
        if (rows[(size_t)i] == 0u) continue;                   // (an image no item names is never looked at)
        const unsigned K = interval_rows[i];
        if (seek_point_count(descs[i].width, descs[i].height, K) < 0) return fail(QOIMI_E_ARG, "image " + std::to_string(i) + ": interval_rows * width below 128");
        qoimi_band b;
        b.image = (unsigned)i; b.first_row = top[(size_t)i] / K * K; b.rows = rows[(size_t)i] - b.first_row; b.reserved = 0u;
        BandPlan p;
        if (const char* what = band_wrong(&descs[i], sizes[i], K, points + point_firsts[i], &b, p)) return fail(QOIMI_E_ARG, "image " + std::to_string(i) + ": " + what);
        out.number[(size_t)i] = (int)plans.size();
        plans.push_back(p); image_of.push_back((uint32_t)i); out.shift.push_back(p.info.pad_rows - b.first_row); out.at.push_back(arena);
        arena += ((size_t)p.info.size + 15u) & ~(size_t)15u;
    }
    std::vector<uint32_t> first_tile; uint32_t tiles = 0;
    if (plans.size() > 0xFFFFFFFFu / kSeekHeadSlot) return fail(QOIMI_E_ARG, "more than 12 782 640 referenced images in one call");
    if (!band_tiles(plans, (uintptr_t)0, out.at.data(), first_tile, tiles)) return fail(QOIMI_E_ARG, "more than 2^31 tiles of band stream words in one call");
    {
        DeviceGuard guard(c->device);
        if (const int rc = reserve_exact(c->band_arena, arena)) return rc;
    }
    if (const int rc = assemble_bands(c, d_streams, stream_offsets, plans, image_of, c->band_arena.base, out.at.data(), first_tile, tiles, stream)) return rc;
    c->seek_stats[2] = (long long)arena;
    for (const BandPlan& p : plans) { out.sz.push_back((int)p.info.size); out.ds.push_back(p.info.desc); }
    return QOIMI_OK;
}

// The smallest y over the items of every image (~0: no item names it); the items have been checked.
template <class Item>
static std::vector<uint32_t> item_tops(const Item* items, size_t n, int n_images) {
    std::vector<uint32_t> top((size_t)n_images, ~0u);
    for (size_t j = 0; j < n; ++j) if (items[j].y < top[items[j].image]) top[items[j].image] = items[j].y;
    return top;
}

// The items as the inner call takes them: `image` the band's number, y - first_row + pad_rows.
template <class Item>
static std::vector<Item> rebase_items(const Item* items, size_t n, const BandedCall& b) {
    std::vector<Item> out(items, items + n);
    for (size_t j = 0; j < n; ++j) {
        const size_t r = (size_t)b.number[items[j].image];
        out[j].image = (unsigned)r; out[j].y = items[j].y + b.shift[r];
    }
    return out;
}

// The bands of qoi_amd/seekindex.py: bands_for_crops into the context's band arena, then qoimi_decode_crops as it is over them.
extern "C" int qoimi_decode_crops_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                          int n_images, int channels, const qoimi_crop* crops, int n_crops, void* d_out, const size_t* out_offsets,
                                          size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                          const size_t* point_firsts) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !crops || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_crops <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    const size_t n = (size_t)n_crops;
    CheckedItems ok;
    if (const int rc = check_items("crop", sizes, descs, n_images, channels, crops, n, d_out, out_offsets, crop_rect_wrong, crop_bytes, ok)) return rc;
    BandedCall b;
    if (const int rc = stage_bands(c, d_streams, stream_offsets, sizes, descs, n_images, ok.rows, item_tops(crops, n, n_images), interval_rows, points, point_firsts, stream, b)) return rc;
    const std::vector<qoimi_crop> cs = rebase_items(crops, n, b);
    return qoimi_decode_crops(c, c->band_arena.base, b.at.data(), b.sz.data(), b.ds.data(), (int)b.sz.size(), channels, cs.data(), n_crops, d_out, out_offsets, staging_bytes, stream);
}

// ... then qoimi_decode_resized as it is over them: the bands are those of the items' SOURCE rectangles.
extern "C" int qoimi_decode_resized_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                            int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                            size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                            const size_t* point_firsts) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    if (mode != QOIMI_RESIZE_PLAIN && mode != QOIMI_RESIZE_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_RESIZE_PLAIN or QOIMI_RESIZE_ALPHA_WEIGHTED");
    const size_t n = (size_t)n_items;
    CheckedItems ok;
    if (const int rc = check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, resize_item_wrong, resize_bytes, ok)) return rc;
    BandedCall b;
    if (const int rc = stage_bands(c, d_streams, stream_offsets, sizes, descs, n_images, ok.rows, item_tops(items, n, n_images), interval_rows, points, point_firsts, stream, b)) return rc;
    const std::vector<qoimi_resize> rs = rebase_items(items, n, b);
    return qoimi_decode_resized(c, c->band_arena.base, b.at.data(), b.sz.data(), b.ds.data(), (int)b.sz.size(), channels, rs.data(), n_items, mode, d_out, out_offsets, staging_bytes, stream);
}

// ... qoimi_decode_bilinear likewise.
extern "C" int qoimi_decode_bilinear_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                             int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                             size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                             const size_t* point_firsts) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (channels != 0 && channels != 3 && channels != 4) return fail(QOIMI_E_ARG, "channels must be 0, 3 or 4 (qoi.h:499)");
    if (mode != QOIMI_RESIZE_PLAIN && mode != QOIMI_RESIZE_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_RESIZE_PLAIN or QOIMI_RESIZE_ALPHA_WEIGHTED");
    const size_t n = (size_t)n_items;
    CheckedItems ok;
    if (const int rc = check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, bilinear_item_wrong, resize_bytes, ok)) return rc;
    BandedCall b;
    if (const int rc = stage_bands(c, d_streams, stream_offsets, sizes, descs, n_images, ok.rows, item_tops(items, n, n_images), interval_rows, points, point_firsts, stream, b)) return rc;
    const std::vector<qoimi_resize> rs = rebase_items(items, n, b);
    return qoimi_decode_bilinear(c, c->band_arena.base, b.at.data(), b.sz.data(), b.ds.data(), (int)b.sz.size(), channels, rs.data(), n_items, mode, d_out, out_offsets, staging_bytes, stream);
}

// ... and qoimi_pixel_stats (`first` is a pixel's value, not its place: the result is the plain call's).
extern "C" int qoimi_pixel_stats_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                         int n_images, const qoimi_crop* regions, int n_regions, qoimi_pixel_stat* stats_out, unsigned* d_hist,
                                         size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                         const size_t* point_firsts) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves stats_out as it was)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !regions || !stats_out || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_regions <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    const size_t n = (size_t)n_regions;
    CheckedItems ok;
    if (const int rc = check_refs("region", sizes, descs, n_images, 4, regions, n, crop_rect_wrong,
                                  [](size_t, const qoimi_crop*, unsigned) { return (int)QOIMI_OK; }, ok)) return rc;
    BandedCall b;
    if (const int rc = stage_bands(c, d_streams, stream_offsets, sizes, descs, n_images, ok.rows, item_tops(regions, n, n_images), interval_rows, points, point_firsts, stream, b)) return rc;
    const std::vector<qoimi_crop> rs = rebase_items(regions, n, b);
    return qoimi_pixel_stats(c, c->band_arena.base, b.at.data(), b.sz.data(), b.ds.data(), (int)b.sz.size(), rs.data(), n_regions, stats_out, d_hist, staging_bytes, stream);
}

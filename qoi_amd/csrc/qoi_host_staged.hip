// qoi_host_staged.hip — the gather calls of the C-ABI shim: they decode a pack's images into bounded staging and run one table-driven kernel
// over each sub-batch: qoimi_verify_images (and qoimi_compare_images, whose kernels it runs), qoimi_decode_thumbnails, qoimi_decode_crops,
// qoimi_decode_resized and qoimi_decode_bilinear (one body, two filter kinds), qoimi_decode_warped, qoimi_pixel_stats.  What they share with the row seek index
// and the indexed calls (qoi_host_seek.hip) - the item checks, the gather plan, run_staged - stands in qoi_staged.h.
#include "qoi_staged.h"
#include "qoi_thumb_core.h"
#include "qoi_stats_core.h"

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
    launch_compare((const uint8_t*)d_a, (const uint8_t*)d_b, d_tab, m, tiles, d_diffs, grid_bound(c, tiles), st, &c->timer);
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
    if (const int rc = check_out_channels(channels)) return rc;
    if (mode != QOIMI_THUMB_PLAIN && mode != QOIMI_THUMB_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_THUMB_PLAIN or QOIMI_THUMB_ALPHA_WEIGHTED");
    const size_t n = (size_t)n_images;
    std::vector<size_t> out_bytes(n);
    std::vector<uint32_t> rows(n);
    for (size_t i = 0; i < n; ++i) {
        if (sizes[i] < kHeaderBytes + kTrailerBytes) return fail(QOIMI_E_ARG, "stream " + std::to_string(i) + " shorter than 22 bytes (qoi.h:500)");
        if (!desc_ok(&descs[i])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(i) + " rejected (qoi.h:513-521 rules)");
        if (channels == 0 && descs[i].channels != descs[0].channels) return fail(QOIMI_E_ARG, "all images of a call must share the output channel count");
        if (factors[i] < 1u || factors[i] > kThumbMaxFactor) return fail(QOIMI_E_ARG, "factor " + std::to_string(i) + " outside 1..64");
        out_bytes[i] = (size_t)thumb_extent(descs[i].width, factors[i]) * thumb_extent(descs[i].height, factors[i]) * (size_t)(channels ? channels : descs[i].channels);
        rows[i] = descs[i].height;
    }
    const unsigned och = channels ? (unsigned)channels : descs[0].channels;
    // (unlike check_items, this call has never looked whether an output ends inside the address space)
    if (ranges_overlap(thumb_offsets, out_bytes)) return fail(QOIMI_E_ARG, "the output ranges of two thumbnails overlap");
    GatherPlan gp;                                             // (entry i is image i)
    if (const int rc = plan_gather(descs, n_images, rows, staging_bytes, n, [](size_t i) { return (uint32_t)i; },
                                   [&](size_t i) { return thumb_tiles(descs[i].width, descs[i].height, factors[i]); },
                                   "more than 2^31 tiles of thumbnail pixels in one sub-batch", gp)) return rc;
    const RowsPlan& plan = gp.rows; const ItemPlan& items = gp.items;
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
    if (const int rc = check_out_channels(channels)) return rc;
    const size_t n = (size_t)n_crops;
    CheckedItems ok;
    if (const int rc = check_items("crop", sizes, descs, n_images, channels, crops, n, d_out, out_offsets, crop_rect_wrong, crop_bytes, ok)) return rc;
    const unsigned och = ok.och;
    GatherPlan gp;
    if (const int rc = plan_gather(descs, n_images, ok.rows, staging_bytes, n, [&](size_t j) { return crops[j].image; },
                                   [&](size_t j) { return crop_tiles((uint64_t)(uintptr_t)d_out + out_offsets[j], ok.out_bytes[j]); },
                                   "more than 2^31 tiles of output words in one sub-batch", gp)) return rc;
    const RowsPlan& plan = gp.rows; const ItemPlan& items = gp.items;
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
// rectangles of a pack's images resampled to fixed sizes: the area filter and the antialiased bilinear filter (qoi_resize.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_resize) == 32 && offsetof(qoimi_resize, image) == 0 && offsetof(qoimi_resize, x) == 4 && offsetof(qoimi_resize, y) == 8 &&
              offsetof(qoimi_resize, width) == 12 && offsetof(qoimi_resize, height) == 16 && offsetof(qoimi_resize, out_width) == 20 &&
              offsetof(qoimi_resize, out_height) == 24 && offsetof(qoimi_resize, flags) == 28, "qoimi_resize layout");
static_assert(QOIMI_RESIZE_FLIP_X == (int)kResizeFlipX && QOIMI_RESIZE_FLIP_Y == (int)kResizeFlipY, "the table's flag bits");
static_assert(QOIMI_RESIZE_PLAIN == 0 && QOIMI_RESIZE_ALPHA_WEIGHTED == 1, "the table's mode bit");

static size_t resample_size(const ResampleKind& kind, const qoi_desc* desc, const qoimi_resize* item, int channels) {
    size_t bytes = 0;
    if (!desc_ok(desc) || !item || (channels != 3 && channels != 4) || kind.wrong(desc, item) || !resize_bytes(item, (unsigned)channels, &bytes)) return 0;
    return bytes;
}

// gather_resampled (qoi_staged.h) with bytes as the output: one launch of the filter's kernel over the sub-batch's items.
static int decode_resampled(const ResampleKind& kind, qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                            int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                            size_t staging_bytes, void* stream) {
    return gather_resampled(kind, c, d_streams, stream_offsets, sizes, descs, n_images, channels, items, n_items, mode, d_out, out_offsets, staging_bytes, stream,
                            accept_any, resize_bytes, accept_outputs, kind.stats, kind.kernel,
        [&](const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            kind.launch((const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, grid, st);
        });
}

extern "C" size_t qoimi_resize_size(const qoi_desc* desc, const qoimi_resize* item, int channels) { return resample_size(kAreaKind, desc, item, channels); }

extern "C" int qoimi_decode_resized(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                    int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                    size_t staging_bytes, void* stream) {
    return decode_resampled(kAreaKind, c, d_streams, stream_offsets, sizes, descs, n_images, channels, items, n_items, mode, d_out, out_offsets, staging_bytes, stream);
}

extern "C" size_t qoimi_bilinear_size(const qoi_desc* desc, const qoimi_resize* item, int channels) { return resample_size(kTentKind, desc, item, channels); }

extern "C" int qoimi_decode_bilinear(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                     int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                     size_t staging_bytes, void* stream) {
    return decode_resampled(kTentKind, c, d_streams, stream_offsets, sizes, descs, n_images, channels, items, n_items, mode, d_out, out_offsets, staging_bytes, stream);
}

// ------------------------------------------------------------------------------------
// rectangles of a pack's images sampled through an affine map (qoi_warp.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_warp) == 72 && offsetof(qoimi_warp, image) == 0 && offsetof(qoimi_warp, x) == 4 && offsetof(qoimi_warp, y) == 8 &&
              offsetof(qoimi_warp, width) == 12 && offsetof(qoimi_warp, height) == 16 && offsetof(qoimi_warp, out_width) == 20 &&
              offsetof(qoimi_warp, out_height) == 24 && offsetof(qoimi_warp, flags) == 28 && offsetof(qoimi_warp, a) == 32 && offsetof(qoimi_warp, b) == 36 &&
              offsetof(qoimi_warp, d) == 40 && offsetof(qoimi_warp, e) == 44 && offsetof(qoimi_warp, fill) == 48 && offsetof(qoimi_warp, reserved) == 52 &&
              offsetof(qoimi_warp, c) == 56 && offsetof(qoimi_warp, f) == 64, "qoimi_warp layout");
static_assert(QOIMI_WARP_REPLICATE == (int)kWarpReplicate && QOIMI_WARP_NEAREST == (int)kWarpNearest && QOIMI_WARP_BICUBIC == (int)kWarpBicubic &&
              QOIMI_WARP_REFLECT == (int)kWarpReflect && QOIMI_WARP_REFLECT_101 == (int)kWarpReflect101 && QOIMI_WARP_WRAP == (int)kWarpWrap,
              "the table's flag bits: 2, 8 and 32 are not flags, nor is a bit from 512 on");
static_assert(QOIMI_WARP_SUPER2 == (int)kWarpSuper2 && QOIMI_WARP_SUPER4 == (int)kWarpSuper4 && (kWarpSuper4 << 16) != 0u,
              "the supersampling flags: 512 is not a flag, nor is 4096; the table carries 16 flag bits");
static_assert(QOIMI_WARP_VOTE2 == (int)kWarpVote2 && QOIMI_WARP_VOTE4 == (int)kWarpVote4 && (kWarpVote4 << 16) == (1u << 30),
              "the vote flags: 4096 is not a flag, nor is a bit from 32768 on; the table carries 16 flag bits");
static_assert(QOIMI_WARP_PROJECTIVE == (int)kWarpProjective && kWarpProjective == (1u << 17) && (kWarpEntryProjective & 0xFFFFFDFFu) == 0u,
              "the projective flag: 32768 and 65536 are not flags; the table carries it in bit 9 of cfg, between the alpha mode and the 16 flag bits");

extern "C" size_t qoimi_warp_size(const qoi_desc* desc, const qoimi_warp* item, int channels) {
    size_t bytes = 0;
    if (!desc_ok(desc) || !item || (channels != 3 && channels != 4) || warp_item_wrong(desc, item) || !warp_bytes(item, (unsigned)channels, &bytes)) return 0;
    return bytes;
}

// The map that shows the rectangle in an EXIF orientation (qoi_amd/warp.py: orient): every output pixel's position is a sample's centre, so
// every blend has one sample of the full weight.  S = 65536: a column k of the rectangle mirrored is cw - 1 - k, 2 * (cw - 1 - k) + 1 =
// 2 * cw - (2k + 1): the factor -S and the offset 2 * cw * S.
extern "C" int qoimi_warp_orient(const qoi_desc* desc, unsigned x, unsigned y, unsigned width, unsigned height, int exif_orientation, qoimi_warp* out) {
    if (!desc_ok(desc) || !out) return fail(QOIMI_E_ARG, "NULL argument or rejected descriptor");
    if (exif_orientation < 1 || exif_orientation > 8) return fail(QOIMI_E_ARG, "exif_orientation must be 1..8");
    if (width == 0u || height == 0u) return fail(QOIMI_E_ARG, "zero width or height");
    if ((uint64_t)x + width > desc->width || (uint64_t)y + height > desc->height) return fail(QOIMI_E_ARG, "the rectangle leaves its image");
    const bool transposed = exif_orientation >= 5;                 // 5..8: the output's columns run along the rectangle's rows
    const bool mirror_cols = exif_orientation == 2 || exif_orientation == 3 || exif_orientation == 7 || exif_orientation == 8;
    const bool mirror_rows = exif_orientation == 3 || exif_orientation == 4 || exif_orientation == 6 || exif_orientation == 7;
    const int S = 65536;
    const int sx = mirror_cols ? -S : S, sy = mirror_rows ? -S : S;
    memset(out, 0, sizeof(*out));
    out->x = x; out->y = y; out->width = width; out->height = height;
    out->out_width = transposed ? height : width; out->out_height = transposed ? width : height;
    out->a = transposed ? 0 : sx; out->b = transposed ? sx : 0;
    out->d = transposed ? sy : 0; out->e = transposed ? 0 : sy;
    out->c = mirror_cols ? 2ll * width * S : 0; out->f = mirror_rows ? 2ll * height * S : 0;
    return QOIMI_OK;
}

// gather_warped (qoi_staged.h) with bytes as the output: one launch of warp_gather over the sub-batch's items - of warp_bicubic_bytes
// (qoi_warp_cubic.hip) where an item of the call carries QOIMI_WARP_BICUBIC, of warp_border_bytes (qoi_warp_border.hip) where one carries
// QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 or QOIMI_WARP_WRAP, of warp_super_bytes (qoi_warp_super.hip) where one carries QOIMI_WARP_SUPER2 or
// QOIMI_WARP_SUPER4, of warp_vote_bytes (qoi_warp_vote.hip) where one carries QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4, of warp_proj_bytes (qoi_warp_proj.hip)
// where one carries QOIMI_WARP_PROJECTIVE.
extern "C" int qoimi_decode_warped(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                   int n_images, int channels, const qoimi_warp* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                   size_t staging_bytes, void* stream) {
    return gather_warped(c, d_streams, stream_offsets, sizes, descs, n_images, channels, items, n_items, mode, d_out, out_offsets, staging_bytes, stream,
                         accept_any, warp_bytes, accept_outputs, &qoimi_ctx::warp_stats, {"warp_gather", "warp_bicubic_bytes", "warp_border_bytes", "warp_super_bytes", "warp_vote_bytes"}, "warp_proj_bytes",
        [&](WarpKernel kind, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            (kind == kWarpKernelProj ? launch_warp_proj : kind == kWarpKernelVote ? launch_warp_vote
                                    : (kind == kWarpKernelSuper ? launch_warp_super : (kind == kWarpKernelBorder ? launch_warp_border : (kind == kWarpKernelCubic ? launch_warp_cubic : launch_warp))))(
                (const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, grid, st);
        });
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
    if (const int rc = check_regions(sizes, descs, n_images, regions, n, ok)) return rc;
    GatherPlan gp;
    if (const int rc = plan_gather(descs, n_images, ok.rows, staging_bytes, n, [&](size_t j) { return regions[j].image; },
                                   [&](size_t j) { return stats_tiles(regions[j].width, regions[j].height); },
                                   "more than 2^31 tiles of region pixels in one sub-batch", gp)) return rc;
    const RowsPlan& plan = gp.rows; const ItemPlan& items = gp.items;
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


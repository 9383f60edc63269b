// qoi_staged.h — what the host files of the calls that decode through bounded staging share (qoi_host_staged.hip: the gather calls,
// qoi_host_tensor.hip: the tensor calls, qoi_host_seek.hip: the seek index build and the indexed calls): the checks of a call's items, the
// plan of a gather call, run_staged - the driver of "decode a sub-batch into the staging arena, one table-driven launch over it" - and the
// bodies of the resampling and warp calls.  Host only; no kernel file includes it.
#pragma once
#include "qoi_ctx.h"
#include "qoi_crop_core.h"
#include "qoi_resize_core.h"
#include "qoi_bilinear_core.h"
#include "qoi_warp_core.h"
#include "qoi_warp_border_core.h"
#include "qoi_warp_cubic_core.h"
#include "qoi_warp_super_core.h"
#include "qoi_warp_vote_core.h"
#include "qoi_warp_proj_core.h"

// ------------------------------------------------------------------------------------
// the few lines several entry points repeat
// ------------------------------------------------------------------------------------
static int check_resize_mode(int mode) {
    if (mode != QOIMI_RESIZE_PLAIN && mode != QOIMI_RESIZE_ALPHA_WEIGHTED) return fail(QOIMI_E_ARG, "mode must be QOIMI_RESIZE_PLAIN or QOIMI_RESIZE_ALPHA_WEIGHTED");
    return QOIMI_OK;
}

// Behind a launch: QOIMI_OK, or - the stream waited for - the failure with `kernel` in its message.
static int launch_check(const char* kernel, hipStream_t st) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return QOIMI_OK;
    (void)hipStreamSynchronize(st);
    return fail(QOIMI_E_INTERNAL, std::string(kernel) + ": " + hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------
// a call's items
// ------------------------------------------------------------------------------------
// What check_items makes of a call's items.  rows[i]: the rows of image i that are decoded, 0: no item names it; out_bytes[j]: the bytes of
// output j; och: the output channel count of the call.
struct CheckedItems { std::vector<uint32_t> rows; std::vector<size_t> out_bytes; unsigned och = 0; };

// The items of qoimi_decode_crops (`noun` "crop"), of qoimi_decode_resized, qoimi_decode_bilinear and qoimi_decode_warped ("item") and of qoimi_pixel_stats ("region"), looked at in the order
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

// What the items of both resampling calls are checked for first, in this order; then the ratio and, for bilinear, the area product last.
static const char* resample_rect_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (r->width == 0u || r->height == 0u || r->out_width == 0u || r->out_height == 0u) return "zero width or height";
    if ((r->flags & ~(unsigned)(QOIMI_RESIZE_FLIP_X | QOIMI_RESIZE_FLIP_Y)) != 0u) return "unknown flag bit";
    if ((uint64_t)r->x + r->width > d->width || (uint64_t)r->y + r->height > d->height) return "the rectangle leaves its image";
    return nullptr;
}

// nullptr if the item is fine for an accepted descriptor, else what is wrong with it
static const char* resize_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (const char* what = resample_rect_wrong(d, r)) return what;
    if (r->width > (uint64_t)kResizeMaxRatio * r->out_width || r->height > (uint64_t)kResizeMaxRatio * r->out_height) return "reduced by more than 64 in an axis";
    return nullptr;
}

// ... with the ratio limit of 32 and the product limit (qoi_bilinear_core.h: what keeps a weight in 32 bits and the sums in 64)
static const char* bilinear_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (const char* what = resample_rect_wrong(d, r)) return what;
    if (r->width > (uint64_t)kBilinearMaxRatio * r->out_width || r->height > (uint64_t)kBilinearMaxRatio * r->out_height) return "reduced by more than 32 in an axis";
    const uint64_t mx = r->width > r->out_width ? r->width : r->out_width, my = r->height > r->out_height ? r->height : r->out_height;
    if (mx * my >= kBilinearMaxArea) return "max(width, out_width) * max(height, out_height) is 2^30 or more";
    return nullptr;
}

// out_width * out_height * och, false if that does not fit a size_t
static bool resize_bytes(const qoimi_resize* r, unsigned och, size_t* bytes) {
    const uint64_t px = (uint64_t)r->out_width * r->out_height;
    if (px > ~(size_t)0 / och) return false;
    *bytes = (size_t)px * och;
    return true;
}

// The items of qoimi_decode_warped, in this order: the rectangle rules of resample_rect_wrong (a zero size, then a rectangle that leaves its
// image), the output's sides, its pixels, the map's offsets (qoi_warp_core.h: what keeps both positions in 64 bits), the flags (a bit that is
// none, then the two samplings together, then more than one of the four borders, then both SUPER flags, then a SUPER flag with a sampling
// that is not the bilinear one, then both VOTE flags, then a VOTE flag with another sampling or a SUPER flag), reserved.  With
// QOIMI_WARP_PROJECTIVE `reserved` holds the item's g and h and is not looked at as such; in its place stand the rules of
// qoi_warp_proj_core.h: the flag with a SUPER or VOTE flag, then the tighter offsets, then the least denominator inside the output.
static const char* warp_item_wrong(const qoi_desc* d, const qoimi_warp* r) {
    if (r->width == 0u || r->height == 0u || r->out_width == 0u || r->out_height == 0u) return "zero width or height";
    if ((uint64_t)r->x + r->width > d->width || (uint64_t)r->y + r->height > d->height) return "the rectangle leaves its image";
    if (r->out_width >= kWarpMaxOut || r->out_height >= kWarpMaxOut) return "out_width or out_height is 2^20 or more";
    if ((uint64_t)r->out_width * r->out_height >= kWarpMaxArea) return "out_width * out_height is 400 000 000 or more";
    if (r->c <= -kWarpMaxOffset || r->c >= kWarpMaxOffset || r->f <= -kWarpMaxOffset || r->f >= kWarpMaxOffset) return "|c| or |f| is 2^56 or more";
    const unsigned supers = r->flags & (QOIMI_WARP_SUPER2 | QOIMI_WARP_SUPER4);
    const unsigned known = QOIMI_WARP_REPLICATE | QOIMI_WARP_NEAREST | QOIMI_WARP_BICUBIC | QOIMI_WARP_REFLECT | QOIMI_WARP_REFLECT_101 | QOIMI_WARP_WRAP |
                           QOIMI_WARP_SUPER2 | QOIMI_WARP_SUPER4 | QOIMI_WARP_VOTE2 | QOIMI_WARP_VOTE4 | QOIMI_WARP_PROJECTIVE;
    const unsigned votes = r->flags & (QOIMI_WARP_VOTE2 | QOIMI_WARP_VOTE4);
    const unsigned borders = r->flags & (QOIMI_WARP_REPLICATE | QOIMI_WARP_REFLECT | QOIMI_WARP_REFLECT_101 | QOIMI_WARP_WRAP);
    if ((r->flags & ~known) != 0u) return "unknown flag bit";
    if ((r->flags & QOIMI_WARP_NEAREST) != 0u && (r->flags & QOIMI_WARP_BICUBIC) != 0u) return "QOIMI_WARP_NEAREST and QOIMI_WARP_BICUBIC together";
    if ((borders & (borders - 1u)) != 0u)                          // (more than one bit)
        return "more than one border of QOIMI_WARP_REPLICATE, QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 and QOIMI_WARP_WRAP";
    if ((supers & (supers - 1u)) != 0u) return "QOIMI_WARP_SUPER2 and QOIMI_WARP_SUPER4 together";
    if (supers != 0u && (r->flags & (QOIMI_WARP_NEAREST | QOIMI_WARP_BICUBIC)) != 0u)
        return "supersampling is defined for the bilinear sampling only: QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4 with QOIMI_WARP_NEAREST or QOIMI_WARP_BICUBIC";
    if ((votes & (votes - 1u)) != 0u) return "QOIMI_WARP_VOTE2 and QOIMI_WARP_VOTE4 together";
    if (votes != 0u && (r->flags & (QOIMI_WARP_NEAREST | QOIMI_WARP_BICUBIC | QOIMI_WARP_SUPER2 | QOIMI_WARP_SUPER4)) != 0u)
        return "the vote is a sampling of its own: QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4 with QOIMI_WARP_NEAREST, QOIMI_WARP_BICUBIC, QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4";
    if ((r->flags & QOIMI_WARP_PROJECTIVE) != 0u) {
        if (supers != 0u || votes != 0u)
            return "the projective map is defined for the bilinear, nearest and bicubic samplings: QOIMI_WARP_PROJECTIVE with QOIMI_WARP_SUPER2, QOIMI_WARP_SUPER4, QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4";
        if (r->c <= -kWarpProjMaxOffset || r->c >= kWarpProjMaxOffset || r->f <= -kWarpProjMaxOffset || r->f >= kWarpProjMaxOffset)
            return "|c| or |f| is 2^53 or more with QOIMI_WARP_PROJECTIVE";
        const uint32_t F = warp_proj_bits(r->out_width, r->out_height);
        if (warp_proj_least(warp_proj_of(r->reserved), F, r->out_width, r->out_height) < ((int64_t)1 << (F - 3u)))
            return "the denominator of QOIMI_WARP_PROJECTIVE falls below 1/8 inside the output: 2^F - |g| * (out_width - 1) - |h| * (out_height - 1) < 2^(F - 3)";
        return nullptr;                                            // (reserved holds g and h)
    }
    if (r->reserved != 0u) return "reserved is not 0";
    return nullptr;
}

// out_width * out_height * och (fewer than 400 000 000 pixels: it always fits)
static bool warp_bytes(const qoimi_warp* r, unsigned och, size_t* bytes) {
    *bytes = (size_t)r->out_width * r->out_height * och;
    return true;
}

// The regions of qoimi_pixel_stats: no output per item.
static int check_regions(const int* sizes, const qoi_desc* descs, int n_images, const qoimi_crop* regions, size_t n, CheckedItems& ok) {
    return check_refs("region", sizes, descs, n_images, 4, regions, n, crop_rect_wrong, [](size_t, const qoimi_crop*, unsigned) { return (int)QOIMI_OK; }, ok);
}

// ------------------------------------------------------------------------------------
// the plan of a gather call
// ------------------------------------------------------------------------------------
// rows: plan_rows over the rows of every image that are decoded (qoi_amd/crops.py: plan - a function of descs, the items and staging_bytes
// alone); items: plan_items over the items, item j of n naming image image_of(j) and taking tiles_of(j) tiles.  `overflow`: the message of
// a sub-batch with 2^31 - 1 tiles or more.
struct GatherPlan { RowsPlan rows; ItemPlan items; };

template <class ImageOf, class TilesOf>
static int plan_gather(const qoi_desc* descs, int n_images, const std::vector<uint32_t>& rows, size_t staging_bytes, size_t n, ImageOf image_of,
                       TilesOf tiles_of, const char* overflow, GatherPlan& out) {
    out.rows = plan_rows(descs, n_images, rows, staging_bytes);
    std::vector<uint32_t> image(n);
    std::vector<uint64_t> tiles(n);
    for (size_t j = 0; j < n; ++j) { image[j] = image_of(j); tiles[j] = tiles_of(j); }
    out.items = plan_items(image, out.rows.ref_of, out.rows.firsts, tiles);
    if (out.items.overflow) return fail(QOIMI_E_ARG, overflow);
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// decode through staging, then one table-driven kernel per sub-batch
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
    for (size_t k = 0; k < items.subs.size(); ++k) {
        const ItemSub& s = items.subs[k];
        const int rc = decode_rows(c, d_streams, stream_offsets, sizes, descs, plan, rows, k, stream);
        if (rc != QOIMI_OK) { (void)hipStreamSynchronize(st); return rc; }
        stats[0] += 1;
        launch(d_tab + s.entry, s.m, s.tiles, grid_bound(c, s.tiles), st);
        if (const int failed = launch_check(kernel, st)) return failed;
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
// the resampling calls and the warp call, whatever their kernels write (qoi_host_staged.hip: bytes, qoi_host_tensor.hip: tensors)
// ------------------------------------------------------------------------------------
// A resampling filter: what is wrong with an item, how an output pixel's source pixels are split over lanes and the tiles of an item (its
// core header); and of the call that writes bytes: its launcher, the context's counters of its last call, its kernel's name for a launch
// failure.
struct ResampleKind {
    const char* (*wrong)(const qoi_desc*, const qoimi_resize*);
    void (*split)(uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh, uint32_t& lg, uint32_t& c);
    uint64_t (*tiles)(uint32_t cw, uint32_t rh, uint32_t ow, uint32_t oh);
    void (*launch)(const uint8_t*, const ResizeEntry*, uint32_t, uint32_t, uint8_t*, uint32_t, hipStream_t);
    long long (qoimi_ctx::*stats)[4];
    const char* kernel;
};
// The filters that split an output pixel's COLUMNS over lanes and loop over its rows: their split and tiles take no heights
template <void (*Split)(uint32_t, uint32_t, uint32_t&, uint32_t&)>
static void split_columns(uint32_t cw, uint32_t, uint32_t ow, uint32_t, uint32_t& lg, uint32_t& c) { Split(cw, ow, lg, c); }
template <uint64_t (*Tiles)(uint32_t, uint32_t, uint32_t)>
static uint64_t tiles_columns(uint32_t cw, uint32_t, uint32_t ow, uint32_t oh) { return Tiles(cw, ow, oh); }
static const ResampleKind kAreaKind = {resize_item_wrong, split_columns<resize_split>, tiles_columns<resize_tiles>, launch_resize, &qoimi_ctx::resize_stats, "resize_filter"};
static const ResampleKind kTentKind = {bilinear_item_wrong, split_columns<bilinear_split>, tiles_columns<bilinear_tiles>, launch_bilinear, &qoimi_ctx::bilinear_stats, "bilinear_filter"};

// The hooks of a call that has nothing to add to the checks
static int accept_any() { return QOIMI_OK; }
static int accept_outputs(const CheckedItems&) { return QOIMI_OK; }

// A resampling call from its arguments to its last launch.  The checks, in this order: NULL / empty arguments, channels, mode, before() - what
// the call checks of arguments of its own -, the items (check_items with bytes_of(item, och, &bytes), the size of an output),
// after(checked items) - what it checks of the accepted outputs.  Then the plan of qoimi_decode_crops over the items' rectangles
// (qoi_amd/resize.py: plan, qoi_amd/bilinear.py: plan) and run_staged with launch(entries, m, tiles, workgroups, stream) once per sub-batch;
// stats: the context's counters of the call, kernel: the name in the message of a failed launch.
template <class Before, class Bytes, class After, class Launch>
static int gather_resampled(const ResampleKind& kind, qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                            int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                            size_t staging_bytes, void* stream, Before before, Bytes bytes_of, After after, long long (qoimi_ctx::*stats)[4], const char* kernel,
                            Launch launch) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (const int rc = check_out_channels(channels)) return rc;
    if (const int rc = check_resize_mode(mode)) return rc;
    if (const int rc = before()) return rc;
    const size_t n = (size_t)n_items;
    CheckedItems ok;
    if (const int rc = check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, kind.wrong, bytes_of, ok)) return rc;
    if (const int rc = after(ok)) return rc;
    const unsigned och = ok.och;
    GatherPlan gp;
    if (const int rc = plan_gather(descs, n_images, ok.rows, staging_bytes, n, [&](size_t j) { return items[j].image; },
                                   [&](size_t j) { return kind.tiles(items[j].width, items[j].height, items[j].out_width, items[j].out_height); },
                                   "more than 2^31 tiles of output pixels in one sub-batch", gp)) return rc;
    const RowsPlan& plan = gp.rows; const ItemPlan& order = gp.items;
    const uint32_t weighted = (mode == QOIMI_RESIZE_ALPHA_WEIGHTED && och == 4u) ? 1u : 0u;   // with 3 output channels the mode is PLAIN
    return run_staged<ResizeEntry>(c, c->*stats, (long long)plan.refs.size(), kernel, d_streams, stream_offsets, sizes, descs, plan, ok.rows, order,
        [&](ResizeEntry& t, size_t e) {
            const size_t j = order.by_ref[e];
            const qoimi_resize& r = items[j];
            uint32_t lg, cols;
            kind.split(r.width, r.height, r.out_width, r.out_height, lg, cols);
            t.src_off = (u64)plan.at[(size_t)plan.ref_of[r.image]]; t.dst_off = (u64)out_offsets[j];
            t.w = descs[r.image].width; t.x = r.x; t.y = r.y; t.cw = r.width; t.rh = r.height; t.ow = r.out_width; t.oh = r.out_height;
            t.first_tile = order.first_tile[e]; t.cfg = lg | (cols << 8) | (och << 16) | (weighted << 24) | (r.flags << 28); t.reserved = 0u;
        }, launch, stream);
}

// ... and the warp call (the plan: qoi_amd/warp.py: plan).  launch(kind, entries, m, tiles, workgroups, stream): kind is kWarpKernelProj
// where an item of the CALL carries QOIMI_WARP_PROJECTIVE - then every sub-batch runs the kernel of qoi_warp_proj.hip, which serves every
// other item as well, VOTE items included; `proj_kernel` is its name in the message of a failed launch -, else kWarpKernelVote
// where an item of the CALL carries QOIMI_WARP_VOTE2 or QOIMI_WARP_VOTE4 - then every sub-batch runs the kernel of qoi_warp_vote.hip, which
// serves every other item as well -, else kWarpKernelSuper
// where one carries QOIMI_WARP_SUPER2 or QOIMI_WARP_SUPER4 - the kernel of qoi_warp_super.hip, likewise -, else kWarpKernelBorder
// where one carries QOIMI_WARP_REFLECT, QOIMI_WARP_REFLECT_101 or QOIMI_WARP_WRAP - the kernel of
// qoi_warp_border.hip, likewise -, else kWarpKernelCubic where one carries QOIMI_WARP_BICUBIC - the kernel of
// qoi_warp_cubic.hip, likewise -, else kWarpKernelPlain: a call without those flags launches what it always launched.  kernels[kind] is the
// name in the message of a failed launch.
enum WarpKernel { kWarpKernelPlain = 0, kWarpKernelCubic = 1, kWarpKernelBorder = 2, kWarpKernelSuper = 3, kWarpKernelVote = 4, kWarpKernelProj = 5 };
template <class Before, class Bytes, class After, class Launch>
static int gather_warped(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs, int n_images, int channels,
                         const qoimi_warp* items, int n_items, int mode, void* d_out, const size_t* out_offsets, size_t staging_bytes, void* stream,
                         Before before, Bytes bytes_of, After after, long long (qoimi_ctx::*stats)[4], const char* const (&kernels)[5], const char* proj_kernel, Launch launch) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (const int rc = check_out_channels(channels)) return rc;
    if (const int rc = check_resize_mode(mode)) return rc;
    if (const int rc = before()) return rc;
    const size_t n = (size_t)n_items;
    CheckedItems ok;
    if (const int rc = check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, warp_item_wrong, bytes_of, ok)) return rc;
    if (const int rc = after(ok)) return rc;
    const unsigned och = ok.och;
    GatherPlan gp;
    if (const int rc = plan_gather(descs, n_images, ok.rows, staging_bytes, n, [&](size_t j) { return items[j].image; },
                                   [&](size_t j) { return warp_tiles(items[j].out_width, items[j].out_height); },
                                   "more than 2^31 tiles of output pixels in one sub-batch", gp)) return rc;
    const RowsPlan& plan = gp.rows; const ItemPlan& order = gp.items;
    const uint32_t weighted = (mode == QOIMI_RESIZE_ALPHA_WEIGHTED && och == 4u) ? 1u : 0u;   // with 3 output channels the mode is PLAIN
    unsigned any = 0u;
    for (size_t j = 0; j < n; ++j) any |= items[j].flags;
    const WarpKernel kind = (any & kWarpProjective) != 0u ? kWarpKernelProj
                          : (any & kWarpVotes) != 0u ? kWarpKernelVote
                          : ((any & kWarpSupers) != 0u ? kWarpKernelSuper
                          : ((any & kWarpBorders) != 0u ? kWarpKernelBorder : ((any & QOIMI_WARP_BICUBIC) != 0u ? kWarpKernelCubic : kWarpKernelPlain)));
    return run_staged<WarpEntry>(c, c->*stats, (long long)plan.refs.size(), kind == kWarpKernelProj ? proj_kernel : kernels[kind], d_streams, stream_offsets, sizes, descs, plan, ok.rows, order,
        [&](WarpEntry& t, size_t e) {
            const size_t j = order.by_ref[e];
            const qoimi_warp& r = items[j];
            t.src_off = (u64)plan.at[(size_t)plan.ref_of[r.image]]; t.dst_off = (u64)out_offsets[j];
            t.w = descs[r.image].width; t.x = r.x; t.y = r.y; t.cw = r.width; t.rh = r.height; t.ow = r.out_width; t.oh = r.out_height;
            t.first_tile = order.first_tile[e]; t.cfg = och | (weighted << 8) | ((r.flags & 0xFFFFu) << 16); t.fill = r.fill;
            t.a = r.a; t.b = r.b; t.d = r.d; t.e = r.e; t.c = r.c; t.f = r.f;
            const bool projective = (r.flags & kWarpProjective) != 0u;
            const WarpProj pj = warp_proj_of(projective ? r.reserved : 0u);
            if (projective) t.cfg |= kWarpEntryProjective;
            t.g = pj.g; t.h = pj.h;
        }, [&](const WarpEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) { launch(kind, tab, m, tiles, grid, st); }, stream);
}

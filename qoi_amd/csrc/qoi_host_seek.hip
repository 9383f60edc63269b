// qoi_host_seek.hip — the calls of the C-ABI shim around the row seek index: qoimi_seek_points, its two builds (qoimi_build_seek_index through
// the staged-decode driver of qoi_staged.h, qoimi_seek_index_from_pixels - which stages nothing; one kernel pair, seekpx_last + seekpx_carry,
// serves both: over the staging arena and over the caller's pixels), qoimi_band_plan, qoimi_make_band_streams, and the indexed forms of the
// gather calls (qoimi_decode_crops_indexed, qoimi_decode_resized_indexed, qoimi_decode_bilinear_indexed, qoimi_pixel_stats_indexed), which
// assemble the band streams their items need and make the plain call of qoi_host_staged.hip over them.
#include "qoi_staged.h"
#include "qoi_seek_core.h"

#include <stddef.h>

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
    GatherPlan gp;                                             // (its refs are k.refs, the images that have a point; entry r is the r-th of them)
    if (const int rc = plan_gather(descs, n_images, rows, staging_bytes, k.refs.size(), [&](size_t r) { return (uint32_t)k.refs[r]; },
                                   [&](size_t r) { return k.ref_tiles[r]; }, "more than 2^31 tiles of pixels in one sub-batch", gp)) return rc;
    const RowsPlan& plan = gp.rows; const ItemPlan& items = gp.items;
    const size_t R = plan.refs.size();
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
    launch_seek_tables_px((const uint8_t*)d_pixels, (const SeekPxImage*)at.d_extra, (uint32_t)R, t, at.d_last, at.d_loc, at.d_points, grid_bound(c, t), st);
    if (const int failed = launch_check("seekpx_last", st)) return failed;
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
    launch_band_assemble((const uint8_t*)d_streams, (const BandEntry*)c->cmp_ws.base, (uint32_t)n, tiles, (const uint8_t*)c->cmp_ws.base + tab_bytes,
                         (uint8_t*)d_out, grid_bound(c, tiles), st);
    if (const int failed = launch_check("band_assemble", st)) return failed;
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


// What the four indexed calls do behind their NULL / channels / mode tests: check(ok) - the item check of the family, as the plain call makes
// it -, the bands of qoi_amd/seekindex.py: bands_for_crops into the context's band arena, then inner(band arena, stream_offsets, sizes, descs,
// n_images, items): the plain call as it is over the band streams and the rebased items (which it checks again).
template <class Item, class Check, class Inner>
static int run_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs, int n_images,
                       const Item* items, size_t n, const unsigned* interval_rows, const qoimi_seek_point* points, const size_t* point_firsts,
                       void* stream, Check check, Inner inner) {
    CheckedItems ok;
    if (const int rc = check(ok)) return rc;
    BandedCall b;
    if (const int rc = stage_bands(c, d_streams, stream_offsets, sizes, descs, n_images, ok.rows, item_tops(items, n, n_images), interval_rows, points, point_firsts, stream, b)) return rc;
    const std::vector<Item> rebased = rebase_items(items, n, b);
    return inner(c->band_arena.base, b.at.data(), b.sz.data(), b.ds.data(), (int)b.sz.size(), rebased.data());
}

// ... qoimi_decode_crops over the bands of the crops.
extern "C" int qoimi_decode_crops_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                          int n_images, int channels, const qoimi_crop* crops, int n_crops, void* d_out, const size_t* out_offsets,
                                          size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                          const size_t* point_firsts) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !crops || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_crops <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (const int rc = check_out_channels(channels)) return rc;
    const size_t n = (size_t)n_crops;
    return run_indexed(c, d_streams, stream_offsets, sizes, descs, n_images, crops, n, interval_rows, points, point_firsts, stream,
        [&](CheckedItems& ok) { return check_items("crop", sizes, descs, n_images, channels, crops, n, d_out, out_offsets, crop_rect_wrong, crop_bytes, ok); },
        [&](const void* bands, const size_t* at, const int* sz, const qoi_desc* ds, int m, const qoimi_crop* cs) {
            return qoimi_decode_crops(c, bands, at, sz, ds, m, channels, cs, n_crops, d_out, out_offsets, staging_bytes, stream);
        });
}

// ... qoimi_decode_resized: the bands are those of the items' SOURCE rectangles.
extern "C" int qoimi_decode_resized_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                            int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                            size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                            const size_t* point_firsts) {
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (const int rc = check_out_channels(channels)) return rc;
    if (const int rc = check_resize_mode(mode)) return rc;
    const size_t n = (size_t)n_items;
    return run_indexed(c, d_streams, stream_offsets, sizes, descs, n_images, items, n, interval_rows, points, point_firsts, stream,
        [&](CheckedItems& ok) { return check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, resize_item_wrong, resize_bytes, ok); },
        [&](const void* bands, const size_t* at, const int* sz, const qoi_desc* ds, int m, const qoimi_resize* rs) {
            return qoimi_decode_resized(c, bands, at, sz, ds, m, channels, rs, n_items, mode, d_out, out_offsets, staging_bytes, stream);
        });
}

// ... qoimi_decode_bilinear likewise.
extern "C" int qoimi_decode_bilinear_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                             int n_images, int channels, const qoimi_resize* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                             size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                             const size_t* point_firsts) {
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (const int rc = check_out_channels(channels)) return rc;
    if (const int rc = check_resize_mode(mode)) return rc;
    const size_t n = (size_t)n_items;
    return run_indexed(c, d_streams, stream_offsets, sizes, descs, n_images, items, n, interval_rows, points, point_firsts, stream,
        [&](CheckedItems& ok) { return check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, bilinear_item_wrong, resize_bytes, ok); },
        [&](const void* bands, const size_t* at, const int* sz, const qoi_desc* ds, int m, const qoimi_resize* rs) {
            return qoimi_decode_bilinear(c, bands, at, sz, ds, m, channels, rs, n_items, mode, d_out, out_offsets, staging_bytes, stream);
        });
}

// ... qoimi_decode_warped likewise (the map is relative to the rectangle: only `image` and y change).
extern "C" int qoimi_decode_warped_indexed(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                           int n_images, int channels, const qoimi_warp* items, int n_items, int mode, void* d_out, const size_t* out_offsets,
                                           size_t staging_bytes, void* stream, const unsigned* interval_rows, const qoimi_seek_point* points,
                                           const size_t* point_firsts) {
    if (!c || !d_streams || !stream_offsets || !sizes || !descs || !items || !d_out || !out_offsets || !interval_rows || !points || !point_firsts ||
        n_images <= 0 || n_items <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (const int rc = check_out_channels(channels)) return rc;
    if (const int rc = check_resize_mode(mode)) return rc;
    const size_t n = (size_t)n_items;
    return run_indexed(c, d_streams, stream_offsets, sizes, descs, n_images, items, n, interval_rows, points, point_firsts, stream,
        [&](CheckedItems& ok) { return check_items("item", sizes, descs, n_images, channels, items, n, d_out, out_offsets, warp_item_wrong, warp_bytes, ok); },
        [&](const void* bands, const size_t* at, const int* sz, const qoi_desc* ds, int m, const qoimi_warp* rs) {
            return qoimi_decode_warped(c, bands, at, sz, ds, m, channels, rs, n_items, mode, d_out, out_offsets, staging_bytes, stream);
        });
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
    return run_indexed(c, d_streams, stream_offsets, sizes, descs, n_images, regions, n, interval_rows, points, point_firsts, stream,
        [&](CheckedItems& ok) { return check_regions(sizes, descs, n_images, regions, n, ok); },
        [&](const void* bands, const size_t* at, const int* sz, const qoi_desc* ds, int m, const qoimi_crop* rs) {
            return qoimi_pixel_stats(c, bands, at, sz, ds, m, rs, n_regions, stats_out, d_hist, staging_bytes, stream);
        });
}

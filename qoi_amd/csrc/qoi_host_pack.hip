// qoi_host_pack.hip — packs of streams in the C-ABI shim: qoimi_pack_streams, qoimi_encode_packed / qoimi_encode_images_packed,
// qoimi_encode_tiles / qoimi_tile_size / qoimi_tile_pyramid, qoimi_read_descs, qoimi_inspect_streams.
#include "qoi_ctx.h"
#include "qoi_ingest_core.h"
#include "qoi_label_core.h"
#include "qoi_tile_core.h"

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
    if (const int rc = timer_room(c, st)) return rc;
    launch_pack_streams((const uint8_t*)d_streams, stream_stride, d_stream_len, (uint32_t)n_streams, align, (uint8_t*)d_packed, packed_capacity,
                        (u64*)d_packed_off, grid_bound(c, ~0ull), st, &c->timer);
    HIP_TRY(hipGetLastError());
    return QOIMI_OK;
}

// ------------------------------------------------------------------------------------
// encode into a pack through bounded staging
// ------------------------------------------------------------------------------------
// (the sub-batch plan: qoi_stage_plan.h: stage_plan)
// What a call's sub-batches are encoded from: the caller's pixels as the entry points take them (pixel_offsets == nullptr: image i at
// i * pixel_stride, descs holds one descriptor; else n_images of each) - or, px_part != nullptr (qoimi_encode_tiles), images that the
// call itself puts into the staging: image i's pixels then stand at the front of its slot, px_part[i] bytes (a multiple of 256), and
// its stream goes behind them.  extra: bytes of a table of the call's own that travels with the source offsets (256-aligned behind
// them in the pinned staging and in the arena).
struct PackPixels { const void* d_pixels; size_t pixel_stride; const size_t* pixel_offsets; const qoi_desc* descs; const size_t* px_part; size_t extra; };

// The loop both calls share.  slots, plan: the staging slot of every image and stage_plan over them.  begin(pinned table, its copy's
// address on the device) fills the call's own table before it is sent; front(k, first, m, staging, stream) runs in front of sub-batch
// k's encoder - images [first, first + m) - on the caller's stream.  Then every sub-batch is one call of the encoder as it is into the
// staging arena, qoimi_encode_status (which waits for it and encodes it again order-free if a placement wait gave up: the pack never takes
// bytes of a sub-batch whose status has not been looked at), then the append scan and copy on the caller's stream; the next sub-batch's
// front and encoder are ordered behind that copy by the stream.
template <class Begin, class Front>
static int encode_packed(qoimi_ctx* c, const PackPixels& px, int n_images, const std::vector<size_t>& slots, const StagePlan& plan,
                         unsigned align, void* d_packed, size_t packed_capacity, unsigned long long* d_packed_off, int* d_stream_len,
                         unsigned long long* packed_off_out, int* stream_len_out, void* stream, Begin begin, Front front) {
    const bool staged = px.px_part != nullptr, mixed = staged || px.pixel_offsets != nullptr;
    const size_t n = (size_t)n_images;
    size_t largest = 0;
    for (size_t i = 0; i < n; ++i) if (slots[i] > largest) largest = slots[i];
    const std::vector<int>& firsts = plan.firsts;
    std::vector<size_t> src(plan.at);                        // where stream i lies in the staging of its sub-batch
    if (staged) for (size_t i = 0; i < n; ++i) src[i] += px.px_part[i];
    const size_t need = plan.need;
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    const size_t table_bytes = (mixed ? up256(n * sizeof(u64)) : 0) + px.extra;
    { int rc = c->enc_stage.reserve(table_bytes + need); if (rc) return rc; }
    { int rc = c->pin.reserve(std::max(table_bytes, (n + 1u) * sizeof(u64) + n * sizeof(int)) + 256u); if (rc) return rc; }
    u64* const d_src = mixed ? (u64*)c->enc_stage.base : nullptr;
    uint8_t* const staging = (uint8_t*)c->enc_stage.base + table_bytes;
    if (mixed) {                                             // where stream j lies in the staging of its sub-batch: one table for the whole call
        for (size_t i = 0; i < n; ++i) ((u64*)c->pin.buf)[i] = (u64)src[i];
        if (px.extra != 0u) { const int rc = begin((uint8_t*)c->pin.buf + (table_bytes - px.extra), (uint8_t*)c->enc_stage.base + (table_bytes - px.extra)); if (rc) return rc; }
        HIP_TRY(hipMemcpyAsync(d_src, c->pin.buf, px.extra != 0u ? table_bytes : n * sizeof(u64), hipMemcpyHostToDevice, st));
    }
    int rc = QOIMI_OK;
    for (size_t k = 0; k + 1 < firsts.size() && rc == QOIMI_OK; ++k) {
        const int first = firsts[k], m = firsts[k + 1] - first;
        size_t span = 0;
        for (int i = first; i < first + m; ++i) span += slots[(size_t)i] - (staged ? px.px_part[(size_t)i] : 0u);
        rc = front(k, first, m, staging, st);
        if (rc != QOIMI_OK) break;
        rc = staged ? qoimi_encode_images(c, staging, plan.at.data() + first, px.descs + first, m, staging, src.data() + first, d_stream_len + first, stream)
           : mixed  ? qoimi_encode_images(c, px.d_pixels, px.pixel_offsets + first, px.descs + first, m, staging, src.data() + first, d_stream_len + first, stream)
                    : qoimi_encode_batch(c, (const uint8_t*)px.d_pixels + (size_t)first * px.pixel_stride, px.pixel_stride, px.descs, m, staging, largest, d_stream_len + first, stream);
        if (rc == QOIMI_OK) rc = qoimi_encode_status(c, stream);
        if (rc != QOIMI_OK) break;
        if (const int full = timer_room(c, st)) return full;
        // (a stream is no longer than its slot and align is at most 256, so the sub-batch takes no more of the pack than `span` bytes:
        // that many tiles, one more for where the range begins in its first tile and one for the destination's own alignment)
        const size_t tiles = span / kPackTile + 3u;
        launch_pack_append(staging, largest, d_src, d_stream_len, (uint32_t)first, (uint32_t)m, align, (uint8_t*)d_packed, packed_capacity,
                           (u64*)d_packed_off, grid_bound(c, tiles), st, &c->timer);
        if (hipGetLastError() != hipSuccess) rc = fail(QOIMI_E_INTERNAL, "launch of the pack's append kernels failed");
    }
    // whatever happened, qoimi_encode_status must not encode "the last call" again: it went into staging
    c->last_enc.valid = false; c->last_enc_err = nullptr; c->last_enc_err2 = nullptr;
    if (rc != QOIMI_OK) { (void)hipStreamSynchronize(st); return rc; }
    u64* const h_off = (u64*)c->pin.buf; int* const h_len = (int*)(h_off + n + 1u);
    HIP_TRY(hipMemcpyAsync(h_off, d_packed_off, (n + 1u) * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_len, d_stream_len, n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (packed_off_out) memcpy(packed_off_out, h_off, (n + 1u) * sizeof(u64));
    if (stream_len_out) memcpy(stream_len_out, h_len, n * sizeof(int));
    return QOIMI_OK;
}

// Both entry points of the caller's own pixels: descs holds one descriptor (pixel_offsets == nullptr) or n_images of them; a slot is the
// image's encode bound rounded up to 256.
static int encode_packed(qoimi_ctx* c, const void* d_pixels, size_t pixel_stride, const size_t* pixel_offsets, const qoi_desc* descs, int n_images,
                         unsigned align, void* d_packed, size_t packed_capacity, unsigned long long* d_packed_off, int* d_stream_len,
                         size_t staging_bytes, unsigned long long* packed_off_out, int* stream_len_out, void* stream) {
    std::vector<size_t> slots((size_t)n_images);
    for (size_t i = 0; i < slots.size(); ++i) slots[i] = up256(qoimi_encode_bound(&descs[pixel_offsets ? i : 0]));
    const StagePlan plan = stage_plan(slots, staging_bytes);
    const PackPixels px = {d_pixels, pixel_stride, pixel_offsets, descs, nullptr, 0u};
    return encode_packed(c, px, n_images, slots, plan, align, d_packed, packed_capacity, d_packed_off, d_stream_len, packed_off_out, stream_len_out, stream,
                         [](uint8_t*, uint8_t*) { return (int)QOIMI_OK; }, [](size_t, int, int, uint8_t*, hipStream_t) { return (int)QOIMI_OK; });
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

// ------------------------------------------------------------------------------------
// tiles and pyramid levels of device images as a pack (qoi_tile.hip)
// ------------------------------------------------------------------------------------
static_assert(sizeof(qoimi_tile) == 32 && offsetof(qoimi_tile, image) == 0 && offsetof(qoimi_tile, x) == 4 && offsetof(qoimi_tile, y) == 8 &&
              offsetof(qoimi_tile, width) == 12 && offsetof(qoimi_tile, height) == 16 && offsetof(qoimi_tile, factor) == 20 &&
              offsetof(qoimi_tile, flags) == 24 && offsetof(qoimi_tile, reserved) == 28, "qoimi_tile layout");
static_assert(QOIMI_CROP_FLIP_X == (int)kCropFlipX && QOIMI_CROP_FLIP_Y == (int)kCropFlipY, "the table's flag bits");
static_assert(QOIMI_TILE_NEAREST == 4 && QOIMI_TILE_MODE == 5 && kTileModeMaxFactor == 16u, "2 and 3 are not modes; a block votes over at most 16 x 16 pixels");
static_assert(QOIMI_TILE_SRC == (int)kTileSrc && QOIMI_TILE_SRC_CHW == (int)kTileSrcCHW && QOIMI_TILE_SRC_F16 == (int)(kIngestF16 << kTileSrcDtypeShift) &&
              QOIMI_TILE_SRC_BF16 == (int)(kIngestBF16 << kTileSrcDtypeShift) && QOIMI_TILE_SRC_F32 == (int)(kIngestF32 << kTileSrcDtypeShift) &&
              QOIMI_TILE_SRC_SYMMETRIC == (int)(kIngestSymmetric << kTileSrcRangeShift) && QOIMI_TILE_SRC_BYTES == (int)(kIngestBytes << kTileSrcRangeShift) &&
              (int)kIngestU8 == QOIMI_TENSOR_U8 && (int)kIngestF16 == QOIMI_TENSOR_F16 && (int)kIngestBF16 == QOIMI_TENSOR_BF16 && (int)kIngestF32 == QOIMI_TENSOR_F32,
              "the source format's bits: the dtype field holds QOIMI_TENSOR_U8 .. _F32");
static_assert(QOIMI_TILE_LABELS == (int)kTileLabels && QOIMI_TILE_LABELS_I32 == (int)(kLabelI32 << kTileLabelsDtypeShift) &&
              QOIMI_TILE_LABELS_I64 == (int)(kLabelI64 << kTileLabelsDtypeShift) && kTileLabelsMask == 0x3800u && (kTileLabelsMask & kTileSrcMask) == 0u,
              "the label source's bits: 11, and the dtype field in 12-13; bit 10 stays an unknown flag bit");
static_assert(QOIMI_TILE_LABELS_ID24 == (int)kTileLabelsId24 && kTileLabelsId24 == 1u << 15 && (kTileLabelsId24 & (kTileLabelsMask | kTileSrcMask)) == 0u && (kLabelId24 & 3u) == 0u,
              "24-bit ids: bit 15, beside the dtype field; bit 14 stays an unknown flag bit");

// nullptr if the tile is fine for an accepted descriptor, else what is wrong with it
static const char* tile_wrong(const qoi_desc* d, const qoimi_tile* t) {
    if (t->width == 0u || t->height == 0u) return "zero width or height";
    if ((uint64_t)t->x + t->width > d->width || (uint64_t)t->y + t->height > d->height) return "the rectangle leaves its image";
    if (t->factor < 1u || t->factor > kThumbMaxFactor) return "factor outside 1..64";
    if ((t->flags & ~((unsigned)(QOIMI_CROP_FLIP_X | QOIMI_CROP_FLIP_Y) | kTileSrcMask | kTileLabelsMask | kTileLabelsId24)) != 0u) return "unknown flag bit";
    if (t->reserved != 0u) return "reserved is not 0";
    return nullptr;
}

// ... and of its source format (QOIMI_TILE_SRC*), looked at behind everything else of the tile
static const char* tile_src_wrong(const qoimi_tile* t) {
    const uint32_t src = t->flags & kTileSrcMask;
    if (src == 0u) return nullptr;
    if ((src & kTileSrc) == 0u) return "a QOIMI_TILE_SRC_* bit without QOIMI_TILE_SRC";
    if (ingest_range(src) == 3u) return "768 is not a range of a tensor source";
    if (ingest_range(src) != kIngestUnit && ingest_dtype(src) == kIngestU8) return "a range with a u8 tensor source (the byte is the element)";
    if (t->factor != 1u) return "a tensor source (QOIMI_TILE_SRC) takes factor 1 only";
    return nullptr;
}

// ... and of its label source (QOIMI_TILE_LABELS*), looked at behind those; averaging: the call's mode is one of the two box averages
static const char* tile_label_wrong(const qoimi_tile* t, bool averaging) {
    const uint32_t lab = t->flags & (kTileLabelsMask | kTileLabelsId24);
    if (lab == 0u) return nullptr;
    if ((lab & kTileLabels) == 0u) return "a QOIMI_TILE_LABELS_* bit without QOIMI_TILE_LABELS";
    if (label_dtype(lab) == 3u) return "12288 is not a dtype of a label source";
    if ((t->flags & kTileSrcMask) != 0u) return "QOIMI_TILE_LABELS together with a QOIMI_TILE_SRC bit (a source is a tensor or a label plane)";
    if (averaging && t->factor != 1u) return "a label source is never averaged: factor != 1 takes QOIMI_TILE_NEAREST or QOIMI_TILE_MODE";
    return nullptr;
}

extern "C" size_t qoimi_tile_size(const qoi_desc* desc, const qoimi_tile* tile, int channels, unsigned* tw, unsigned* th) {
    if (!desc_ok(desc) || !tile || (channels != 0 && channels != 3 && channels != 4) || tile_wrong(desc, tile) || tile_src_wrong(tile) || tile_label_wrong(tile, false)) return 0;
    const uint32_t x = thumb_extent(tile->width, tile->factor), y = thumb_extent(tile->height, tile->factor);
    if (tw) *tw = x;
    if (th) *th = y;
    return (size_t)x * y * (size_t)(channels ? channels : desc->channels);
}

extern "C" int qoimi_tile_pyramid(const qoi_desc* desc, unsigned tile_w, unsigned tile_h, unsigned levels, qoimi_tile* out, int cap) {
    if (!desc_ok(desc)) return fail(QOIMI_E_ARG, "descriptor rejected (qoi.h:364-372 rules)");
    if (tile_w == 0u || tile_h == 0u || tile_w > (1u << 24) || tile_h > (1u << 24)) return fail(QOIMI_E_ARG, "tile_w and tile_h must be 1..2^24");
    if (levels < 1u || levels > 7u) return fail(QOIMI_E_ARG, "levels must be 1..7");
    uint64_t total = 0;
    for (unsigned l = 0; l < levels; ++l) {
        const uint32_t f = 1u << l;
        total += (uint64_t)thumb_extent(thumb_extent(desc->height, f), tile_h) * thumb_extent(thumb_extent(desc->width, f), tile_w);
    }
    if (total > 0x7FFFFFFFull) return fail(QOIMI_E_ARG, "more than 2^31 - 1 tiles");
    if (!out) return (int)total;
    if (cap < 0 || (uint64_t)cap < total) return fail(QOIMI_E_ARG, "cap is smaller than the number of tiles");
    qoimi_tile* t = out;
    for (unsigned l = 0; l < levels; ++l) {
        const uint32_t f = 1u << l, sw = tile_w * f, sh = tile_h * f;        // (2^24 * 64: the source side of a tile fits 32 bits)
        const uint32_t rows = thumb_extent(thumb_extent(desc->height, f), tile_h), cols = thumb_extent(thumb_extent(desc->width, f), tile_w);
        for (uint32_t r = 0; r < rows; ++r)
            for (uint32_t col = 0; col < cols; ++col, ++t) {
                t->image = 0u; t->x = col * sw; t->y = r * sh;               // (both inside the image: col * tile_w < ceil(w / f))
                t->width = desc->width - t->x < sw ? desc->width - t->x : sw;
                t->height = desc->height - t->y < sh ? desc->height - t->y : sh;
                t->factor = f; t->flags = 0u; t->reserved = 0u;
            }
    }
    return (int)total;
}

// Tile j's slot: up256 of its pixels, then up256 of its encode bound; sub-batches by stage_plan over those slots in tile order
// (qoi_amd/tiles.py: plan).  Every sub-batch: one launch of tile_gather - of tile_select in QOIMI_TILE_NEAREST / QOIMI_TILE_MODE, which
// change the reduction and the count of work items, no size - over its tiles, then the loop of encode_packed as it is.  A tensor call
// (every tile carries QOIMI_TILE_SRC) runs tensor_ingest in their place: a third kind of entry, factor 1 only, the same table and plan.
// A label call (every tile carries QOIMI_TILE_LABELS) runs label_ingest: one-plane integer sources, copied or reduced by the two label modes.
extern "C" int qoimi_encode_tiles(qoimi_ctx* c, const void* d_pixels, const size_t* pixel_offsets, const qoi_desc* descs, int n_images, int channels,
                                  const qoimi_tile* tiles, int n_tiles, int mode, unsigned align, void* d_packed, size_t packed_capacity,
                                  unsigned long long* d_packed_off, int* d_stream_len, size_t staging_bytes, unsigned long long* packed_off_out,
                                  int* stream_len_out, qoi_desc* tile_descs_out, void* stream) {
    // (everything is looked at before the context is: a rejected call launches nothing and leaves the caller's buffers as they were)
    if (!c || !d_pixels || !pixel_offsets || !descs || !tiles || !d_packed_off || !d_stream_len || n_images <= 0 || n_tiles <= 0 ||
        (!d_packed && packed_capacity != 0)) return fail(QOIMI_E_ARG, "NULL/empty argument");
    if (align == 0 || align > 256u || (align & (align - 1u)) != 0) return fail(QOIMI_E_ARG, "align must be a power of two, 1..256");
    if (const int rc = check_out_channels(channels)) return rc;
    if (mode != QOIMI_THUMB_PLAIN && mode != QOIMI_THUMB_ALPHA_WEIGHTED && mode != QOIMI_TILE_NEAREST && mode != QOIMI_TILE_MODE)
        return fail(QOIMI_E_ARG, "mode must be QOIMI_THUMB_PLAIN, QOIMI_THUMB_ALPHA_WEIGHTED, QOIMI_TILE_NEAREST or QOIMI_TILE_MODE");
    // the kind of every entry of the call's table: the label modes run tile_select, the box filter tile_gather as ever
    uint32_t kind = mode == QOIMI_TILE_NEAREST ? kTileKindNearest : mode == QOIMI_TILE_MODE ? kTileKindMode : kTileKindBox;
    const size_t n = (size_t)n_tiles;
    std::vector<uint8_t> named((size_t)n_images, 0);
    size_t n_src = 0, n_lab = 0;
    for (size_t j = 0; j < n; ++j) {
        const qoimi_tile& t = tiles[j];
        if (t.image >= (unsigned)n_images) return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": no image " + std::to_string(t.image));
        if (!named[t.image]) {                                 // (an image no tile names is never looked at)
            if (!desc_ok(&descs[t.image])) return fail(QOIMI_E_ARG, "descriptor " + std::to_string(t.image) + " rejected (qoi.h:364-372 rules)");
            named[t.image] = 1;
        }
        if (const char* what = tile_wrong(&descs[t.image], &t)) return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": " + what);
        if (kind == kTileKindMode && t.factor > kTileModeMaxFactor)
            return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": factor above 16 with QOIMI_TILE_MODE (a block votes over at most 16 x 16 pixels; QOIMI_TILE_NEAREST has no such limit)");
        if (const char* what = tile_src_wrong(&t)) return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": " + what);
        if (const char* what = tile_label_wrong(&t, mode == QOIMI_THUMB_PLAIN || mode == QOIMI_THUMB_ALPHA_WEIGHTED)) return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": " + what);
        if ((t.flags & kTileSrc) != 0u) ++n_src;
        if ((t.flags & kTileLabels) != 0u) ++n_lab;
    }
    // a call is a byte call or a tensor call; in a tensor call an image has ONE format (its element size: 1 in a byte call)
    if (n_src != 0u && n_src != n) return fail(QOIMI_E_ARG, "some tiles carry QOIMI_TILE_SRC and some do not: a call is a byte call or a tensor call");
    if (n_lab != 0u && n_lab != n) return fail(QOIMI_E_ARG, "some tiles carry QOIMI_TILE_LABELS and some do not: a call is a byte call, a tensor call or a label call");
    std::vector<uint32_t> src_of((size_t)n_images, 0u);
    if (n_src != 0u) {
        kind = kTileKindIngest;                                // (at factor 1 all four modes are the rectangle itself)
        for (size_t j = 0; j < n; ++j) {
            const uint32_t src = tiles[j].flags & kTileSrcMask;
            if (src_of[tiles[j].image] != 0u && src_of[tiles[j].image] != src)
                return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": image " + std::to_string(tiles[j].image) + " is named with two different source formats");
            src_of[tiles[j].image] = src;
        }
        for (size_t i = 0; i < named.size(); ++i)
            if (named[i] && ((uintptr_t)d_pixels + pixel_offsets[i]) % ingest_elem(ingest_dtype(src_of[i])) != 0u)
                return fail(QOIMI_E_ARG, "image " + std::to_string(i) + ": its address is not a multiple of the element size");
    }
    // in a label call an image is ONE plane of elements of one dtype
    const bool labels = n_lab != 0u, vote = mode == QOIMI_TILE_MODE;
    std::vector<uint32_t> lab_of((size_t)n_images, 0u);
    if (labels) {
        kind = kTileKindLabel;
        for (size_t j = 0; j < n; ++j) {
            const uint32_t lab = tiles[j].flags & (kTileLabelsMask | kTileLabelsId24);      // (bit 15 too: an image is bytes or ids)
            if (lab_of[tiles[j].image] != 0u && lab_of[tiles[j].image] != lab)
                return fail(QOIMI_E_ARG, "tile " + std::to_string(j) + ": image " + std::to_string(tiles[j].image) + " is named with two different label dtypes");
            lab_of[tiles[j].image] = lab;
        }
        for (size_t i = 0; i < named.size(); ++i)
            if (named[i] && ((uintptr_t)d_pixels + pixel_offsets[i]) % label_elem(label_dtype(lab_of[i])) != 0u)
                return fail(QOIMI_E_ARG, "image " + std::to_string(i) + ": its address is not a multiple of the element size");
    }
    long long referenced = 0;
    for (size_t i = 0; i < named.size(); ++i) {
        if (!named[i]) continue;
        ++referenced;
        const uintptr_t room = ~(uintptr_t)0 - (uintptr_t)d_pixels;
        const size_t last = labels ? (size_t)descs[i].width * descs[i].height * label_elem(label_dtype(lab_of[i])) - 1u                   // (one plane, whatever channels says)
                                   : (size_t)descs[i].width * descs[i].height * descs[i].channels * ingest_elem(ingest_dtype(src_of[i])) - 1u;     // the image's last byte from its first
        if (pixel_offsets[i] > room || last > room - pixel_offsets[i]) return fail(QOIMI_E_ARG, "image " + std::to_string(i) + " ends behind the address space");
        const uintptr_t s0 = (uintptr_t)d_pixels + pixel_offsets[i], p0 = (uintptr_t)d_packed;
        if (packed_capacity != 0 && s0 <= p0 + (packed_capacity - 1u) && p0 <= s0 + last) return fail(QOIMI_E_ARG, "image " + std::to_string(i) + " and the pack overlap");
    }
    // the tiles' descriptors, slots and plan
    std::vector<qoi_desc> td(n);
    std::vector<size_t> px_part(n), slots(n);
    for (size_t j = 0; j < n; ++j) {
        const qoimi_tile& t = tiles[j];
        const qoi_desc& d = descs[t.image];
        td[j].width = thumb_extent(t.width, t.factor); td[j].height = thumb_extent(t.height, t.factor);
        td[j].channels = (unsigned char)(channels ? channels : d.channels); td[j].colorspace = d.colorspace;
        px_part[j] = up256((size_t)td[j].width * td[j].height * td[j].channels);
        slots[j] = px_part[j] + up256(qoimi_encode_bound(&td[j]));
    }
    const StagePlan plan = stage_plan(slots, staging_bytes);
    std::vector<uint32_t> first_tile(n), sub_tiles(plan.firsts.size() - 1u);
    for (size_t k = 0; k + 1 < plan.firsts.size(); ++k) {
        uint64_t sum = 0;
        for (int j = plan.firsts[k]; j < plan.firsts[k + 1]; ++j) {
            if (sum >= 0x7FFFFFFFull) break;
            first_tile[(size_t)j] = (uint32_t)sum;
            sum += kind == kTileKindLabel ? label_tiles(tiles[j].width, tiles[j].height, tiles[j].factor, vote, td[(size_t)j].channels)
                 : kind == kTileKindIngest ? ingest_tiles(tiles[j].width, tiles[j].height)
                 : kind == kTileKindBox ? tile_tiles(tiles[j].width, tiles[j].height, tiles[j].factor, td[(size_t)j].channels)
                                        : tile_select_tiles(kind, tiles[j].width, tiles[j].height, tiles[j].factor, td[(size_t)j].channels);
        }
        if (sum >= 0x7FFFFFFFull) return fail(QOIMI_E_ARG, "more than 2^31 tiles of work items of the gather kernel in one sub-batch");
        sub_tiles[k] = (uint32_t)sum;
    }
    long long (&stats)[4] = c->tile_stats;
    stats[0] = 0; stats[1] = 0; stats[2] = (long long)plan.need; stats[3] = referenced;
    const TileEntry* d_tab = nullptr;
    const PackPixels px = {d_pixels, 0, nullptr, td.data(), px_part.data(), up256(n * sizeof(TileEntry))};
    const int rc = encode_packed(c, px, n_tiles, slots, plan, align, d_packed, packed_capacity, d_packed_off, d_stream_len, packed_off_out, stream_len_out, stream,
        [&](uint8_t* h_extra, uint8_t* d_extra) {
            TileEntry* tab = (TileEntry*)h_extra;
            for (size_t j = 0; j < n; ++j) {
                const qoimi_tile& t = tiles[j];
                const qoi_desc& d = descs[t.image];
                TileEntry& e = tab[j];
                e.src_off = (u64)pixel_offsets[t.image]; e.dst_off = (u64)plan.at[j];
                e.w = d.width; e.x = t.x; e.y = t.y; e.cw = t.width; e.ch = t.height; e.tw = td[j].width; e.th = td[j].height; e.f = t.factor;
                e.first_tile = first_tile[j];
                if (kind == kTileKindLabel) { e.cfg = label_cfg(t.flags, t.factor, vote, td[j].channels); continue; }
                if (kind == kTileKindIngest) { e.f = d.height; e.cfg = ingest_cfg(t.flags, d.channels, td[j].channels, t.flags); continue; }   // (the factor is 1: f holds the image's height)
                e.cfg = kind == kTileKindBox ? tile_cfg(t.factor, d.channels, td[j].channels, mode == QOIMI_THUMB_ALPHA_WEIGHTED && d.channels == 4u, t.flags)   // with 3 source channels the mode is PLAIN
                                             : tile_select_cfg(kind, t.factor, d.channels, td[j].channels, t.flags);
            }
            d_tab = (const TileEntry*)d_extra;
            return (int)QOIMI_OK;
        },
        [&](size_t k, int first, int m, uint8_t* staging, hipStream_t st) {
            stats[0] += 1;
            (kind == kTileKindLabel ? launch_label_ingest : kind == kTileKindIngest ? launch_tensor_ingest : kind == kTileKindBox ? launch_tile_gather : launch_tile_select)((const uint8_t*)d_pixels, d_tab + first, (uint32_t)m, sub_tiles[k], staging, grid_bound(c, sub_tiles[k]), st);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(QOIMI_E_INTERNAL, std::string(kind == kTileKindLabel ? "label_ingest: " : kind == kTileKindIngest ? "tensor_ingest: " : kind == kTileKindBox ? "tile_gather: " : "tile_select: ") + hipGetErrorString(e));
            stats[1] += 1;
            return (int)QOIMI_OK;
        });
    if (rc == QOIMI_OK && tile_descs_out) memcpy(tile_descs_out, td.data(), n * sizeof(qoi_desc));
    return rc;
}

extern "C" int qoimi_read_descs(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, int n_streams,
                                qoi_desc* descs_out, int* first_bad, void* stream) {
    if (!c || !d_streams || !stream_offsets || !sizes || !descs_out || n_streams <= 0) return fail(QOIMI_E_ARG, "NULL/empty argument");
    DeviceGuard guard(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    // offsets in, header bytes out: both through the context's pinned staging, which the kernel reads and writes in place
    const size_t n = (size_t)n_streams, bytes = n * (sizeof(u64) + 16u) + 256u;
    if (const int rc = c->pin.reserve(bytes)) return rc;
    u64* offs = (u64*)c->pin.buf;
    uint8_t* hdr = (uint8_t*)c->pin.buf + ((n * sizeof(u64) + 255u) & ~(size_t)255u);
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
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    if (const int rc = timer_room(c, st)) return rc;
    // pinned staging: [stream table][block table] go to the device, [results][header + trailer bytes] are written by inspect_reduce in place
    const size_t tab_bytes = up256(n * sizeof(InsStream)) + up256(nb * sizeof(InsBlock));
    const size_t bytes = tab_bytes + up256(n * sizeof(InsResult)) + up256(n * 32u);
    if (const int rc = c->pin.reserve(bytes)) return rc;
    uint8_t* pin = (uint8_t*)c->pin.buf;
    InsStream* h_tab = (InsStream*)pin;
    InsBlock* h_blk = (InsBlock*)(pin + up256(n * sizeof(InsStream)));
    InsResult* h_res = (InsResult*)(pin + tab_bytes);
    const uint8_t* h_raw = pin + tab_bytes + up256(n * sizeof(InsResult));
    ins_fill_tables(stream_offsets, sizes, n, h_tab, h_blk);
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
    launch_inspect((const uint8_t*)d_streams, (const InsStream*)d_tab, (uint32_t)n, (const InsBlock*)(d_tab + up256(n * sizeof(InsStream))), (uint32_t)nb,
                   d_map, d_entry, d_piece, d_part, h_res, (uint32_t*)(pin + tab_bytes + up256(n * sizeof(InsResult))), st, &c->timer);
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

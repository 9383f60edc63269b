// qoi_host_pack.hip — packs of streams in the C-ABI shim: qoimi_pack_streams, qoimi_encode_packed / qoimi_encode_images_packed,
// qoimi_read_descs, qoimi_inspect_streams.
#include "qoi_ctx.h"

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
    if (const int rc = wait_decode_tail(c, stream)) return rc;
    const size_t table_bytes = mixed ? (n * sizeof(u64) + 255u) & ~(size_t)255u : 0;
    { int rc = c->enc_stage.reserve(table_bytes + need); if (rc) return rc; }
    { int rc = c->pin.reserve((n + 1u) * sizeof(u64) + n * sizeof(int) + 256u); if (rc) return rc; }
    u64* const d_src = mixed ? (u64*)c->enc_stage.base : nullptr;
    uint8_t* const staging = (uint8_t*)c->enc_stage.base + table_bytes;
    if (mixed) {                                             // where stream j lies in the staging of its sub-batch: one table for the whole call
        for (size_t i = 0; i < n; ++i) ((u64*)c->pin.buf)[i] = (u64)src[i];
        HIP_TRY(hipMemcpyAsync(d_src, c->pin.buf, n * sizeof(u64), hipMemcpyHostToDevice, st));
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

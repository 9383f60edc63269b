// qoi_host_decode.hip — the decode calls of the C-ABI shim: qoimi_decode_batch, qoimi_decode_images and what they share.
#include "qoi_ctx.h"
#include "qoi_decode_core.h"

#include <algorithm>
#include <numeric>

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
    if (const int rc = wait_decode_tail(c, stream)) return rc;
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
        if (const int rc = c->pin.reserve(bytes)) return rc;
        memset(c->pin.buf, 0, 256);
        memcpy((uint8_t*)c->pin.buf + 256, imgs.data(), bytes - 256u);
        HIP_TRY(hipMemcpyAsync(p.pending, c->pin.buf, bytes, hipMemcpyHostToDevice, st));
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
    if (const int rc = check_out_channels(channels)) return rc;
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
    if (const int rc = check_out_channels(channels)) return rc;
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

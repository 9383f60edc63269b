// qoi_host_encode.hip — the encode calls of the C-ABI shim: qoimi_encode_batch, qoimi_encode_images, qoimi_encode_status.
#include "qoi_ctx.h"

#include <type_traits>

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
    enc_poll_recheck(c, true);
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
    if (const int rc = timer_room(c, st)) return rc;
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
    enc_poll_recheck(c, false);
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
                memcpy((uint8_t*)c->enc_pin.buf + pin_off, tab.data(), tbytes);
                HIP_TRY(hipMemcpyAsync(d_tab, (uint8_t*)c->enc_pin.buf + pin_off, tbytes, hipMemcpyHostToDevice, st));
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
            rc = c->enc_pin.reserve(need); if (rc) return rc;
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

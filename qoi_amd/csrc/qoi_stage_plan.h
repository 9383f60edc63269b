// qoi_stage_plan.h — the host-side plans of the calls that work through bounded staging (qoimi_encode_packed, qoimi_verify_images,
// qoimi_decode_thumbnails, qoimi_decode_crops, qoimi_decode_resized): sub-batches over 256-aligned slots, the rows of the images that are
// decoded, the order of the table entries and their tiles, the overlap check of the output ranges.  Integer arithmetic over vectors and
// nothing else - no HIP, no context - so that tests/host/plan_host.cpp compiles it with g++ and tests/test_stage_plan_host.py compares it
// with the Python statements (qoi_amd/packplan.py: plan, qoi_amd/crops.py: plan) without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace qoimi {

static inline size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// The staging a call takes when the caller passes 0.
static const size_t kPackStagingDefault = (size_t)1 << 30;

// The sub-batch plan (normative; qoi_amd/packplan.py: plan states it in Python): a slot is an image's bytes rounded up to 256, images are
// taken in order, a sub-batch closes when the next slot would not fit in staging_bytes - but never empty: a slot larger than the request is
// a sub-batch of its own.  Returns the first image of every sub-batch and, behind the last one, n.
static inline std::vector<int> pack_plan(const std::vector<size_t>& slots, size_t staging_bytes) {
    std::vector<int> firsts(1, 0);
    size_t used = 0;
    for (size_t i = 0; i < slots.size(); ++i) {
        if ((int)i > firsts.back() && (slots[i] > staging_bytes || used > staging_bytes - slots[i])) { firsts.push_back((int)i); used = 0; }
        used += slots[i];
    }
    firsts.push_back((int)slots.size());
    return firsts;
}

// firsts: pack_plan; at: every slot's offset within its sub-batch; need: the largest sub-batch.  staging_bytes 0: kPackStagingDefault.
struct StagePlan { std::vector<int> firsts; std::vector<size_t> at; size_t need = 0; };
static inline StagePlan stage_plan(const std::vector<size_t>& slots, size_t staging_bytes) {
    StagePlan p;
    p.firsts = pack_plan(slots, staging_bytes ? staging_bytes : kPackStagingDefault);
    p.at.resize(slots.size());
    for (size_t k = 0; k + 1 < p.firsts.size(); ++k) {
        size_t used = 0;
        for (int i = p.firsts[k]; i < p.firsts[k + 1]; ++i) { p.at[(size_t)i] = used; used += slots[(size_t)i]; }
        if (used > p.need) p.need = used;
    }
    return p;
}

// true if two of the output ranges [offsets[j], + bytes[j]) overlap
static inline bool ranges_overlap(const size_t* offsets, const std::vector<size_t>& bytes) {
    const size_t n = bytes.size();
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return offsets[a] < offsets[b]; });
    for (size_t k = 1; k < n; ++k) {
        const size_t a = order[k - 1], b = order[k];
        if (offsets[b] - offsets[a] < bytes[a]) return true;   // (sorted: the difference cannot wrap)
    }
    return false;
}

// The plan of qoi_amd/crops.py: plan.  rows[i]: the rows of image i that are decoded, 0: no item names it (qoimi_decode_thumbnails: every
// image at its full height).  refs: the referenced images, ascending; ref_of: image -> index into refs or -1; slots: width * rows * 4 rounded
// up to 256; firsts, at, need: stage_plan over the slots, as indices into refs.  Desc: anything with a `width`.
struct RowsPlan : StagePlan { std::vector<int> refs, ref_of; std::vector<size_t> slots; };
template <class Desc>
static inline RowsPlan plan_rows(const Desc* descs, int n_images, const std::vector<uint32_t>& rows, size_t staging_bytes) {
    RowsPlan p;
    p.ref_of.assign((size_t)n_images, -1);
    for (int i = 0; i < n_images; ++i) if (rows[(size_t)i] != 0u) { p.ref_of[(size_t)i] = (int)p.refs.size(); p.refs.push_back(i); }
    p.slots.resize(p.refs.size());
    for (size_t r = 0; r < p.refs.size(); ++r) p.slots[r] = up256((size_t)descs[p.refs[r]].width * rows[(size_t)p.refs[r]] * 4u);
    static_cast<StagePlan&>(p) = stage_plan(p.slots, staging_bytes);
    return p;
}

// The table of a call: one entry per item, the entries of a sub-batch together - by_ref[e] is the item of entry e: the items in the order
// of their images' sub-batches, otherwise as the caller gave them - and the tiles of a sub-batch's entries counted from 0: first_tile[e].
// image_of[j]: the image item j names (a referenced one); tiles_of[j]: its tiles.  overflow: a sub-batch holds 2^31 - 1 tiles or more (looked
// at before an item is added and behind the sub-batch: no first_tile is ever cut to 32 bits); the rest is then not to be used.
struct ItemSub { uint32_t entry, m, tiles; };
struct ItemPlan { std::vector<size_t> by_ref; std::vector<ItemSub> subs; std::vector<uint32_t> first_tile; bool overflow = false; };
static inline ItemPlan plan_items(const std::vector<uint32_t>& image_of, const std::vector<int>& ref_of, const std::vector<int>& firsts,
                                  const std::vector<uint64_t>& tiles_of) {
    const size_t n = image_of.size();
    ItemPlan p;
    p.by_ref.resize(n); p.first_tile.resize(n); p.subs.resize(firsts.size() - 1u);
    std::iota(p.by_ref.begin(), p.by_ref.end(), (size_t)0);
    std::stable_sort(p.by_ref.begin(), p.by_ref.end(), [&](size_t a, size_t b) { return ref_of[image_of[a]] < ref_of[image_of[b]]; });
    size_t e = 0;
    for (size_t k = 0; k + 1 < firsts.size(); ++k) {
        uint64_t tiles = 0;
        p.subs[k].entry = (uint32_t)e;
        for (; e < n && ref_of[image_of[p.by_ref[e]]] < firsts[k + 1]; ++e) {
            if (tiles >= 0x7FFFFFFFull) { p.overflow = true; return p; }
            p.first_tile[e] = (uint32_t)tiles;
            tiles += tiles_of[p.by_ref[e]];
        }
        if (tiles >= 0x7FFFFFFFull) { p.overflow = true; return p; }
        p.subs[k].m = (uint32_t)(e - p.subs[k].entry); p.subs[k].tiles = (uint32_t)tiles;
    }
    return p;
}

}  // namespace qoimi

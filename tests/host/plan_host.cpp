// plan_host.cpp — the host plans of the calls that work through bounded staging (qoi_amd/csrc/qoi_stage_plan.h) behind a C interface, so that
// tests/test_stage_plan_host.py can compare them with the Python statements (qoi_amd/packplan.py, qoi_amd/crops.py) without a GPU.  With
// -DPLAN_HOST_MAIN the same source is a stand-alone program that walks the plans over a grid of inputs and checks what defines them (the test
// builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include <stddef.h>
#include <stdint.h>

#include "../../qoi_amd/csrc/qoi_stage_plan.h"

static_assert(sizeof(size_t) == sizeof(uint64_t), "the interface passes size_t as 64-bit words");

namespace {

struct Width { uint32_t width; };

std::vector<size_t> sizes(const uint64_t* p, int n) { return std::vector<size_t>(p, p + n); }
template <class T, class U> void put(T* out, const std::vector<U>& v) { for (size_t i = 0; i < v.size(); ++i) out[i] = (T)v[i]; }

}  // namespace

extern "C" {

uint64_t plan_host_up256(uint64_t x) { return qoimi::up256((size_t)x); }

// pack_plan as it is (staging_bytes 0 is a very small request here); firsts: room for n + 1.  Returns the entries of firsts.
int plan_host_pack(const uint64_t* slots, int n, uint64_t staging_bytes, int* firsts) {
    const std::vector<int> f = qoimi::pack_plan(sizes(slots, n), (size_t)staging_bytes);
    put(firsts, f);
    return (int)f.size();
}

// stage_plan (staging_bytes 0: the default); firsts: room for n + 1, at: for n.  Returns the entries of firsts.
int plan_host_stage(const uint64_t* slots, int n, uint64_t staging_bytes, int* firsts, uint64_t* at, uint64_t* need) {
    const qoimi::StagePlan p = qoimi::stage_plan(sizes(slots, n), (size_t)staging_bytes);
    put(firsts, p.firsts); put(at, p.at);
    *need = p.need;
    return (int)p.firsts.size();
}

// plan_rows; refs, slots, at: room for n_images, ref_of: n_images, firsts: n_images + 1.  Returns the referenced images; *n_firsts: the
// entries of firsts.
int plan_host_rows(const uint32_t* widths, int n_images, const uint32_t* rows, uint64_t staging_bytes, int* refs, int* ref_of, uint64_t* slots,
                   int* firsts, int* n_firsts, uint64_t* at, uint64_t* need) {
    std::vector<Width> descs((size_t)n_images);
    for (int i = 0; i < n_images; ++i) descs[(size_t)i].width = widths[i];
    const qoimi::RowsPlan p = qoimi::plan_rows(descs.data(), n_images, std::vector<uint32_t>(rows, rows + n_images), (size_t)staging_bytes);
    put(refs, p.refs); put(ref_of, p.ref_of); put(slots, p.slots); put(firsts, p.firsts); put(at, p.at);
    *n_firsts = (int)p.firsts.size();
    *need = p.need;
    return (int)p.refs.size();
}

// plan_items; by_ref, first_tile: room for n, entry, m, tiles: for n_firsts - 1.  Returns 1 if it reports an overflow (the outputs are then
// not written), else 0.
int plan_host_items(const uint32_t* image_of, int n, const int* ref_of, int n_images, const int* firsts, int n_firsts, const uint64_t* tiles_of,
                    uint64_t* by_ref, uint32_t* first_tile, uint32_t* entry, uint32_t* m, uint32_t* tiles) {
    const qoimi::ItemPlan p = qoimi::plan_items(std::vector<uint32_t>(image_of, image_of + n), std::vector<int>(ref_of, ref_of + n_images),
                                                std::vector<int>(firsts, firsts + n_firsts), std::vector<uint64_t>(tiles_of, tiles_of + n));
    if (p.overflow) return 1;
    put(by_ref, p.by_ref); put(first_tile, p.first_tile);
    for (size_t k = 0; k < p.subs.size(); ++k) { entry[k] = p.subs[k].entry; m[k] = p.subs[k].m; tiles[k] = p.subs[k].tiles; }
    return 0;
}

int plan_host_overlap(const uint64_t* offsets, const uint64_t* bytes, int n) {
    const std::vector<size_t> off = sizes(offsets, n);
    return qoimi::ranges_overlap(off.data(), sizes(bytes, n)) ? 1 : 0;
}

}

#ifdef PLAN_HOST_MAIN
#include <stdio.h>

#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// What defines a plan, over every staging from 0 to beyond the sum of the slots: the sub-batches are the slots in order, none is empty, one of
// more than one slot fits the request and would not with the next slot; at is the running sum within a sub-batch and need the largest sum.
static int stage_cases(const std::vector<size_t>& slots, long long& plans) {
    size_t all = 0;
    for (size_t s : slots) all += s;
    for (size_t staging = 0; staging <= all + 512u; staging += 128u) {
        const qoimi::StagePlan p = qoimi::stage_plan(slots, staging);
        const size_t limit = staging ? staging : qoimi::kPackStagingDefault;
        CHECK(p.firsts.size() >= 2u && p.firsts.front() == 0 && p.firsts.back() == (int)slots.size() && p.at.size() == slots.size());
        size_t need = 0;
        for (size_t k = 0; k + 1 < p.firsts.size(); ++k) {
            const int first = p.firsts[k], next = p.firsts[k + 1];
            CHECK(next > first);
            size_t used = 0;
            for (int i = first; i < next; ++i) { CHECK(p.at[(size_t)i] == used); used += slots[(size_t)i]; }
            CHECK(next - first == 1 || used <= limit);
            CHECK(next == (int)slots.size() || used + slots[(size_t)next] > limit);
            if (used > need) need = used;
        }
        CHECK(p.need == need);
        ++plans;
    }
    return 0;
}

int main() {
    long long plans = 0;
    if (stage_cases(std::vector<size_t>(13, 12288u), plans)) return 1;
    if (stage_cases({256u, 24832u, 512u, 3328u, 9472u, 9216u, 9472u, 37120u, 256u}, plans)) return 1;

    // rows: images 1 and 3 are not referenced; items name the others out of order and image 4 twice
    const Width descs[6] = {{64}, {7}, {131}, {9}, {1}, {333}};
    const std::vector<uint32_t> rows = {48, 0, 1, 0, 97, 7};
    const std::vector<uint32_t> image_of = {5, 4, 0, 4, 2, 0};
    for (size_t staging : {(size_t)0, (size_t)1, (size_t)12288, (size_t)13000, (size_t)40000}) {
        const qoimi::RowsPlan p = qoimi::plan_rows(descs, 6, rows, staging);
        CHECK(p.refs == std::vector<int>({0, 2, 4, 5}) && p.ref_of == std::vector<int>({0, -1, 1, -1, 2, 3}));
        CHECK(p.slots == std::vector<size_t>({12288u, 768u, 512u, 9472u}));
        const qoimi::StagePlan s = qoimi::stage_plan(p.slots, staging);
        CHECK(p.firsts == s.firsts && p.at == s.at && p.need == s.need);
        const std::vector<uint64_t> tiles_of = {3, 1, 4, 1, 5, 9};
        const qoimi::ItemPlan it = qoimi::plan_items(image_of, p.ref_of, p.firsts, tiles_of);
        CHECK(!it.overflow && it.by_ref == std::vector<size_t>({2, 5, 4, 1, 3, 0}) && it.subs.size() + 1u == p.firsts.size());
        size_t e = 0;
        for (size_t k = 0; k < it.subs.size(); ++k) {
            CHECK(it.subs[k].entry == e);
            uint64_t t = 0;
            for (uint32_t j = 0; j < it.subs[k].m; ++j, ++e) {
                const int r = p.ref_of[image_of[it.by_ref[e]]];
                CHECK(r >= p.firsts[k] && r < p.firsts[k + 1] && it.first_tile[e] == t);
                t += tiles_of[it.by_ref[e]];
            }
            CHECK(it.subs[k].tiles == t);
        }
        CHECK(e == image_of.size());
        ++plans;
    }

    // the identity map of qoimi_decode_thumbnails, and the tile limit: reached by the last item, by an item before the last one, not reached
    {
        const std::vector<int> ident = {0, 1, 2, 3}, firsts = {0, 3, 4};
        const std::vector<uint32_t> each = {0, 1, 2, 3};
        const qoimi::ItemPlan it = qoimi::plan_items(each, ident, firsts, {2, 1, 1, 7});
        CHECK(!it.overflow && it.subs[0].entry == 0u && it.subs[0].m == 3u && it.subs[0].tiles == 4u && it.subs[1].entry == 3u && it.subs[1].m == 1u && it.subs[1].tiles == 7u);
        CHECK(it.first_tile == std::vector<uint32_t>({0, 2, 3, 0}));
        CHECK(!qoimi::plan_items(each, ident, firsts, {0x7FFFFFF0ull, 7, 7, 0x7FFFFFFEull}).overflow);
        CHECK(qoimi::plan_items(each, ident, firsts, {0x7FFFFFF0ull, 7, 8, 1}).overflow);
        CHECK(qoimi::plan_items(each, ident, firsts, {0x7FFFFFF0ull, 15, 1, 1}).overflow);
        CHECK(qoimi::plan_items(each, ident, firsts, {1, 1, 1, 0x7FFFFFFFull}).overflow);
    }

    // ranges: touching, one byte shared, unsorted, one range, the end of the address space
    {
        const size_t top = ~(size_t)0;
        const size_t a[3] = {100, 0, 40}, b[2] = {top - 15u, 16};
        CHECK(!qoimi::ranges_overlap(a, {28, 40, 60}));
        CHECK(qoimi::ranges_overlap(a, {28, 41, 60}));
        CHECK(qoimi::ranges_overlap(a, {28, 40, 61}));
        CHECK(!qoimi::ranges_overlap(a, {1000}));
        CHECK(!qoimi::ranges_overlap(b, {15, top - 31u}));
        CHECK(qoimi::ranges_overlap(b, {15, top - 30u}));
        CHECK(!qoimi::ranges_overlap(a, {}));
    }
    printf("plan_host: %lld plans ok\n", plans);
    return 0;
}
#endif

// crop_host.cpp — the item arithmetic of qoimi_decode_crops (qoi_amd/csrc/qoi_crop_core.h) compiled for the host: the item loop of crop_gather,
// tile by tile, over a synthetic staging array and the checking memory functor of host_mem.h (StagedMem), so that tests/test_crop_core_host.py
// can compare it with the Python model without a GPU.  With -DCROP_HOST_MAIN the same source is a stand-alone program that walks a grid of
// crops against a plain per-byte loop (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include "../../qoi_amd/csrc/qoi_crop_core.h"
#include "host_mem.h"

extern "C" {

// One crop as crop_gather walks it: stage holds stage_px pixels (rows of w), the output of cw * ch * och bytes begins at out[q - base].
// writes[i] counts the stores to out[i].  Returns the items walked, or -1 - the number of bad accesses if there was one.
long long crop_host_run(const uint32_t* stage, uint64_t stage_px, uint32_t w, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch, uint32_t flags,
                        uint32_t och, uint64_t q, uint64_t base, uint8_t* out, uint8_t* writes, uint64_t out_len) {
    long long bad = 0, walked = 0, loads = 0;                            // (nobody reads the loads: an item loads what it stores)
    const hostmem::StagedMem mem = {{out, writes, out_len, base, &bad}, stage, stage_px, &loads};
    const qoimi::CropRect g = {w, x, y, cw, ch, flags};
    const uint32_t B = cw * ch * och;
    const uint64_t items = qoimi::crop_items(q, B), tiles = qoimi::crop_tiles(q, B);
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint32_t lane = 0; lane < qoimi::kCropThreads; ++lane) {
            const uint64_t k = t * qoimi::kCropThreads + lane;
            if (k >= items) continue;
            if (och == 3u) qoimi::crop_item<3u>(mem, g, q, B, (uint32_t)k);
            else qoimi::crop_item<4u>(mem, g, q, B, (uint32_t)k);
            ++walked;
        }
    return hostmem::checked(bad, walked);
}

unsigned long long crop_host_items(uint64_t q, uint64_t B) { return qoimi::crop_items(q, B); }
unsigned long long crop_host_tiles(uint64_t q, uint64_t B) { return qoimi::crop_tiles(q, B); }

}

#ifdef CROP_HOST_MAIN
#include <stdio.h>

// Every och, alignment, flag value and the small widths and heights, plus one crop of more than 256 items, in arrays of exactly the size the
// walk may touch: the staging ends with the crop's last row, the output with its guard band.
int main() {
    const uint32_t widths[] = {1, 2, 3, 5, 16, 17, 70}, heights[] = {1, 2, 7, 20};
    const uint64_t base = 4096, guard = 32;
    long long crops = 0;
    for (uint32_t och = 3; och <= 4; ++och)
        for (uint32_t a = 0; a < 16; ++a)
            for (uint32_t flags = 0; flags < 4; ++flags)
                for (uint32_t cw : widths)
                    for (uint32_t ch : heights) {
                        if ((cw == 70u) != (ch == 20u)) continue;            // 70 x 20: 4200 / 5600 bytes, more than one tile
                        const uint32_t x = 3, y = 2, w = cw + 5;
                        std::vector<uint32_t> stage((size_t)w * (y + ch));
                        for (size_t i = 0; i < stage.size(); ++i) stage[i] = (uint32_t)(i * 2654435761u + 12345u);
                        const uint32_t B = cw * ch * och;
                        std::vector<uint8_t> out(guard + a + B + guard, hostmem::kGuard), writes(out.size(), 0);
                        const uint64_t q = base + guard + a;
                        const long long rc = crop_host_run(stage.data(), stage.size(), w, x, y, cw, ch, flags, och, q, base, out.data(), writes.data(), out.size());
                        if (rc != (long long)qoimi::crop_items(q, B)) { printf("bad access: och %u a %u flags %u %u x %u: %lld\n", och, a, flags, cw, ch, rc); return 1; }
                        const long long off = hostmem::first_miswritten(out, writes, guard + a, B);
                        if (off >= 0) { printf("byte %lld written %u times\n", off, writes[off]); return 1; }
                        for (uint32_t b = 0; b < B; ++b) {
                            const uint32_t p = b / och, r = p / cw, c = p % cw;
                            const uint32_t sy = (flags & 2u) ? y + ch - 1u - r : y + r, sx = (flags & 1u) ? x + cw - 1u - c : x + c;
                            if (out[guard + a + b] != (uint8_t)(stage[(size_t)sy * w + sx] >> (8u * (b % och)))) { printf("wrong byte %u: och %u a %u flags %u %u x %u\n", b, och, a, flags, cw, ch); return 1; }
                        }
                        ++crops;
                    }
    printf("crop_host: %lld crops ok\n", crops);
    return 0;
}
#endif

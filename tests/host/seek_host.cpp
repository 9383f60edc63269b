// seek_host.cpp — the arithmetic of the row seek index (qoi_amd/csrc/qoi_seek_core.h) compiled for the host: the walk of one 64-byte piece that
// seek_locate runs, and a whole band stream written item by item as band_assemble writes it - over a memory functor that checks every load of
// the tail and every store - so that tests/test_seek_core_host.py can compare both with the Python model (qoi_amd/seekindex.py) without a GPU.
// With -DSEEK_HOST_MAIN the same source is a stand-alone program that writes band streams at every alignment into buffers of exactly their
// size and compares them with a plain sequential writer (the test builds it with -fsanitize=address,undefined and runs it).  Not part of the library.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../qoi_amd/csrc/qoi_seek_core.h"

namespace {

struct HostMem {
    const uint8_t* heads; const uint8_t* tail_bytes; uint32_t tail_len;
    uint8_t* out; uint64_t out_len;          // addresses are offsets into out
    long long* bad;
    uint32_t head(uint32_t i) const { if (i >= qoimi::kSeekHeadMost) { ++*bad; return 0u; } return heads[i]; }
    uint32_t tail1(uint32_t i) const { if (i >= tail_len) { ++*bad; return 0u; } return tail_bytes[i]; }
    void tail16(uint32_t i, uint32_t (&W)[4]) const {
        if ((uint64_t)i + 16u > tail_len) { ++*bad; return; }
        memcpy(W, tail_bytes + i, 16);
    }
    void put(uint64_t a, uint32_t v, uint32_t n, uint32_t align) const {
        if (a % align != 0u || a + n > out_len) { ++*bad; return; }
        for (uint32_t k = 0; k < n; ++k) out[a + k] = (uint8_t)(v >> (8u * k));
    }
    void store1(uint64_t a, uint32_t v) const { put(a, v, 1u, 1u); }
    void store2(uint64_t a, uint32_t v) const { put(a, v, 2u, 2u); }
    void store4(uint64_t a, uint32_t v) const { put(a, v, 4u, 4u); }
    void store16(uint64_t a, const uint32_t (&W)[4]) const { for (uint32_t k = 0; k < 4u; ++k) put(a + 4u * k, W[k], 4u, k == 0u ? 16u : 4u); }
};

}  // namespace

extern "C" {

long long seek_host_points(uint32_t w, uint32_t h, uint32_t K) { return (long long)qoimi::seek_point_count(w, h, K); }

// the piece bytes[0 .. plen) entered at phase p: its pixels; *pos, *before as seek_piece_walk gives them
unsigned seek_host_piece(const uint8_t* bytes, uint32_t plen, uint32_t p, uint32_t target, uint32_t* pos, uint32_t* before) {
    uint32_t d[16];
    uint8_t raw[64];
    memset(raw, 0xEE, sizeof(raw));
    memcpy(raw, bytes, plen);
    memcpy(d, raw, sizeof(raw));
    return qoimi::seek_piece_walk(d, plen, p, target, *pos, *before);
}

// The band stream of `rows` rows that starts at point e (NULL: row 0) with the tail tail[0 .. tail_len), written at out + at item by item.
// Returns its size, -1 - the number of bad loads / stores if there was one, or -1000000 - n for a point with n > 64 loads (nothing is written).  *pad_rows: the rows in front of the band's.
long long seek_host_band(const qoimi::SeekPoint* e, uint32_t w, uint32_t rows, uint32_t channels, uint32_t colorspace, const uint8_t* tail, uint32_t tail_len,
                         uint8_t* out, uint64_t out_len, uint64_t at, uint32_t* pad_rows) {
    long long bad = 0;
    uint8_t head[qoimi::kSeekHeadSlot];
    memset(head, 0, sizeof(head));
    const qoimi::SeekPrefix f = qoimi::seek_prefix_plan(e, w);
    if (f.n > qoimi::kSeekMaxLoads) return -1000000 - (long long)f.n;       // (no point of a stream: the library rejects it before a head is written)
    qoimi::seek_write_head(e, w, f.pad_rows + rows, channels, colorspace, head);
    const uint32_t B = qoimi::seek_prefix_len(f) + tail_len;
    const HostMem mem = {head, tail, tail_len, out, out_len, &bad};
    const uint64_t items = qoimi::crop_items(at, B);
    for (uint64_t k = 0; k < items; ++k) qoimi::seek_band_item(mem, f, at, B, (uint32_t)k);
    if (pad_rows) *pad_rows = f.pad_rows;
    return bad ? -1 - bad : (long long)B;
}

}

#ifdef SEEK_HOST_MAIN
#include <stdio.h>
#include <vector>

int main() {
    long long bands = 0;
    for (uint32_t w : {1u, 2u, 61u, 64u, 129u, 5000u})
        for (uint32_t filled : {0u, 1u, 7u, 64u})
            for (uint32_t skip : {0u, 1u, 61u})
                for (uint32_t tail_len : {8u, 9u, 31u, 32u, 33u, 1000u}) {
                    qoimi::SeekPoint e;
                    memset(&e, 0, sizeof(e));
                    e.byte_off = 14u; e.skip = skip; e.prev = 0x01020304u * (filled + 1u);
                    for (uint32_t s = 0; s < filled; ++s) e.table[(s * 7u) % 64u] = s % 5u == 4u ? e.prev : 0x11000000u + s * 0x01010101u;
                    std::vector<uint8_t> tail(tail_len);
                    for (uint32_t i = 0; i < tail_len; ++i) tail[i] = (uint8_t)(i * 37u + 11u);
                    // the plain writer
                    std::vector<uint8_t> want;
                    uint32_t n = 1;
                    for (uint32_t s = 0; s < 64u; ++s) n += e.table[s] != 0u && e.table[s] != e.prev;
                    uint32_t pad = (n + skip + w - 1u) / w; if (pad == 0u) pad = 1u;
                    const uint32_t R = pad * w - skip - n, height = pad + 3u;
                    const uint8_t hdr[14] = {'q', 'o', 'i', 'f', (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w, 0, 0, (uint8_t)(height >> 8), (uint8_t)height, 4, 1};
                    want.insert(want.end(), hdr, hdr + 14);
                    for (uint32_t s = 0; s <= 64u; ++s) {
                        const uint32_t v = s < 64u ? e.table[s] : e.prev;
                        if (s < 64u && (v == 0u || v == e.prev)) continue;
                        want.push_back(0xFF); for (uint32_t k = 0; k < 4u; ++k) want.push_back((uint8_t)(v >> (8u * k)));
                    }
                    want.insert(want.end(), R / 62u, (uint8_t)0xFD);
                    if (R % 62u) want.push_back((uint8_t)(0xC0u | (R % 62u - 1u)));
                    want.insert(want.end(), tail.begin(), tail.end());
                    for (uint64_t at = 0; at <= 16u; ++at) {
                        std::vector<uint8_t> out(at + want.size(), (uint8_t)0xA5);      // exactly: a store beside the band stream is out of bounds
                        uint32_t pad_rows = 0;
                        const long long rc = seek_host_band(&e, w, 3u, 4u, 1u, tail.data(), tail_len, out.data(), out.size(), at, &pad_rows);
                        if (rc != (long long)want.size() || pad_rows != pad || memcmp(out.data() + at, want.data(), want.size()) != 0) {
                            printf("band differs: w %u filled %u skip %u tail %u at %llu: %lld\n", w, filled, skip, tail_len, (unsigned long long)at, rc);
                            return 1;
                        }
                        for (uint64_t k = 0; k < at; ++k) if (out[k] != 0xA5) { printf("a byte in front was written\n"); return 1; }
                        ++bands;
                    }
                }
    {   // 64 table words that all differ from prev: 65 loads, a head of 339 bytes - refused, nothing written
        qoimi::SeekPoint e;
        memset(&e, 0, sizeof(e));
        e.byte_off = 14u; e.prev = 0x7F7F7F7Fu;
        for (uint32_t s = 0; s < 64u; ++s) e.table[s] = 0x01000000u + s;
        std::vector<uint8_t> tail(8, (uint8_t)0), out(512, (uint8_t)0xA5);
        if (qoimi::seek_prefix_plan(&e, 64u).n != 65u || seek_host_band(&e, 64u, 3u, 4u, 0u, tail.data(), 8u, out.data(), out.size(), 0u, nullptr) != -1000065) {
            printf("a point with 65 loads was not refused\n");
            return 1;
        }
        for (uint8_t b : out) if (b != 0xA5) { printf("a refused point wrote\n"); return 1; }
        e.table[9] = e.prev;                                          // 64 loads: the largest head there is, exactly kSeekHeadMost bytes
        std::vector<uint8_t> full(qoimi::kSeekHeadMost + 1u + 8u, (uint8_t)0xA5);      // + the pad run of 64 - 64 = 0 ... one row of 64: R = 0
        const long long rc = seek_host_band(&e, 64u, 3u, 4u, 0u, tail.data(), 8u, full.data(), full.size(), 0u, nullptr);
        if (qoimi::seek_prefix_plan(&e, 64u).head_len != qoimi::kSeekHeadMost || rc != (long long)qoimi::kSeekHeadMost + 8) { printf("the largest head: %lld\n", rc); return 1; }
    }
    printf("seek_host: %lld bands ok\n", bands);
    return 0;
}
#endif

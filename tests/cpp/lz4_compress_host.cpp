// lz4_compress_host.cpp — the compressor's integer code (spec_amd/csrc/lz4_compress_core.hpp, what
// the kernels of lz4_compress.hip call) on the host, under AddressSanitizer and UBSan: legal
// sequence lists — found by a small greedy finder over random and periodic inputs, and built by
// hand at the length codes' and the block end's extremes — are written into a heap buffer of
// exactly the computed size and must decompress (oracle/lz4.c) to the input; the stored /
// compressed decision and the frame arithmetic must be those of so_lz4_frame_write.
// Built and run by tests/test_lz4_compress_host.py.  Exit 0 = all pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lz4_compress_core.hpp"
#include "spec_oracle.h"

using namespace spec::lz4c;

namespace {

int failures = 0;
long checks = 0;
#define REQUIRE(cond)                                                  \
    do {                                                               \
        checks++;                                                      \
        if (!(cond)) {                                                 \
            if (failures++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                              \
    } while (0)

uint64_t rng_state = 88172645463325252ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

struct Seq {
    uint32_t ls, ll, off, ml; // ml == 0: the last sequence
};
struct HeapOut { // no check of its own: an overrun is the sanitizer's to report
    uint8_t *p;
    void put(uint32_t pos, uint32_t v) { p[pos] = (uint8_t)v; }
};
struct HeapIn {
    const uint8_t *p;
    uint32_t get(uint32_t pos) const { return p[pos]; }
};

// the format's rules over a list (what the GPU test walks in the device's output)
void check_rules(const std::vector<Seq> &seqs, uint32_t n) {
    uint32_t pos = 0;
    for (size_t i = 0; i < seqs.size(); i++) {
        const Seq &s = seqs[i];
        REQUIRE(s.ls == pos);
        pos += s.ll;
        if (i + 1 == seqs.size()) {
            REQUIRE(s.ml == 0 && pos == n);
            REQUIRE(seqs.size() == 1 || s.ll >= LAST_LITERALS);
        } else {
            REQUIRE(s.ml >= MIN_MATCH && s.off >= 1 && s.off <= MAX_OFFSET && s.off <= pos);
            REQUIRE(pos + MF_LIMIT <= n && pos + s.ml + LAST_LITERALS <= n);
            REQUIRE(clamp_match(pos, s.ml, n) == s.ml);
            pos += s.ml;
        }
    }
    if (n < MF_LIMIT + 1) REQUIRE(seqs.size() == 1);
}

// emit into exactly the computed size, decode with the oracle -> the compressed size
uint32_t emit_and_check(const std::vector<uint8_t> &data, const std::vector<Seq> &seqs) {
    const uint32_t n = (uint32_t)data.size();
    check_rules(seqs, n);
    uint32_t size = 0;
    for (const Seq &s : seqs) size += seq_size(s.ll, s.ml);
    uint8_t *buf = (uint8_t *)std::malloc(size); // exactly: one byte more written is a report
    HeapOut out{buf};
    HeapIn in{data.data()};
    uint32_t o = 0;
    for (const Seq &s : seqs) {
        const uint32_t q = put_sequence(out, o, in, s.ls, s.ll, s.off, s.ml);
        REQUIRE(q == o + seq_size(s.ll, s.ml));
        // the pieces the kernel calls on their own
        REQUIRE(put_head(out, o, s.ll, s.ml) == o + 1 + lit_ext_bytes(s.ll));
        REQUIRE(put_tail(out, o + 1 + lit_ext_bytes(s.ll) + s.ll, s.off, s.ml) == q);
        o = q;
    }
    REQUIRE(o == size);
    std::vector<uint8_t> back(n + 1, 0xEE);
    const long long d = so_lz4_decompress_block(buf, size, back.data(), n);
    REQUIRE(d == (long long)n);
    REQUIRE(d != (long long)n || n == 0 || std::memcmp(back.data(), data.data(), n) == 0);
    std::free(buf);
    return size;
}

// a greedy finder (last position per 4-byte hash), the end of the block by clamp_match
std::vector<Seq> find(const std::vector<uint8_t> &d) {
    const uint32_t n = (uint32_t)d.size();
    std::vector<Seq> seqs;
    std::vector<int32_t> tab(1 << 12, -1);
    uint32_t anchor = 0, i = 0;
    const uint32_t lim = match_start_limit(n);
    while (i < lim) {
        uint32_t v;
        std::memcpy(&v, &d[i], 4);
        const uint32_t h = (v * 2654435761u) >> 20;
        const int32_t ref = tab[h];
        tab[h] = (int32_t)i;
        uint32_t ml = 0;
        if (ref >= 0 && i - (uint32_t)ref <= MAX_OFFSET) {
            while (i + ml < n && d[(uint32_t)ref + ml] == d[i + ml]) ml++; // unclamped
            ml = clamp_match(i, ml, n);
        }
        if (!ml) {
            i++;
            continue;
        }
        seqs.push_back({anchor, i - anchor, i - (uint32_t)ref, ml});
        i += ml;
        anchor = i;
    }
    seqs.push_back({anchor, n - anchor, 0, 0});
    return seqs;
}

// one frame of one flush segment by the core's arithmetic against so_lz4_frame_write
void check_frame(const std::vector<uint8_t> &data, uint32_t block_max, bool cc, bool close) {
    const uint64_t n = data.size();
    const uint32_t flags = FLAG_OPEN | (cc ? FLAG_CONTENT : 0) | (close ? FLAG_CLOSE : 0);
    std::vector<uint8_t> frame(frame_bound(n, block_max, flags) + 64);
    const uint64_t fe = n;
    const long long fs = so_lz4_frame_write(data.data(), &fe, 1, block_max, cc, 0, close, frame.data(), frame.size());
    REQUIRE(fs >= 7);
    REQUIRE(frame[4] == header_flg(flags) && frame[5] == (uint8_t)(block_code(block_max) << 4));
    uint64_t at = head_bytes(flags);
    std::vector<uint8_t> tmp(block_max + block_max / 255 + 64);
    const uint64_t nb = block_count(n, block_max);
    for (uint64_t k = 0; k < nb; k++) {
        const uint32_t bn = block_len(n, block_max, k);
        const long long c = so_lz4_compress_block(data.data() + k * block_max, bn, tmp.data(), tmp.size());
        REQUIRE(c > 0);
        uint32_t word;
        std::memcpy(&word, &frame[at], 4);
        REQUIRE(word == block_word((uint32_t)c, bn)); // the oracle stores exactly when the core says so
        REQUIRE(block_stored((uint32_t)c, bn) == (bool)(word >> 31));
        at += 4 + (word & ~STORED_BIT);
    }
    REQUIRE(at + trailer_bytes(flags) == (uint64_t)fs);
    REQUIRE((uint64_t)fs <= frame_bound(n, block_max, flags));
    const Workspace w = workspace_layout(n, block_max);
    REQUIRE(w.nblocks == nb && w.offsets_off >= 4 * nb && w.slots_off >= w.offsets_off + 8 * (nb + 1));
    REQUIRE(w.bytes == w.slots_off + nb * w.slot && w.slot >= block_max && !(w.offsets_off & 15) && !(w.slots_off & 15));
}

std::vector<uint8_t> make_input(uint32_t n, int kind) {
    std::vector<uint8_t> d(n);
    const uint32_t period = 1 + rnd() % 300;
    for (uint32_t i = 0; i < n; i++)
        d[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? (uint8_t)(i < period ? rnd() : d[i - period]) : (uint8_t)(rnd() % 3);
    return d;
}

// data built from the sequences: ll fresh literals, then ml bytes copied from `off` back
void build(std::vector<uint8_t> &d, std::vector<Seq> &seqs, uint32_t ll, uint32_t off, uint32_t ml) {
    const uint32_t ls = (uint32_t)d.size();
    for (uint32_t i = 0; i < ll; i++) d.push_back((uint8_t)rnd());
    for (uint32_t i = 0; i < ml; i++) d.push_back(d[d.size() - off]);
    seqs.push_back({ls, ll, off, ml});
}

} // namespace

int main() {
    // found sequences: every length 0..700, random / periodic / three-letter inputs
    uint32_t with_match = 0;
    for (int round = 0; round < 4; round++)
        for (uint32_t n = 0; n <= 700; n++)
            for (int kind = 0; kind < 3; kind++) {
                const std::vector<uint8_t> d = make_input(n, kind);
                const std::vector<Seq> seqs = find(d);
                const uint32_t size = emit_and_check(d, seqs);
                with_match += seqs.size() > 1;
                REQUIRE(n >= 13 || (seqs.size() == 1 && block_stored(size, n)));
                if (round == 0 && n % 50 == 13) check_frame(d, 64u << 10, kind & 1, n & 1);
            }
    REQUIRE(with_match > 2000);
    for (uint32_t n : {65535u, 65536u, 65537u, 2u * 65536u + 13u})
        for (int kind = 0; kind < 3; kind++) {
            const std::vector<uint8_t> d = make_input(n, kind);
            emit_and_check(d, find(d));
            for (int f = 0; f < 4; f++) check_frame(d, 64u << 10, f & 1, f & 2);
        }
    check_frame(make_input(300000, 1), 256u << 10, true, true);
    for (uint32_t n : {0u, 1u, 12u, 13u}) check_frame(make_input(n, 1), 64u << 10, true, true);
    // the length codes' extremes, every literal length with every match length
    const uint32_t lls[] = {0, 1, 14, 15, 16, 269, 270, 271, 524, 525}, mls[] = {4, 5, 18, 19, 20, 273, 274, 275, 528, 529};
    for (uint32_t ll : lls)
        for (uint32_t ml : mls)
            for (uint32_t tail : {5u, 6u, 20u}) {
                std::vector<uint8_t> d;
                std::vector<Seq> s2;
                build(d, s2, 40 + ll, 1 + rnd() % (40 + ll), ml); // 40 bytes more, to copy from
                const uint32_t reach = (uint32_t)d.size() + ll;
                build(d, s2, ll, 1 + rnd() % (reach < MAX_OFFSET ? reach : MAX_OFFSET), ml);
                if (tail + ml < MF_LIMIT) continue; // the last match would start too late
                const uint32_t ls = (uint32_t)d.size();
                for (uint32_t i = 0; i < tail; i++) d.push_back((uint8_t)rnd());
                s2.push_back({ls, tail, 0, 0});
                emit_and_check(d, s2);
                if (tail == 5) { // the match ends exactly at n - 5: one byte more is clamped back
                    const uint32_t p = ls - ml, n = (uint32_t)d.size();
                    REQUIRE(p + ml == n - 5 && clamp_match(p, ml + 1, n) == ml && clamp_match(p, ml + 1000, n) == ml);
                }
            }
    // the block end: 12 bytes take no match, 13 take one at position 0 only
    REQUIRE(match_start_limit(12) == 0 && match_start_limit(13) == 1 && match_start_limit(0) == 0);
    REQUIRE(clamp_match(0, 100, 12) == 0 && clamp_match(0, 100, 13) == 8 && clamp_match(1, 100, 13) == 0);
    REQUIRE(clamp_match(0, 4, 13) == 4 && clamp_match(0, 3, 13) == 0 && clamp_match(87, 9, 100) == 8 && clamp_match(88, 9, 100) == 0);
    REQUIRE(seq_size(12, 0) == 13 && block_stored(13, 12) && block_stored(12, 12) && !block_stored(11, 12));
    REQUIRE(block_word(7, 12) == 7 && block_word(12, 12) == (12 | STORED_BIT));
    REQUIRE(seq_size(14, 4) == 17 && seq_size(15, 4) == 19 && seq_size(269, 18) == 273 && seq_size(270, 19) == 276 &&
            seq_size(0, 274) == 5 && seq_size(0, 273) == 4);
    REQUIRE(frame_bound(0, 65536, FLAG_OPEN | FLAG_CLOSE | FLAG_CONTENT) == 15 && frame_bound(1, 65536, 7) == 20 &&
            frame_bound(12, 65536, 7) == 31 && frame_bound(65537, 65536, 0) == 65537 + 8);
    REQUIRE(block_code(65536) == 4 && block_code(1 << 18) == 5 && block_code(1 << 20) == 6 && block_code(1 << 22) == 7 &&
            block_code(1 << 19) < 0 && flags_ok(7) && !flags_ok(8));
    std::printf("%ld checks, %d failed\n", checks, failures);
    return failures ? 1 : 0;
}

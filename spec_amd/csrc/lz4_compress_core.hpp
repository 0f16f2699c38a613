// lz4_compress_core.hpp — the integer code of the LZ4 frame compressor, shared by the kernels
// (lz4_compress.hip), the entry points (lz4_host.cpp) and a host test program
// (tests/cpp/lz4_compress_host.cpp): the encoded size of a sequence, the bytes of a sequence
// written at a position under a capacity, the end-of-block clamp of a match, the stored /
// compressed decision and the frame layout arithmetic.
//
// A block is a list of sequences [token][literal length ext][literals][offset u16 LE][match
// length ext]; the last one is literals only.  The format's end rules (what pierrec's decodeBlock
// and oracle/lz4.c accept from a compressor): the last 5 bytes are literals, the last match starts
// at least 12 bytes before the block's end, so a block under 13 bytes has no match.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZ4C_HD __host__ __device__ inline
#else
#define LZ4C_HD inline
#endif

namespace spec {
namespace lz4c {

constexpr uint32_t MIN_MATCH = 4, LAST_LITERALS = 5, MF_LIMIT = 12, MAX_OFFSET = 65535;
constexpr uint32_t STORED_BIT = 0x80000000u;
constexpr uint32_t FRAME_MAGIC = 0x184D2204u, HEADER_BYTES = 7;
constexpr uint32_t FLAG_OPEN = 1, FLAG_CLOSE = 2, FLAG_CONTENT = 4;

// ---- sizes ----
// bytes after the token that carry a length whose nibble is 15 (v = length - 15 >= 0)
LZ4C_HD uint32_t ext_bytes(uint32_t v) { return v / 255 + 1; }
LZ4C_HD uint32_t lit_ext_bytes(uint32_t ll) { return ll >= 15 ? ext_bytes(ll - 15) : 0; }
LZ4C_HD uint32_t match_ext_bytes(uint32_t ml) { return ml >= 19 ? ext_bytes(ml - 19) : 0; }
// a sequence of ll literals and a match of ml >= 4 bytes; ml == 0: the block's last sequence
LZ4C_HD uint32_t seq_size(uint32_t ll, uint32_t ml) {
    return 1 + lit_ext_bytes(ll) + ll + (ml ? 2 + match_ext_bytes(ml) : 0);
}

// ---- the end of a block ----
// positions where a match may start: [0, match_start_limit(n))
LZ4C_HD uint32_t match_start_limit(uint32_t n) { return n > MF_LIMIT ? n - MF_LIMIT : 0; }
// a match at p verified for ml bytes, cut so that the last 5 bytes stay literals (0: no match)
LZ4C_HD uint32_t clamp_match(uint32_t p, uint32_t ml, uint32_t n) {
    if (n < MF_LIMIT + 1 || p >= n - MF_LIMIT) return 0;
    const uint32_t room = n - LAST_LITERALS - p;
    if (ml > room) ml = room;
    return ml >= MIN_MATCH ? ml : 0;
}

// ---- stored or compressed: a block is compressed into n - 1 bytes or stored ----
LZ4C_HD bool block_stored(uint32_t csize, uint32_t n) { return csize >= n; }
LZ4C_HD uint32_t block_word(uint32_t csize, uint32_t n) { return block_stored(csize, n) ? (n | STORED_BIT) : csize; }

// ---- writing ----
// Out: put(uint32_t pos, uint32_t byte) drops what lies at or past its capacity.
template <class Out> LZ4C_HD uint32_t put_ext(Out &out, uint32_t o, uint32_t v) {
    const uint32_t full = v / 255; // trip count known before the loop
    for (uint32_t i = 0; i < full; i++) out.put(o + i, 255);
    out.put(o + full, v - 255 * full);
    return o + full + 1;
}
// token and literal length -> where the literals go
template <class Out> LZ4C_HD uint32_t put_head(Out &out, uint32_t o, uint32_t ll, uint32_t ml) {
    const uint32_t mn = ml ? (ml - MIN_MATCH >= 15 ? 15 : ml - MIN_MATCH) : 0;
    out.put(o, ((ll >= 15 ? 15 : ll) << 4) | mn);
    return ll >= 15 ? put_ext(out, o + 1, ll - 15) : o + 1;
}
// In: get(uint32_t pos) -> byte of the block being compressed
template <class Out, class In> LZ4C_HD uint32_t put_literals(Out &out, uint32_t o, const In &in, uint32_t ls, uint32_t ll) {
    for (uint32_t i = 0; i < ll; i++) out.put(o + i, in.get(ls + i));
    return o + ll;
}
// offset and match length (after the literals) -> the next sequence's token
template <class Out> LZ4C_HD uint32_t put_tail(Out &out, uint32_t o, uint32_t off, uint32_t ml) {
    if (!ml) return o;
    out.put(o, off & 0xff);
    out.put(o + 1, (off >> 8) & 0xff);
    return ml >= 19 ? put_ext(out, o + 2, ml - 19) : o + 2;
}
template <class Out, class In>
LZ4C_HD uint32_t put_sequence(Out &out, uint32_t o, const In &in, uint32_t ls, uint32_t ll, uint32_t off, uint32_t ml) {
    o = put_head(out, o, ll, ml);
    o = put_literals(out, o, in, ls, ll);
    return put_tail(out, o, off, ml);
}

// ---- the frame ----
LZ4C_HD int block_code(uint32_t block_max) { // BD's block max code, -1: not a legal size
    return block_max == (64u << 10) ? 4 : block_max == (256u << 10) ? 5 : block_max == (1u << 20) ? 6
           : block_max == (4u << 20) ? 7 : -1;
}
LZ4C_HD bool flags_ok(uint32_t flags) { return (flags & ~(FLAG_OPEN | FLAG_CLOSE | FLAG_CONTENT)) == 0; }
LZ4C_HD uint64_t block_count(uint64_t len, uint32_t block_max) { return (len + block_max - 1) / block_max; }
LZ4C_HD uint32_t block_len(uint64_t len, uint32_t block_max, uint64_t k) { // block k of block_count
    const uint64_t lo = k * block_max;
    return (uint32_t)(len - lo < block_max ? len - lo : block_max);
}
LZ4C_HD uint32_t head_bytes(uint32_t flags) { return (flags & FLAG_OPEN) ? HEADER_BYTES : 0; }
LZ4C_HD uint32_t trailer_bytes(uint32_t flags) {
    return (flags & FLAG_CLOSE) ? ((flags & FLAG_CONTENT) ? 8 : 4) : 0;
}
// the size with every block stored: what out must hold
LZ4C_HD uint64_t frame_bound(uint64_t len, uint32_t block_max, uint32_t flags) {
    return head_bytes(flags) + len + 4 * block_count(len, block_max) + trailer_bytes(flags);
}
LZ4C_HD uint8_t header_flg(uint32_t flags) { return (uint8_t)(0x60 | ((flags & FLAG_CONTENT) ? 4 : 0)); }

// ---- the workspace: [words u32 x nblocks | offsets u64 x (nblocks + 1) | slots], 16-aligned ----
struct Workspace {
    uint64_t nblocks, slot; // slot: bytes a block compresses into (its buffer resource's size)
    uint64_t words_off, offsets_off, slots_off, bytes;
};
LZ4C_HD Workspace workspace_layout(uint64_t len, uint32_t block_max) {
    Workspace w;
    w.nblocks = block_count(len, block_max);
    w.slot = block_max;
    w.words_off = 0;
    w.offsets_off = (4 * w.nblocks + 15) & ~(uint64_t)15;
    w.slots_off = w.offsets_off + ((8 * (w.nblocks + 1) + 15) & ~(uint64_t)15);
    w.bytes = w.slots_off + w.nblocks * w.slot;
    return w;
}

} // namespace lz4c
} // namespace spec

// lz4_compress.hip — spec_lz4_compress_frame: one Write + Flush of mpx's LZ4 writer on the device
// (mpx/conn_writer.go:42-56: one LZ4 frame of independent blocks per connection).
//
// Three launches:
//   * FIND + EMIT, one wave per block.  The wave walks its block in steps of 64 positions: every
//     lane hashes the 4 bytes at its position, takes the candidate the LDS position table holds
//     for that hash (the last position an earlier step saw it at; used when at most 65535
//     bytes back) and puts its own position in with an LDS max, so the table's content does
//     not depend on the order lanes are served in; a candidate is verified against the input and extended, by its lane up to 32
//     bytes, beyond that wave-wide (256 bytes per round).  A ballot picks the step's
//     non-overlapping matches from the left.  The output position is a running sum the wave
//     carries (a sequence's encoded size is a function of its two lengths), so every picked
//     sequence is written at once by its own lane into the block's workspace slot; literal runs
//     over 16 bytes are copied wave-wide.  A candidate comes from an earlier step only: a period
//     under 64 is found from the block's second step on.
//   * SCAN: an exclusive scan over the blocks' size words (one workgroup, 1024 blocks a chunk)
//     gives every block its place in the frame.
//   * PACK: a workgroup per block copies size word and payload (from the slot, or for a stored
//     block straight from the data) to its place, bytewise up to the output's first 16-byte
//     boundary, then in 16-byte stores; one more workgroup writes the header, the end mark, the
//     content checksum and *total.
//
// Construction (a wrong index gives wrong bytes, never an access outside the buffers):
//   1. input bytes are loaded only through a buffer resource over exactly the block being
//      compressed (wave-uniform 64-bit base, 32-bit offsets; a dword is loaded whole only where
//      all of it lies inside, else bytewise);
//   2. output bytes are stored only through buffer stores on a resource over exactly the region
//      the wave may write: its block's slot, or its block's record inside out[0, bound); plain
//      stores only for the block's size word (one lane, index < nblocks), the scan's offsets
//      and *total;
//   3. the LDS table has a power-of-two size and every index is a masked hash;
//   4. every loop's trip count is computed from the block length (or a constant) before the
//      loop; a block belongs to one wave, workgroups synchronise with barriers only;
//   5. slot and block addresses are 64-bit products;
//   6. the workspace layout is lz4c::workspace_layout, for the size query and the launch alike.
#include <hip/hip_runtime.h>

#include "lz4_compress_core.hpp"
#include "spec_internal.hpp"

namespace spec {

namespace {

using namespace lz4c;

constexpr uint32_t TAB_BITS = 13, TAB = 1u << TAB_BITS; // the position table (u32 entries: 32 KiB)
constexpr uint32_t LANE_ROUNDS = 7;                      // a lane extends its match by this many dwords
constexpr uint32_t LANE_LIT = 16;                        // literal runs a lane copies itself
constexpr uint32_t STEP_SEQS = 64 / MIN_MATCH;           // sequences a step can start
constexpr uint32_t SCAN_CHUNK = 1024;                    // blocks per pass of the scan

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t lane_val(uint32_t v, uint32_t k) { return uni(__builtin_amdgcn_readlane(v, k)); }

struct BufIn { // the block being compressed: [0, n)
    __amdgpu_buffer_rsrc_t r;
    uint32_t n;
    __device__ __forceinline__ uint32_t get(uint32_t p) const { return __builtin_amdgcn_raw_buffer_load_b8(r, p, 0, 0); }
    // 4 bytes at p, zeros past the end
    __device__ __forceinline__ uint32_t get32(uint32_t p) const {
        if (p < n && n - p >= 4) return __builtin_amdgcn_raw_buffer_load_b32(r, p, 0, 0);
        uint32_t w = 0;
        for (uint32_t b = 0; b < 4; b++)
            if (p < n && b < n - p) w |= (uint32_t)get(p + b) << (8 * b);
        return w;
    }
};
struct BufOut { // the region this wave may write; the hardware drops what lies past it
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ void put(uint32_t p, uint32_t v) const {
        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, r, p, 0, 0);
    }
};

__device__ __forceinline__ void wave_copy(const BufOut &out, uint32_t o, const BufIn &in, uint32_t ls, uint32_t ll,
                                          uint32_t lane) {
    const uint32_t rounds = (ll + 63) / 64;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t i = 64 * r + lane;
        if (i < ll) out.put(o + i, in.get(ls + i));
    }
}

struct CompressArgs {
    const uint8_t *data;
    uint64_t len;
    uint32_t block_max;
    uint8_t *slots;
    uint64_t slot;
    uint32_t *words;
};

__global__ __launch_bounds__(64) void lz4c_block_kernel(CompressArgs a) {
    __shared__ uint32_t tab[TAB]; // position + 1 of the last place a hash was seen, 0: nowhere
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t n = block_len(a.len, a.block_max, b);
    const BufIn in{uniform_rsrc(a.data + b * (uint64_t)a.block_max, n), n};
    const BufOut out{uniform_rsrc(a.slots + b * a.slot, a.slot)};
    for (uint32_t i = lane; i < TAB; i += 64) tab[i] = 0;
    __syncthreads();
    const uint32_t mfl = match_start_limit(n);
    const uint32_t nsteps = (mfl + 63) / 64; // no match starts at or past mfl
    uint32_t anchor = 0, o = 0;              // the pending literals' start, the output position
    uint32_t next = in.get32(lane);
    for (uint32_t s = 0; s < nsteps; s++) {
        const uint32_t base = 64 * s, p = base + lane, cur = next;
        next = in.get32(p + 64);
        if (base + 64 <= anchor) continue; // the whole step lies inside a match
        const uint32_t h = (cur * 2654435761u) >> (32 - TAB_BITS);
        // the candidate is what the table held before this step; the step leaves its highest
        // position per hash (an LDS max: the same whichever order the lanes are served in)
        const uint32_t t = __hip_atomic_load(&tab[h & (TAB - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&tab[h & (TAB - 1)], p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t d = p + 1 - t; // t <= p: an earlier step's position
        const uint32_t c = p - d;
        bool has = t != 0 && d <= MAX_OFFSET && d <= p && p < mfl && p >= anchor;
        if (has) has = in.get32(c) == cur;
        uint64_t mask = __ballot(has);
        if (!mask) continue;
        // every lane extends its own match by up to LANE_ROUNDS dwords (to 4 + 4 * LANE_ROUNDS = 32 bytes)
        uint32_t ml = 0;
        bool open = false;
        if (has) {
            ml = MIN_MATCH;
            open = true;
#pragma unroll
            for (uint32_t i = 0; i < LANE_ROUNDS; i++) {
                if (open) {
                    const uint32_t x = in.get32(p + ml) ^ in.get32(c + ml);
                    if (x) {
                        ml += (uint32_t)__builtin_ctz(x) >> 3;
                        open = false;
                    } else {
                        ml += 4;
                    }
                }
            }
        }
        // the step's matches from the left, each past the one before it
        bool sel = false;
        uint32_t my_ls = 0, my_o = 0;
        for (uint32_t it = 0; it < STEP_SEQS; it++) {
            if (!mask) break;
            const uint32_t k = (uint32_t)__builtin_ctzll(mask);
            const uint32_t pk = base + k, ck = pk - lane_val(d, k);
            uint32_t m = lane_val(ml, k);
            if (lane_val(open ? 1u : 0u, k)) { // not ended within those 32 bytes: wave-wide, 256 bytes a round
                const uint32_t rounds = (n - pk) / 256 + 1;
                for (uint32_t r = 0; r < rounds; r++) {
                    const uint32_t x = in.get32(pk + m + 4 * lane) ^ in.get32(ck + m + 4 * lane);
                    const uint64_t diff = __ballot(x != 0);
                    if (diff) {
                        const uint32_t f = (uint32_t)__builtin_ctzll(diff);
                        m += 4 * f + ((uint32_t)__builtin_ctz(lane_val(x, f)) >> 3);
                        break;
                    }
                    m += 256;
                }
            }
            m = clamp_match(pk, m, n);
            uint32_t past = pk + 1; // (a match the clamp leaves nothing of: cannot happen below mfl)
            if (m) {
                if (lane == k) {
                    sel = true;
                    my_ls = anchor;
                    my_o = o;
                    ml = m;
                }
                o += seq_size(pk - anchor, m);
                anchor = pk + m;
                past = anchor;
            }
            const uint32_t rel = past - base;
            mask = rel >= 64 ? 0 : mask & (~0ull << rel);
        }
        // every picked sequence by its own lane; its literals too when they are few
        const uint32_t ll = p - my_ls;
        const bool longlit = sel && ll > LANE_LIT;
        if (sel) {
            const uint32_t q = put_head(out, my_o, ll, ml);
            if (!longlit) put_literals(out, q, in, my_ls, ll);
            put_tail(out, q + ll, d, ml);
        }
        uint64_t lm = __ballot(longlit);
        for (uint32_t it = 0; it < STEP_SEQS; it++) {
            if (!lm) break;
            const uint32_t k = (uint32_t)__builtin_ctzll(lm);
            lm &= lm - 1;
            const uint32_t ls = lane_val(my_ls, k), l = base + k - ls;
            wave_copy(out, lane_val(my_o, k) + 1 + lit_ext_bytes(l), in, ls, l, lane);
        }
    }
    // the last sequence: what is left, as literals (not written when the block will be stored)
    const uint32_t ll = n - anchor;
    const uint32_t csize = o + seq_size(ll, 0);
    if (!block_stored(csize, n)) {
        if (lane == 0) put_head(out, o, ll, 0);
        wave_copy(out, o + 1 + lit_ext_bytes(ll), in, anchor, ll, lane);
    }
    if (lane == 0) a.words[b] = block_word(csize, n);
}

// offsets[k] = where block k's size word goes in the frame; offsets[nblocks] = the blocks' end
__global__ __launch_bounds__(SCAN_CHUNK) void lz4c_scan_kernel(const uint32_t *words, uint64_t nblocks, uint64_t first,
                                                                uint64_t *offsets) {
    __shared__ uint64_t wsum[SCAN_CHUNK / 64];
    __shared__ uint64_t carry_s;
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_s = first;
    __syncthreads();
    const uint64_t chunks = (nblocks + SCAN_CHUNK - 1) / SCAN_CHUNK;
    for (uint64_t ch = 0; ch < chunks; ch++) {
        const uint64_t i = ch * SCAN_CHUNK + t;
        const uint64_t v = i < nblocks ? 4 + (uint64_t)(words[i] & ~STORED_BIT) : 0;
        uint64_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d);
            if ((int)lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint64_t before = 0;
        for (uint32_t k = 0; k < SCAN_CHUNK / 64; k++)
            if (k < w) before += wsum[k];
        const uint64_t carry = carry_s;
        if (i < nblocks) offsets[i] = carry + before + x - v;
        __syncthreads();
        if (t == SCAN_CHUNK - 1) carry_s = carry + before + x;
        __syncthreads();
    }
    if (t == 0) offsets[nblocks] = carry_s;
}

struct PackArgs {
    const uint8_t *data;
    uint64_t len;
    uint32_t block_max;
    uint64_t nblocks;
    const uint8_t *slots;
    uint64_t slot;
    const uint32_t *words;
    const uint64_t *offsets;
    uint8_t *out;
    uint64_t bound;
    uint32_t flags, header_lo, header_hi; // the 7 header bytes, little-endian
    const uint32_t *digest;
    uint64_t *total;
};

// a resource over out[at, at + bytes), cut at the bound
__device__ __forceinline__ BufOut out_region(const PackArgs &a, uint64_t at, uint64_t bytes) {
    const uint64_t room = at < a.bound ? a.bound - at : 0;
    return BufOut{uniform_rsrc(a.out + (room ? at : 0), room < bytes ? room : bytes)};
}

__global__ __launch_bounds__(256) void lz4c_pack_kernel(PackArgs a) {
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    if (b == a.nblocks) { // header, end mark, content checksum, *total
        const uint64_t end = a.nblocks ? a.offsets[a.nblocks] : head_bytes(a.flags);
        const uint32_t hb = head_bytes(a.flags), tb = trailer_bytes(a.flags);
        const BufOut head = out_region(a, 0, hb), tail = out_region(a, end, tb);
        if (t < hb) head.put(t, ((t < 4 ? a.header_lo : a.header_hi) >> (8 * (t & 3))) & 0xff);
        if (t < tb) tail.put(t, t < 4 ? 0u : (*a.digest >> (8 * (t - 4))) & 0xff);
        if (t == 0) *a.total = end + tb;
        return;
    }
    const uint32_t n = block_len(a.len, a.block_max, b);
    const uint32_t word = a.words[b];
    const bool stored = word >> 31;
    uint32_t sz = word & ~STORED_BIT;
    if (sz > n) sz = n; // what the block kernel writes is never larger
    const BufIn src{stored ? uniform_rsrc(a.data + b * (uint64_t)a.block_max, n) : uniform_rsrc(a.slots + b * a.slot, a.slot),
                    stored ? n : (uint32_t)a.slot};
    const uint64_t at = a.offsets[b];
    const uint32_t rec = 4 + sz; // record byte j: the size word, then payload byte j - 4
    const BufOut dst = out_region(a, at, rec);
    auto byte_at = [&](uint32_t j) -> uint32_t { return j < 4 ? (word >> (8 * j)) & 0xff : src.get(j - 4); };
    // up to the output's first 16-byte boundary past the size word
    uint32_t head = (16 - (uint32_t)(((uintptr_t)a.out + at) & 15)) & 15;
    if (head < 4) head += 16;
    if (head > rec) head = rec;
    if (t < head) dst.put(t, byte_at(t));
    const uint32_t granules = (rec - head) / 16;
    const uint32_t rounds = (granules + 255) / 256;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t g = 256 * r + t;
        if (g < granules) {
            const uint32_t j = head + 16 * g;
            u32x4 v;
            v.x = src.get32(j - 4);
            v.y = src.get32(j);
            v.z = src.get32(j + 4);
            v.w = src.get32(j + 8);
            __builtin_amdgcn_raw_buffer_store_b128(v, dst.r, j, 0, 0);
        }
    }
    const uint32_t done = head + 16 * granules;
    if (t < rec - done) dst.put(done + t, byte_at(done + t));
}

} // namespace

int launch_lz4_compress_frame(const uint8_t *data, uint64_t len, uint32_t block_max, uint32_t flags, uint64_t header,
                              const uint32_t *content_digest, uint8_t *out, uint64_t *total, void *workspace,
                              hipStream_t stream) {
    const Workspace w = workspace_layout(len, block_max);
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *words = (uint32_t *)(ws + w.words_off);
    uint64_t *offsets = (uint64_t *)(ws + w.offsets_off);
    if (w.nblocks) {
        CompressArgs c = {data, len, block_max, ws + w.slots_off, w.slot, words};
        hipLaunchKernelGGL(lz4c_block_kernel, dim3((unsigned)w.nblocks), dim3(64), 0, stream, c);
        hipLaunchKernelGGL(lz4c_scan_kernel, dim3(1), dim3(SCAN_CHUNK), 0, stream, (const uint32_t *)words, w.nblocks,
                           (uint64_t)head_bytes(flags), offsets);
    }
    PackArgs p = {data, len, block_max, w.nblocks, ws + w.slots_off, w.slot, words, offsets, out,
                  frame_bound(len, block_max, flags), flags, (uint32_t)header, (uint32_t)(header >> 32),
                  content_digest, total};
    hipLaunchKernelGGL(lz4c_pack_kernel, dim3((unsigned)(w.nblocks + 1)), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace spec

// decode_nested.hip — precompiled (run-time schema) kernels of the list<message> decoder and
// their launchers.  The device code lives in decode_nested_core.hpp; jit.cpp compiles the
// decode kernels specialised to the outer and item schemas.
//
// The items are placed by an index (include/spec_amd.h): nested_count_tail_kernel (per 64-record
// group: item total, from each record's last 64 bytes; nested_count_kernel parses the staged
// span instead) + nested_scan_kernel (exclusive scan of group totals, total items), then
// nested_decode_kernel.  spec_decode_nested_index + spec_decode_nested run the two steps as two
// calls, spec_decode_nested_onepass as one.
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "decode_nested_core.hpp"
#include "spec_internal.hpp"

namespace spec {

namespace {

__global__ __launch_bounds__(256) void nested_count_kernel(NestedArgs a) { nested_count_body(a); }

__global__ __launch_bounds__(256) void nested_count_tail_kernel(NestedArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t wins[256 * TAIL_STRIDE];
    nested_count_tail_body(a, wins);
}

// Exclusive scan of the group totals + total items: one 1024-thread workgroup.  Tiles of
// 16 x 1024 totals: loaded coalesced (all 16 loads in flight) into LDS as u32 (item counts of
// 64 records), each thread then scans 16 CONSECUTIVE totals serially, one block scan of the
// thread sums, results back through LDS, coalesced stores.  (A block scan per 1024 totals
// costs ~1 us of barriers and shuffles on the one CU; this does one per tile.)
__global__ __launch_bounds__(1024) void nested_scan_kernel(NestedArgs a) {
    constexpr int PER = 16, TILE = 1024 * PER;
    __shared__ uint32_t tv[TILE + TILE / 32]; // +1 pad word per 32: thread-contiguous reads spread banks
    __shared__ uint64_t wsum[1024 / 64];
    const uint64_t ngroups = (a.n + 63) / 64;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    auto at = [](int k) { return k + (k >> 5); };
    uint64_t carry = 0;
    for (uint64_t tile = 0; tile < ngroups; tile += TILE) {
        uint64_t v[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const uint64_t k = tile + (uint64_t)i * 1024 + t;
            v[i] = k < ngroups ? a.group_base[k] : 0;
        }
#pragma unroll
        for (int i = 0; i < PER; i++) tv[at(i * 1024 + t)] = (uint32_t)v[i];
        __syncthreads();
        uint32_t mine[PER], sum = 0;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            mine[i] = tv[at(t * PER + i)];
            sum += mine[i];
        }
        uint64_t x = sum; // inclusive wave scan of the thread sums
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint64_t before = 0, tile_total = 0;
#pragma unroll
        for (int k = 0; k < 1024 / 64; k++) {
            before += k < w ? wsum[k] : 0;
            tile_total += wsum[k];
        }
        // exclusive offsets within the tile fit 32 bits (item_begin is uint32)
        uint32_t run = (uint32_t)(before + x - sum);
#pragma unroll
        for (int i = 0; i < PER; i++) {
            tv[at(t * PER + i)] = run;
            run += mine[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const uint64_t k = tile + (uint64_t)i * 1024 + t;
            if (k < ngroups) a.group_base[k] = carry + tv[at(i * 1024 + t)];
        }
        carry += tile_total;
        __syncthreads();
    }
    if (t == 0) *a.total = carry;
}

__global__ __launch_bounds__(256) void nested_decode_kernel(NestedArgs a) {
    nested_decode_body<RuntimeSpec, RuntimeSpec>(a);
}

__global__ __launch_bounds__(256) void nested_decode_ranges_kernel(NestedArgs a) {
    nested_decode_body<RuntimeSpec, RuntimeSpec, true>(a);
}

// spec_set_nested_mode's value: a launcher reads it once, so one call sees one mode
std::atomic<int> g_nested_mode{NESTED_XCD};

// NESTED_HALVES: slabs sized for half a group (32 records), so twice the waves fit a CU's LDS;
// every group is then staged and decoded as two halves (the path a group larger than its
// slab takes anyway).
uint32_t nested_slab_for_mode(int mode, double avg_record) {
    return nested_slab_bytes(mode == NESTED_HALVES ? avg_record * 0.5 : avg_record);
}

// The index kernels under the mode `set`.
int nested_index(NestedArgs a, double avg_record, int set, hipStream_t stream) {
    if (a.n == 0) {
        (void)hipMemsetAsync(a.total, 0, sizeof(uint64_t), stream);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    a.slab = nested_slab_for_mode(set, avg_record);
    const uint64_t groups = (a.n + 63) / 64;
    if (set == NESTED_TAILCOUNT || set == NESTED_XCD) {
        hipLaunchKernelGGL(nested_count_tail_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, stream, a);
    } else {
        dim3 grid((unsigned)((groups + DEC_WAVES - 1) / DEC_WAVES)), block(64 * DEC_WAVES);
        hipLaunchKernelGGL(nested_count_kernel, grid, block, (size_t)DEC_WAVES * a.slab, stream, a);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(nested_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The decode pass after the index kernels: a wave per 64-record group; its items found by an
// owner search (NESTED_GROUPS, default) or from ranges precomputed into LDS (NESTED_RANGES).
int nested_decode(const spec_nested_schema *schema, NestedArgs a, double avg_record, int set, hipStream_t stream) {
    if (a.n == 0) return 0;
    a.slab = nested_slab_for_mode(set, avg_record);
    a.xcd = set == NESTED_XCD ? 1u : 0u;
    const int mode = set >= NESTED_HALVES ? NESTED_GROUPS : set;
    const int j = jit_launch_nested(schema, a, mode, stream);
    if (j != 0) return j > 0 ? 0 : -1;
    const uint64_t groups = (a.n + 63) / 64;
    unsigned blocks = (unsigned)((groups + DEC_WAVES - 1) / DEC_WAVES);
    if (a.xcd) blocks = (blocks + 7) / 8 * 8;
    dim3 grid(blocks), block(64 * DEC_WAVES);
    if (mode == NESTED_RANGES)
        hipLaunchKernelGGL(nested_decode_ranges_kernel, grid, block,
                           (size_t)DEC_WAVES * (a.slab + NESTED_RANGE_BYTES), stream, a);
    else
        hipLaunchKernelGGL(nested_decode_kernel, grid, block, (size_t)DEC_WAVES * a.slab, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace

int launch_nested_index(NestedArgs a, double avg_record, hipStream_t stream) {
    return nested_index(a, avg_record, g_nested_mode.load(std::memory_order_relaxed), stream);
}

int launch_nested_decode(const spec_nested_schema *schema, NestedArgs a, double avg_record, hipStream_t stream) {
    return nested_decode(schema, a, avg_record, g_nested_mode.load(std::memory_order_relaxed), stream);
}

// spec_decode_nested_onepass: the index kernels + the decode kernel back to back (no host round
// trip between them), both under one reading of the mode.
int launch_nested_onepass(const spec_nested_schema *schema, NestedArgs a, double avg_record, hipStream_t stream) {
    const int set = g_nested_mode.load(std::memory_order_relaxed);
    if (nested_index(a, avg_record, set, stream)) return -1;
    return nested_decode(schema, a, avg_record, set, stream);
}

} // namespace spec

extern "C" void spec_set_nested_mode(int mode) {
    if (mode == spec::NESTED_GROUPS || mode == spec::NESTED_RANGES || mode == spec::NESTED_HALVES ||
        mode == spec::NESTED_TAILCOUNT || mode == spec::NESTED_XCD)
        spec::g_nested_mode.store(mode, std::memory_order_relaxed);
}

// tree_internal.hpp — host-side pieces shared by tree.hip (layout, encoder) and tree_decode.hip
// (decoder): the layout of a spec_tree (include/spec_amd.h) with its device descriptor and its
// owner, the row kernels' launch shape, the launcher of a generated kernel, the block scan of both
// files' scan pipelines, a grow-only device buffer.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>

#include "spec_internal.hpp"
#include "tree_core.hpp"

namespace spec {

unsigned row_grid(uint64_t rows); // blocks for a grid-stride pass over `rows` rows
bool is_scalar(int kind);
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The whole host-side description of a tree: the ABI layout + the device descriptor.
struct Layout {
    spec_tree_table tables[TREE_MAX_T];
    spec_tree_column cols[TREE_MAX_C];
    uint32_t nt = 0, nc = 0;
    TreeDesc desc;
};

// jit_tree.cpp jit_tree_kernels(): the kernels of a tree's generated module by these indices, nullptr
// where the module has none and the run-time kernel runs.
enum TreeFn {
    TREE_FN_GROUP = 0,                   // + x: decode of group root x, rows staged in LDS
    TREE_FN_GROUP_HBM = TREE_MAX_T,      // + x: the same, rows from HBM (no staging code)
    TREE_FN_GROUP_PAIR = 2 * TREE_MAX_T, // + x: on 2 waves per 64 rows (root group only, if it splits)
    TREE_FN_SIZE_SET = 3 * TREE_MAX_T,   // the encoder's level-fused size pass
    TREE_FN_WRITE_SET,                   // its level-fused writer, or
    TREE_FN_WRITE_TILE,                  // its record-tile writer (one of the two is generated)
    TREE_FN_GROUP_SET,                   // the level-fused list-group decode
    TREE_FN_COUNT
};

// Builds the layout; false on an invalid tree (rules: include/spec_amd.h spec_tree).
bool build_layout(const spec_tree *tr, Layout &L);

// A built layout on the heap; null for an invalid tree or a failed allocation.
inline std::unique_ptr<Layout> make_layout(const spec_tree *tr) {
    std::unique_ptr<Layout> L(new (std::nothrow) Layout());
    if (L && !build_layout(tr, *L)) L.reset();
    return L;
}

// One kernel of a tree's generated module (jit_tree_kernels) on a gx x gy grid of `block` threads
// with `lds` bytes of dynamic LDS; false on a HIP error, which is noted.
inline bool launch_tree_fn(hipFunction_t fn, unsigned gx, unsigned gy, unsigned block, unsigned lds, hipStream_t st,
                           void **args) {
    const hipError_t e = hipModuleLaunchKernel(fn, gx, gy, 1, block, 1, 1, lds, st, args, nullptr);
    note_hip_error(e);
    return e == hipSuccess;
}

// ---- the scans' shared pieces: tree.hip scans record sizes (scan_tiles / top / apply), tree_decode.hip
// a group's list counts (list_tiles / top / apply); SCAN_PER, elements per thread, is each file's own ----

constexpr int SCAN_T = 1024;          // threads of a scan block
constexpr uint64_t FOLD_TILES = 1024; // up to as many tiles the apply kernel sums the tile totals itself (no top pass)
inline uint64_t scan_tiles(uint64_t n, uint64_t tile) { return (n + tile - 1) / tile; }

// Exclusive block scan through LDS (sh: 17 words; lds_barrier, spec_device.hpp: a caller's loads
// issued before it overlap it).
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *sh, uint64_t &block_total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) sh[wave] = incl;
    lds_barrier();
    if (threadIdx.x == 0) {
        uint64_t acc = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) {
            const uint64_t t = sh[w];
            sh[w] = acc;
            acc += t;
        }
        sh[16] = acc;
    }
    lds_barrier();
    const uint64_t r = sh[wave] + incl - v;
    block_total = sh[16];
    lds_barrier();
    return r;
}

// grow-only device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(bytes, 256);
        if (hipMalloc(&p, want) != hipSuccess) return -1;
        cap = want;
        return 0;
    }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

} // namespace spec

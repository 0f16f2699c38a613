// tree.hip — schema trees on the GPU (include/spec_amd.h spec_tree_*): the layout of a tree and
// the generated writers of internal/lang/generator (message.go:319-439, struct.go:115-142) over
// a batch, for every kind — structs, sub-messages, value lists, lists of structs/messages, any.
// Device code: tree_core.hpp; the decoder (generated readers): tree_decode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "spec_internal.hpp"
#include "tree_internal.hpp"

namespace spec {

unsigned row_grid(uint64_t rows) {
    const uint64_t b = (rows + TB - 1) / TB;
    const uint64_t cap = (uint64_t)device_cus() * 16;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, cap));
}

bool is_scalar(int k) { return k >= SPEC_KIND_BOOL && k <= SPEC_KIND_BYTES; }

namespace {

// ---- encode kernels ------------------------------------------------------------------------

// Encoded size of every row of table x (its children already sized).
__global__ __launch_bounds__(TB) void tree_size_kernel(const TreeDesc *Dp, const TreeBufs *Bp, uint32_t x,
                                                        uint64_t rows) {
    const TreeDesc &D = *Dp;
    const TreeBufs &B = *Bp;
    const TTable &T = D.t[x];
    bool err = false;
    for (uint64_t row = grid_first(); row < rows; row += grid_stride()) {
        uint64_t total;
        if (T.shape == SHAPE_VALUE) {
            const TField &F = D.f[T.field];
            total = value_size(B, D, F.col, F.elem, row, err);
        } else if (T.shape == SHAPE_STRUCT) {
            total = struct_size(B, D, T.field, row, err);
        } else {
            uint64_t data = 0;
            uint32_t nf = 0, maxtag = 0;
            for (uint32_t k = 0; k < T.nd; k++) {
                const TField &F = D.f[D.direct[T.d0 + k]];
                uint64_t sz;
                if (F.kind == K_MESSAGE || F.kind == K_LIST) {
                    if (!cell(B, D, F.present, row)[0]) continue;
                    sz = F.kind == K_MESSAGE ? B.size[F.table][row] : list_size(B, D, F.table, row, err).total;
                } else if (F.opt && !has_bit(B, D, T, row, k)) {
                    continue; // an absent optional field: its columns are not read
                } else if (F.kind == K_STRUCT) {
                    sz = struct_size(B, D, D.direct[T.d0 + k], row, err);
                } else {
                    sz = value_size(B, D, F.col, F.kind, row, err);
                    if (F.kind == K_ANY && sz == 0) continue;
                }
                data += sz;
                nf++;
                maxtag = F.tag > maxtag ? F.tag : maxtag;
            }
            // IsBigMessage (internal/format/msg.go:43-61): a tag > 255 or an end offset > 65535
            const bool big = maxtag > 255 || (nf > 0 && data > 65535);
            const uint64_t tsize = (uint64_t)nf * (big ? 6 : 3);
            if (data > MAX_SIZE) err = true;
            total = data + tsize + vlen64(data) + vlen64(tsize) + 1;
        }
        if (total > 0xffffffffull) err = true;
        B.size[x][row] = (uint32_t)total;
    }
    if (err) *B.err = 1;
}

// Bytes of every row of table x at its start; the starts of its child rows.
__global__ __launch_bounds__(TB) void tree_write_kernel(const TreeDesc *Dp, const TreeBufs *Bp, uint32_t x,
                                                         uint64_t rows) {
    const TreeDesc &D = *Dp;
    const TreeBufs &B = *Bp;
    const TTable &T = D.t[x];
    if (!B.out || *B.err || *B.total > B.out_cap) return;
    extern __shared__ uint32_t tw_ends[]; // MESSAGE tables: [wave][field][lane]
    uint32_t *ends = tw_ends + (threadIdx.x >> 6) * (uint32_t)T.nd * 64 + (threadIdx.x & 63);
    for (uint64_t row = grid_first(); row < rows; row += grid_stride()) {
        const uint64_t start = x == 0 ? B.offsets[row] : B.pos[x][row];
        if (start == ~0ull) continue; // a row no written owner placed (absent message / list)
        if (x == 0 && B.ends_out) B.ends_out[row] = start + B.size[0][row];
        // a framed record's head (mpx/conn_writer.go:84-97) is the first append of its own emitter,
        // which then owns [start - 4, end): nothing below the head is touched
        const uint32_t fh = x == 0 ? B.frame_head : 0u;
        BEmit em{{B.out}, start - fh, start - fh};
        if (fh) em.be(B.size[0][row], 4);
        if (T.shape == SHAPE_VALUE) {
            const TField &F = D.f[T.field];
            emit_value(em, B, D, F.col, F.elem, row);
            em.finish();
            continue;
        }
        if (T.shape == SHAPE_STRUCT) {
            emit_struct(em, B, D, T.field, row);
            em.finish();
            continue;
        }
        // a message (internal/writer/writer.go:376-553): fields in write order, each field's
        // end offset (relative to the message start) kept for the table, in LDS
        // ([field][lane] per wave: a per-lane array indexed at run time would live in scratch)
        uint32_t maxtag = 0, nf = 0;
        for (uint32_t k = 0; k < T.nd; k++) {
            const uint32_t fi = D.direct[T.d0 + k];
            const TField &F = D.f[fi];
            ends[k * 64] = 0xffffffffu; // absent
            if (F.kind == K_MESSAGE || F.kind == K_LIST) {
                if (!cell(B, D, F.present, row)[0]) continue;
                if (F.kind == K_MESSAGE) {
                    B.pos[F.table][row] = em.pos; // the sub-message, written by table F.table
                    em.skip(B.size[F.table][row]);
                } else {
                    // elements (written by table F.table), then EncodeListTable's table and trailer
                    bool e2 = false;
                    uint32_t j0, j1;
                    list_span(B, D, F.table, row, j0, j1, e2);
                    const TreeListSize L = list_size(B, D, F.table, row, e2);
                    const uint64_t lstart = em.pos;
                    for (uint32_t j = j0; j < j1; j++) {
                        B.pos[F.table][j] = em.pos;
                        em.skip(B.size[F.table][j]);
                    }
                    uint64_t off = 0;
                    for (uint32_t j = j0; j < j1; j++) {
                        off += B.size[F.table][j];
                        em.be(off, L.big ? 4 : 2);
                    }
                    (void)lstart;
                    em.rvarint(L.data);
                    em.rvarint((uint64_t)L.count * (L.big ? 4 : 2));
                    em.put1(L.big ? T_BIG_LIST : T_LIST);
                }
            } else if (F.opt && !has_bit(B, D, T, row, k)) {
                continue;
            } else if (F.kind == K_STRUCT) {
                emit_struct(em, B, D, fi, row);
            } else {
                if (F.kind == K_ANY && ((const uint2 *)cell(B, D, F.col, row))->y == 0) continue;
                emit_value(em, B, D, F.col, F.kind, row);
            }
            ends[k * 64] = (uint32_t)(em.pos - start);
            nf++;
            maxtag = F.tag > maxtag ? F.tag : maxtag;
        }
        const uint64_t data = em.pos - start;
        const bool big = maxtag > 255 || (nf > 0 && data > 65535);
        // the table in the writer's order (insertion sort, equal tags: later first,
        // internal/writer/stack_msg.go:37-61), present fields only (encode/msg.go:58-72)
        for (uint32_t k = 0; k < T.nd; k++) {
            const uint32_t fi = D.sorted[T.d0 + k];
            const uint32_t e = ends[D.sslot[T.d0 + k] * 64];
            if (e == 0xffffffffu) continue;
            em.be(D.f[fi].tag, big ? 2 : 1);
            em.be(e, big ? 4 : 2);
        }
        em.rvarint(data);
        em.rvarint((uint64_t)nf * (big ? 6 : 3));
        em.put1(big ? T_BIG_MESSAGE : T_MESSAGE);
        em.finish();
    }
}

// ---- exclusive scans ---------------------------------------------------------------------

constexpr int SCAN_PER = 4, SCAN_TILE = SCAN_T * SCAN_PER; // (SCAN_T, block_excl_scan: tree_internal.hpp)

// pass 1: tile sums of a u32 array; every element counts `add` more (the framed encoder's head
// per record, 0 otherwise)
__global__ __launch_bounds__(SCAN_T) void scan_tiles_kernel(const uint32_t *in, uint64_t n, uint64_t *tile_sums,
                                                            uint32_t add) {
    __shared__ uint64_t sh[17];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_PER;
    uint64_t v = 0;
    for (int k = 0; k < SCAN_PER; k++)
        if (base + k < n) v += (uint64_t)in[base + k] + add;
    uint64_t tot;
    block_excl_scan(v, sh, tot);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

// pass 2: exclusive scan of the tile sums (one workgroup), total
__global__ __launch_bounds__(SCAN_T) void scan_top_kernel(uint64_t *tile_sums, uint64_t ntiles, uint64_t *total,
                                                          const uint32_t *err) {
    __shared__ uint64_t sh[17];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < ntiles; b += SCAN_T) {
        const uint64_t i = b + threadIdx.x;
        const uint64_t v = i < ntiles ? tile_sums[i] : 0;
        uint64_t tot;
        const uint64_t e = block_excl_scan(v, sh, tot);
        if (i < ntiles) tile_sums[i] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = err && *err ? ~0ull : carry; // an encoder error: all-ones
}

// pass 3: per tile, the exclusive prefix of every element: into out32 (u32, + out32[n] = total)
// or out64 (u64); ends64 (optional) = prefix + element.  add: every element is `add` bytes
// longer than in[] says, the extra bytes in FRONT of it — the prefixes written are the elements'
// own starts, past their heads (the framed tree encoder: message starts).  fold (up to FOLD_TILES tiles, no pass 2):
// the tile's offset is the sum of the earlier tiles' totals, summed by the block itself (one load
// per thread), and block 0 sums every tile into *total (all-ones when *err).
__global__ __launch_bounds__(SCAN_T) void scan_apply_kernel(const uint32_t *in, uint64_t n, const uint64_t *tile_sums,
                                                            uint64_t *total, uint32_t *out32, uint64_t *out64,
                                                            uint64_t *ends64, uint32_t fold, const uint32_t *err,
                                                            uint32_t add) {
    __shared__ uint64_t sh[17];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_PER;
    uint32_t v[SCAN_PER];
    uint64_t sum = 0;
    for (int k = 0; k < SCAN_PER; k++) {
        v[k] = base + k < n ? in[base + k] : 0;
        sum += base + k < n ? (uint64_t)v[k] + add : 0;
    }
    uint64_t tot, off = 0, grand = 0;
    if (fold) {
        const uint64_t ntiles = gridDim.x, lim = blockIdx.x ? (uint64_t)blockIdx.x : ntiles;
        uint64_t part = 0;
        for (uint64_t i = threadIdx.x; i < lim; i += SCAN_T) part += tile_sums[i];
        (void)block_excl_scan(part, sh, grand); // earlier tiles (block 0: every tile)
        off = blockIdx.x ? grand : 0;
        if (blockIdx.x == 0) grand = err && *err ? ~0ull : grand; // an encoder error: all-ones
        if (blockIdx.x == 0 && threadIdx.x == 0) *total = grand;
    } else {
        off = tile_sums[blockIdx.x];
    }
    uint64_t p = off + block_excl_scan(sum, sh, tot);
    for (int k = 0; k < SCAN_PER; k++) {
        p += add;
        if (base + k < n) {
            if (out32) out32[base + k] = (uint32_t)p;
            if (out64) out64[base + k] = p;
            if (ends64) ends64[base + k] = p + v[k];
        }
        p += v[k];
    }
    if (out32 && blockIdx.x == 0 && threadIdx.x == 0) out32[n] = (uint32_t)(fold ? grand : *total);
}

// Every child table's row positions to ~0 (unplaced) in one launch: table blockIdx.y
struct PosFill {
    uint64_t *p[TREE_MAX_T];
    uint64_t n[TREE_MAX_T];
};
__global__ __launch_bounds__(256) void tree_pos_fill_kernel(PosFill f) {
    uint64_t *p = f.p[blockIdx.y];
    const uint64_t n = f.n[blockIdx.y];
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) p[i] = ~0ull;
}

size_t scan_ws_bytes(uint64_t n) { return (scan_tiles(n, SCAN_TILE) + 1) * sizeof(uint64_t); }

// exclusive scan of in[0, n) (in place allowed for out32); *total (device) = the sum, or all-ones
// when *err (optional) is set.  add: `add` bytes in front of every element (scan_apply_kernel)
int launch_scan(const uint32_t *in, uint64_t n, uint32_t *out32, uint64_t *out64, uint64_t *ends64, uint64_t *ws,
                uint64_t *total, const uint32_t *err, hipStream_t st, uint32_t add = 0) {
    const uint64_t tiles = std::max<uint64_t>(1, scan_tiles(n, SCAN_TILE));
    const uint32_t fold = tiles <= FOLD_TILES ? 1u : 0u;
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)tiles), dim3(SCAN_T), 0, st, in, n, ws, add);
    if (!fold) hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_T), 0, st, ws, tiles, total, err);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)tiles), dim3(SCAN_T), 0, st, in, n, ws, total, out32, out64,
                       ends64, fold, err, add);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace

// ---- layout (spec_tree_layout) ---------------------------------------------------------------------------------

int add_col(Layout &L, int table, int field, int role, int kind, int width) {
    if (L.nc >= (uint32_t)TREE_MAX_C) return -1;
    spec_tree_column c;
    c.table = (uint16_t)table;
    c.field = (int16_t)field;
    c.role = (uint8_t)role;
    c.kind = (uint8_t)kind;
    c.width = (uint16_t)width;
    L.desc.width[L.nc] = (uint16_t)width;
    L.cols[L.nc] = c;
    return (int)L.nc++;
}

// Builds the layout; false on an invalid tree (rules: include/spec_amd.h spec_tree).
bool build_layout(const spec_tree *tr, Layout &L) {
    if (!tr || tr->nfields > (uint32_t)TREE_MAX_F) return false;
    const uint32_t nf = tr->nfields;
    const spec_tree_field *f = tr->fields;
    TreeDesc &D = L.desc;
    memset(&D, 0, sizeof(D));
    D.nfields = nf;
    for (uint32_t i = 0; i < nf; i++) {
        const int k = f[i].kind, p = f[i].parent;
        if (p < -1 || p >= (int)i) return false;
        if (!is_scalar(k) && k != SPEC_KIND_LIST && k != SPEC_KIND_STRUCT && k != SPEC_KIND_MESSAGE && k != SPEC_KIND_ANY)
            return false;
        if (k == SPEC_KIND_LIST && !is_scalar(f[i].elem) && f[i].elem != SPEC_KIND_STRUCT && f[i].elem != SPEC_KIND_MESSAGE)
            return false;
        // SPEC_TREE_FIELD_OPTIONAL: a scalar or struct that is a direct field of a message (the
        // record, a sub-message, a message-list item); no other bit of `reserved`
        if (f[i].reserved & ~SPEC_TREE_FIELD_OPTIONAL) return false;
        const bool opt = (f[i].reserved & SPEC_TREE_FIELD_OPTIONAL) != 0;
        if (opt && !is_scalar(k) && k != SPEC_KIND_STRUCT) return false;
        if (opt && p >= 0 && f[p].kind != SPEC_KIND_MESSAGE && !(f[p].kind == SPEC_KIND_LIST && f[p].elem == SPEC_KIND_MESSAGE))
            return false;
        if (p >= 0) {
            const int pk = f[p].kind;
            if (pk != SPEC_KIND_STRUCT && pk != SPEC_KIND_MESSAGE && pk != SPEC_KIND_LIST) return false;
            // struct members: value types or other structs (internal/lang/model/struct_field.go:57-70)
            if (pk == SPEC_KIND_STRUCT && !is_scalar(k) && k != SPEC_KIND_STRUCT) return false;
            if (pk == SPEC_KIND_LIST && is_scalar(f[p].elem)) return false;
            if (pk == SPEC_KIND_LIST && f[p].elem == SPEC_KIND_STRUCT && !is_scalar(k) && k != SPEC_KIND_STRUCT)
                return false;
        }
        TField &F = D.f[i];
        F.tag = f[i].tag;
        F.kind = (uint8_t)k;
        F.elem = f[i].elem;
        F.parent = (int16_t)p;
        F.table = F.col = F.present = -1;
        F.send = (uint16_t)(i + 1);
        F.opt = opt ? 1 : 0;
    }
    // subtree ends (pre-order: a field's descendants follow it) and struct nesting depth
    for (uint32_t i = 0; i < nf; i++) {
        int depth = 0;
        for (int p = f[i].parent; p >= 0; p = f[p].parent) {
            D.f[p].send = (uint16_t)std::max<uint32_t>(D.f[p].send, i + 1);
            if (f[p].kind == SPEC_KIND_STRUCT || (f[p].kind == SPEC_KIND_LIST && f[p].elem == SPEC_KIND_STRUCT)) depth++;
        }
        if (f[i].kind == SPEC_KIND_STRUCT) {
            depth++;
            if (f[i].parent >= 0 && (f[f[i].parent].kind == SPEC_KIND_STRUCT ||
                                     (f[f[i].parent].kind == SPEC_KIND_LIST && f[f[i].parent].elem == SPEC_KIND_STRUCT)))
                D.f[f[i].parent].nested = 1;
        }
        if (depth > TREE_MAX_SD) return false;
    }
    // a field's subtree must be contiguous (pre-order): every field inside [i + 1, send) descends from i
    for (uint32_t i = 0; i < nf; i++)
        for (uint32_t j = i + 1; j < D.f[i].send; j++) {
            int p = f[j].parent;
            while (p > (int)i) p = f[p].parent;
            if (p != (int)i) return false;
        }
    auto owner = [&](int i) {
        int p = f[i].parent;
        while (p >= 0 && f[p].kind == SPEC_KIND_STRUCT) p = f[p].parent;
        return p < 0 ? 0 : (int)D.f[p].table;
    };
    // tables
    L.tables[0] = spec_tree_table{-1, -1, SPEC_REL_ROOT, SPEC_SHAPE_MESSAGE, 0, 0};
    L.nt = 1;
    for (uint32_t i = 0; i < nf; i++) {
        const int k = f[i].kind;
        if (k != SPEC_KIND_MESSAGE && k != SPEC_KIND_LIST) continue;
        if (L.nt >= (uint32_t)TREE_MAX_T) return false;
        spec_tree_table t;
        t.parent = (int16_t)owner((int)i);
        t.field = (int16_t)i;
        t.rel = k == SPEC_KIND_MESSAGE ? SPEC_REL_ONE : SPEC_REL_MANY;
        t.shape = (k == SPEC_KIND_MESSAGE || f[i].elem == SPEC_KIND_MESSAGE) ? SPEC_SHAPE_MESSAGE
                  : f[i].elem == SPEC_KIND_STRUCT                             ? SPEC_SHAPE_STRUCT
                                                                              : SPEC_SHAPE_VALUE;
        t.first_column = t.ncolumns = 0;
        D.f[i].table = (int16_t)L.nt;
        L.tables[L.nt++] = t;
    }
    // members of structs (struct fields and lists of structs)
    uint32_t nm = 0;
    for (uint32_t i = 0; i < nf; i++) {
        const bool has_members = f[i].kind == SPEC_KIND_STRUCT || (f[i].kind == SPEC_KIND_LIST && f[i].elem == SPEC_KIND_STRUCT);
        if (!has_members) continue;
        D.f[i].mem0 = (uint16_t)nm;
        for (uint32_t j = i + 1; j < nf; j++)
            if (f[j].parent == (int)i) D.members[nm++] = (uint16_t)j;
        D.f[i].nmem = (uint16_t)(nm - D.f[i].mem0);
        if (D.f[i].nmem > (uint32_t)TREE_MAX_D) return false;
    }
    // columns, table by table; direct-field lists of message tables
    uint32_t nd_all = 0;
    for (uint32_t x = 0; x < L.nt; x++) {
        spec_tree_table &t = L.tables[x];
        TTable &T = D.t[x];
        const int d = t.field;
        T.parent = t.parent;
        T.field = (int16_t)d;
        T.rel = t.rel;
        T.shape = t.shape;
        T.begin_col = -1;
        t.first_column = (uint16_t)L.nc;
        if (t.rel == SPEC_REL_MANY && (T.begin_col = (int16_t)add_col(L, x, d, SPEC_COL_BEGIN, 0, 4)) < 0) return false;
        if (t.shape == SPEC_SHAPE_VALUE) {
            const int c = add_col(L, x, d, SPEC_COL_VALUE, f[d].elem, spec_kind_width(f[d].elem));
            if (c < 0) return false;
            D.f[d].col = (int16_t)c;
        } else if (t.shape == SPEC_SHAPE_STRUCT) {
            for (uint32_t j = (uint32_t)d + 1; j < D.f[d].send; j++) { // scalar members, pre-order
                if (!is_scalar(f[j].kind)) continue;
                const int c = add_col(L, x, (int)j, SPEC_COL_VALUE, f[j].kind, spec_kind_width(f[j].kind));
                if (c < 0) return false;
                D.f[j].col = (int16_t)c;
            }
        } else {
            T.d0 = (uint16_t)nd_all;
            for (uint32_t i = (uint32_t)(d + 1); i < nf; i++) {
                if (f[i].parent != d) continue;
                D.direct[nd_all++] = (uint16_t)i;
                const int k = f[i].kind;
                int c = 0;
                if (is_scalar(k)) {
                    c = D.f[i].col = (int16_t)add_col(L, x, i, SPEC_COL_VALUE, k, spec_kind_width(k));
                } else if (k == SPEC_KIND_ANY) {
                    c = D.f[i].col = (int16_t)add_col(L, x, i, SPEC_COL_VALUE, k, 8);
                    if (c >= 0) c = D.f[i].present = (int16_t)add_col(L, x, i, SPEC_COL_TYPE, 0, 1);
                } else if (k == SPEC_KIND_MESSAGE || k == SPEC_KIND_LIST) {
                    c = D.f[i].present = (int16_t)add_col(L, x, i, SPEC_COL_PRESENT, 0, 1);
                    T.has_children = 1;
                } else { // a struct: its scalar members (inner structs' in place), pre-order
                    for (uint32_t j = i + 1; j < D.f[i].send && c >= 0; j++) {
                        if (!is_scalar(f[j].kind)) continue;
                        c = D.f[j].col = (int16_t)add_col(L, x, (int)j, SPEC_COL_VALUE, f[j].kind, spec_kind_width(f[j].kind));
                    }
                }
                if (c < 0) return false;
            }
            T.nd = (uint16_t)(nd_all - T.d0);
            if (T.nd > (uint32_t)TREE_MAX_D) return false;
            // the writer's table order (insertion sort by tag; an equal tag written later goes
            // first: internal/writer/stack_msg.go:37-61) and each field's index in it
            uint16_t *srt = D.sorted + T.d0;
            for (uint32_t k = 0; k < T.nd; k++) {
                srt[k] = D.direct[T.d0 + k];
                for (int q = (int)k; q > 0 && D.f[srt[q - 1]].tag >= D.f[srt[q]].tag; q--) std::swap(srt[q - 1], srt[q]);
            }
            for (uint32_t k = 0; k < T.nd; k++) D.f[srt[k]].rank = (uint16_t)k;
            for (uint32_t q = 0; q < T.nd; q++) D.sslot[T.d0 + D.f[D.direct[T.d0 + q]].rank] = (uint16_t)q;
        }
        T.err_col = -1;
        // ERRMASK: a bit per direct field, ceil(nd / 64) words (at least one)
        if (t.shape == SPEC_SHAPE_MESSAGE &&
            (T.err_col = (int16_t)add_col(L, x, d, SPEC_COL_ERRMASK, 0, 8 * std::max<uint32_t>(1, (T.nd + 63) / 64))) < 0)
            return false;
        // HASMASK: ERRMASK's words again, only where a direct field is optional
        T.has_col = -1;
        bool any_opt = false;
        for (uint32_t k = 0; t.shape == SPEC_SHAPE_MESSAGE && k < T.nd; k++) any_opt = any_opt || D.f[D.direct[T.d0 + k]].opt;
        if (any_opt && (T.has_col = (int16_t)add_col(L, x, d, SPEC_COL_HASMASK, 0, 8 * std::max<uint32_t>(1, (T.nd + 63) / 64))) < 0)
            return false;
        if ((T.status_col = (int16_t)add_col(L, x, d, SPEC_COL_STATUS, 0, 1)) < 0) return false;
        t.ncolumns = (uint16_t)(L.nc - t.first_column);
    }
    D.ntables = L.nt;
    D.ncols = L.nc;
    // decode groups (tree_decode.hip): every table hangs 1:1 off its owner's group unless it is a
    // list table, which starts its own; groups listed in pre-order, root first
    uint32_t ng = 0;
    for (uint32_t x = 0; x < L.nt; x++) {
        TTable &T = D.t[x];
        T.groot = (x == 0 || T.rel == REL_MANY) ? (uint16_t)x : D.t[T.parent].groot;
        T.gslot = 0xffff;
        T.gn = 0;
    }
    for (uint32_t x = 0; x < L.nt; x++) {
        TTable &T = D.t[x];
        if (T.groot != x) continue;
        T.g0 = (uint16_t)ng;
        for (uint32_t y = x; y < L.nt; y++) {
            if (D.t[y].groot != x) continue;
            if (y != x) D.t[y].gslot = (uint16_t)(T.gn - 1);
            D.group[ng++] = (uint16_t)y;
            T.gn++;
        }
    }
    return true;
}


} // namespace spec

using namespace spec;

extern "C" {

int spec_tree_layout(const spec_tree *tree, spec_tree_table *tables, uint32_t *ntables, spec_tree_column *columns,
                     uint32_t *ncolumns) {
    const std::unique_ptr<Layout> L = make_layout(tree);
    if (!L) return SPEC_E_INVALID_ARGUMENT;
    if (tables) memcpy(tables, L->tables, sizeof(spec_tree_table) * L->nt);
    if (columns) memcpy(columns, L->cols, sizeof(spec_tree_column) * L->nc);
    if (ntables) *ntables = L->nt;
    if (ncolumns) *ncolumns = L->nc;
    return SPEC_OK;
}

} // extern "C"

// ---- encode ----

namespace {
struct EncWs {
    size_t desc, bufs, size[TREE_MAX_T], pos[TREE_MAX_T], offsets, scan, err, total, tblk, tmask;
};

// [desc | bufs | err] first and contiguous: ONE upload (from a pinned slot) sets all three, the
// error word to zero
constexpr size_t ENC_HEAD_DESC = 0;
constexpr size_t ENC_HEAD_BUFS = (sizeof(TreeDesc) + 255) & ~(size_t)255;
constexpr size_t ENC_HEAD_ERR = ENC_HEAD_BUFS + ((sizeof(TreeBufs) + 255) & ~(size_t)255);
constexpr size_t ENC_HEAD = ENC_HEAD_ERR + 256;

size_t enc_plan(const Layout &L, const uint64_t *rows, EncWs &w) {
    size_t o = 0;
    w.desc = ENC_HEAD_DESC;
    w.bufs = ENC_HEAD_BUFS;
    w.err = ENC_HEAD_ERR;
    o = ENC_HEAD;
    for (uint32_t x = 0; x < L.nt; x++) {
        w.size[x] = o;
        o += align256(std::max<uint64_t>(rows[x], 1) * sizeof(uint32_t));
        w.pos[x] = o;
        o += align256(x ? std::max<uint64_t>(rows[x], 1) * sizeof(uint64_t) : 0);
    }
    w.offsets = o;
    o += align256(std::max<uint64_t>(rows[0], 1) * sizeof(uint64_t));
    w.scan = o;
    o += align256(scan_ws_bytes(rows[0]));
    w.total = o;
    o += 256;
    // the record-tile writer's per-record field-block offsets and presence masks (size pass)
    w.tblk = o;
    o += align256(std::max<uint64_t>(rows[0], 1) * TREE_TILE_W * sizeof(uint32_t));
    w.tmask = o;
    o += align256(std::max<uint64_t>(rows[0], 1) * sizeof(uint64_t));
    return o;
}

// copies the workspace head [desc | bufs | err = 0] (ENC_HEAD bytes) to the device on st through
// the library's pinned upload pool (spec::pinned_upload: no host wait on the device); false on a
// HIP error
bool upload_head(const TreeDesc &desc, const TreeBufs &bufs, void *dhead, hipStream_t st) {
    thread_local std::vector<uint8_t> h;
    h.assign(ENC_HEAD, 0);
    memcpy(h.data() + ENC_HEAD_DESC, &desc, sizeof(TreeDesc));
    memcpy(h.data() + ENC_HEAD_BUFS, &bufs, sizeof(TreeBufs));
    return spec::pinned_upload(dhead, h.data(), ENC_HEAD, st) == hipSuccess;
}

// ---- the phases of one encode call (encode_tree_passes), in the order they are issued ----

struct EncCall {
    const Layout &L;
    const TreeBufs &B;  // the call's buffer block (host copy)
    const TreeDesc *Dd; // the descriptor and the block in the workspace head (device)
    TreeBufs *Bd;
    hipStream_t st;
    const hipFunction_t *sets; // the generated module's level-fused kernels, or null: the run-time row kernels
};

// Fills B's columns, heaps, rows and per-table workspace pointers.  INVALID_ARGUMENT: an input
// column or a span column's heap missing where its table has rows, a sub-message table (REL_ONE)
// whose rows are not its owner's.
int bind_columns(const Layout &L, const EncWs &w, uint8_t *ws, const void *const *columns, const uint8_t *const *heaps,
                 const uint64_t *heap_lens, const uint64_t *rows, TreeBufs &B) {
    for (uint32_t c = 0; c < L.nc; c++) {
        B.cols[c] = (void *)columns[c];
        B.heaps[c] = heaps ? heaps[c] : nullptr;
        B.heap_lens[c] = heap_lens ? heap_lens[c] : 0;
        const spec_tree_column &col = L.cols[c];
        const bool spans = col.role == SPEC_COL_VALUE && (col.kind == SPEC_KIND_STRING || col.kind == SPEC_KIND_BYTES ||
                                                         col.kind == SPEC_KIND_ANY);
        // a BEGIN column has owner rows + 1 entries: needed whenever the owner table has rows
        // (an owner whose lists are all empty still reads begin[row], begin[row + 1])
        const uint64_t col_rows = col.role == SPEC_COL_BEGIN ? rows[L.tables[col.table].parent] : rows[col.table];
        const bool input = col.role == SPEC_COL_VALUE || col.role == SPEC_COL_PRESENT || col.role == SPEC_COL_BEGIN ||
                           col.role == SPEC_COL_HASMASK;
        if (input && !columns[c] && col_rows) return SPEC_E_INVALID_ARGUMENT;
        if (spans && rows[col.table] && !B.heaps[c]) return SPEC_E_INVALID_ARGUMENT;
    }
    for (uint32_t x = 0; x < L.nt; x++) {
        B.rows[x] = rows[x];
        B.size[x] = (uint32_t *)(ws + w.size[x]);
        B.pos[x] = x ? (uint64_t *)(ws + w.pos[x]) : nullptr;
        if (L.tables[x].rel == SPEC_REL_ONE && rows[x] != rows[L.tables[x].parent]) return SPEC_E_INVALID_ARGUMENT;
    }
    return SPEC_OK;
}

// Waves per block of the run-time writer (tree_write_kernel) for table T, 0: T does not fit.  A
// message's field ends live in LDS ([wave][field][lane], 256 B per field per wave, 160 KiB per
// block at most): fewer waves for a wide table, and a table of more than 640 direct fields needs
// the generated writer (jit_tree.cpp).
size_t field_ends_bytes(const TTable &T) { // per wave
    return T.shape == SHAPE_MESSAGE ? (size_t)T.nd * 64 * sizeof(uint32_t) : 0;
}
unsigned write_waves(const TTable &T) {
    const size_t per_wave = field_ends_bytes(T);
    return per_wave ? (unsigned)std::min<size_t>(TB / 64, 163840 / per_wave) : TB / 64;
}

// The tables by level: height (a leaf table 0: children have smaller heights, so they are sized
// first) and depth (the records 0: owners have smaller depths, so they are written first).
struct Levels {
    int height[TREE_MAX_T] = {0}, depth[TREE_MAX_T] = {0};
    explicit Levels(const Layout &L) {
        for (uint32_t x = 1; x < L.nt; x++) depth[x] = depth[L.desc.t[x].parent] + 1;
        for (int x = (int)L.nt - 1; x > 0; x--) {
            const int par = L.desc.t[x].parent;
            height[par] = std::max(height[par], height[x] + 1);
        }
    }
};

// Level-fused launches of fn, a level after the other: the level's tables that have rows,
// blockIdx.y picking the table.
bool launch_sets(const EncCall &e, hipFunction_t fn, const int *level) {
    const int top = *std::max_element(level, level + e.L.nt);
    for (int lv = 0; lv <= top; lv++) {
        TableSet ts;
        ts.n = 0;
        uint64_t most = 0;
        for (uint32_t x = 0; x < e.L.nt; x++)
            if (level[x] == lv && e.B.rows[x]) {
                ts.t[ts.n++] = x;
                most = std::max(most, e.B.rows[x]);
            }
        void *args[] = {(void *)&e.Dd, (void *)&e.Bd, &ts};
        if (ts.n && !launch_tree_fn(fn, row_grid(most), ts.n, TB, 0, e.st, args)) return false;
    }
    return true;
}

// Every row's encoded size: level-fused by height, or the run-time kernel table by table
// bottom-up (children before their owners: table order is pre-order).
bool size_pass(const EncCall &e, const Levels &v) {
    if (e.sets) return launch_sets(e, e.sets[TREE_FN_SIZE_SET], v.height);
    for (int x = (int)e.L.nt - 1; x >= 0; x--)
        if (const uint64_t rows = e.B.rows[x])
            hipLaunchKernelGGL(tree_size_kernel, dim3(row_grid(rows)), dim3(TB), 0, e.st, e.Dd, e.Bd, (uint32_t)x, rows);
    return true;
}

// Record offsets and *total (all-ones on an encoder error); no records: *total = 0.
bool record_scan(const EncCall &e, uint64_t *scan_ws) {
    const TreeBufs &B = e.B;
    if (!B.n) return hipMemsetAsync(B.total, 0, sizeof(uint64_t), e.st) == hipSuccess;
    return launch_scan(B.size[0], B.n, nullptr, B.offsets, nullptr, scan_ws, B.total, B.err, e.st, B.frame_head) == 0;
}

// The bytes: the record-tile writer, or a level-fused writer per depth, or the run-time writer
// table by table top-down.
bool write_pass(const EncCall &e, const Levels &v) {
    const Layout &L = e.L;
    if (e.sets && e.sets[TREE_FN_WRITE_TILE]) {
        if (!e.B.n) return true;
        uint32_t cap = TREE_TILE_IMG;
        void *args[] = {(void *)&e.Dd, (void *)&e.Bd, &cap};
        return launch_tree_fn(e.sets[TREE_FN_WRITE_TILE], (unsigned)((e.B.n + 63) / 64), 1, 64 * TREE_TILE_W,
                              TREE_TILE_IMG + 16, e.st, args);
    }
    if (e.sets) return launch_sets(e, e.sets[TREE_FN_WRITE_SET], v.depth);
    // child rows start unplaced: only rows their owner writes get a position (the generated
    // writers mark the rows under an absent or unplaced owner themselves)
    PosFill pf;
    uint64_t most = 0;
    for (uint32_t x = 1; x < L.nt; x++) {
        pf.p[x - 1] = e.B.pos[x];
        pf.n[x - 1] = e.B.rows[x];
        most = std::max(most, e.B.rows[x]);
    }
    if (most) {
        const unsigned gx = (unsigned)std::min<uint64_t>((most + 255) / 256, 1024);
        hipLaunchKernelGGL(tree_pos_fill_kernel, dim3(gx, L.nt - 1), dim3(256), 0, e.st, pf);
    }
    for (uint32_t x = 0; x < L.nt; x++)
        if (const uint64_t rows = e.B.rows[x]) {
            const TTable &T = L.desc.t[x];
            const unsigned wpb = write_waves(T); // (not 0: encode_tree_passes checked before issuing anything)
            const uint64_t blocks = std::min<uint64_t>((rows + 64 * wpb - 1) / (64 * wpb),
                                                       (uint64_t)row_grid(rows) * (TB / 64) / wpb);
            hipLaunchKernelGGL(tree_write_kernel, dim3((unsigned)std::max<uint64_t>(blocks, 1)), dim3(64 * wpb),
                               wpb * field_ends_bytes(T), e.st, e.Dd, e.Bd, x, rows);
        }
    return true;
}
} // namespace

// spec_encode_tree (frame_head 0) and spec_encode_tree_frames (4: every record behind its mpx
// frame head, written by the record's own root writer; the same launches)
int spec::encode_tree_passes(const spec_tree *tree, const void *const *columns, const uint8_t *const *heaps,
                             const uint64_t *heap_lens, const uint64_t *rows, uint8_t *out, uint64_t out_cap,
                             uint64_t *ends, void *workspace, size_t workspace_size, uint64_t *total, void *stream,
                             uint32_t frame_head) {
    if (!columns || !rows || !total || !workspace) return SPEC_E_INVALID_ARGUMENT;
    const std::unique_ptr<Layout> Lp = make_layout(tree);
    if (!Lp) return SPEC_E_INVALID_ARGUMENT;
    const Layout &L = *Lp;
    EncWs w;
    if (enc_plan(L, rows, w) > workspace_size) return SPEC_E_WORKSPACE;
    uint8_t *ws = (uint8_t *)workspace;
    const std::unique_ptr<TreeBufs> Bp(new (std::nothrow) TreeBufs());
    if (!Bp) return SPEC_E_INVALID_ARGUMENT;
    TreeBufs &B = *Bp;
    memset(&B, 0, sizeof(B));
    if (const int rc = bind_columns(L, w, ws, columns, heaps, heap_lens, rows, B)) return rc;
    B.n = rows[0];
    B.out = out;
    B.out_cap = out ? out_cap : 0;
    B.ends_out = ends;
    B.offsets = (uint64_t *)(ws + w.offsets);
    B.tblk = (uint32_t *)(ws + w.tblk);
    B.tmask = (uint64_t *)(ws + w.tmask);
    B.total = total;
    B.err = (uint32_t *)(ws + w.err);
    B.frame_head = frame_head;
    // the generated size passes and writers (jit_tree.cpp), level-fused (tree_core.hpp TableSet): the
    // tables of one height sized together, of one depth written together
    const hipFunction_t *jit = jit_tree_kernels(L.desc);
    const bool sets = jit && jit[TREE_FN_SIZE_SET] && (jit[TREE_FN_WRITE_SET] || jit[TREE_FN_WRITE_TILE]);
    const EncCall e{L, B, (const TreeDesc *)(ws + w.desc), (TreeBufs *)(ws + w.bufs), (hipStream_t)stream,
                    sets ? jit : nullptr};
    // a table the run-time writer cannot take: refused before anything is issued, so the call leaves
    // the stream, *total and out untouched
    for (uint32_t x = 0; !e.sets && out && x < L.nt; x++)
        if (rows[x] && write_waves(L.desc.t[x]) == 0) return SPEC_E_TOO_LARGE;
    const Levels v(L);
    const bool ok = upload_head(L.desc, B, ws, e.st) && size_pass(e, v) && record_scan(e, (uint64_t *)(ws + w.scan)) &&
                    (!out || write_pass(e, v));
    const hipError_t err = hipGetLastError(); // the run-time kernels' launches
    note_hip_error(err);
    return ok && err == hipSuccess ? SPEC_OK : SPEC_E_HIP;
}

extern "C" {

size_t spec_encode_tree_workspace_size(const spec_tree *tree, const uint64_t *rows) {
    const std::unique_ptr<Layout> L = make_layout(tree);
    if (!L || !rows) return 0;
    EncWs w;
    return enc_plan(*L, rows, w);
}

int spec_encode_tree(const spec_tree *tree, const void *const *columns, const uint8_t *const *heaps,
                     const uint64_t *heap_lens, const uint64_t *rows, uint8_t *out, uint64_t out_cap, uint64_t *ends,
                     void *workspace, size_t workspace_size, uint64_t *total, void *stream) {
    return encode_tree_passes(tree, columns, heaps, heap_lens, rows, out, out_cap, ends, workspace, workspace_size,
                              total, stream, 0);
}

// spec_encode_tree with every record behind its mpx frame head (mpx/conn_writer.go:84-97): the
// bytes of spec_frames_write over spec_encode_tree's stream, from the encoder's own launches
int spec_encode_tree_frames(const spec_tree *tree, const void *const *columns, const uint8_t *const *heaps,
                            const uint64_t *heap_lens, const uint64_t *rows, uint8_t *frames, uint64_t frames_cap,
                            uint64_t *frame_ends, void *workspace, size_t workspace_size, uint64_t *total,
                            void *stream) {
    return encode_tree_passes(tree, columns, heaps, heap_lens, rows, frames, frames_cap, frame_ends, workspace,
                              workspace_size, total, stream, 4);
}

} // extern "C"

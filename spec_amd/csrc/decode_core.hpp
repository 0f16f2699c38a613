// decode_core.hpp — device code of the flat-message decoder (gfx950), shared by the
// precompiled generic kernel (decode_flat.hip) and the schema-specialised kernels that
// jit.cpp compiles at run time with hiprtc.
//
// Replaces, per record, spec.OpenMessageErr (internal/types/msg.go:43-55 ->
// internal/decode/msg.go:14-99) followed by one typed getter per schema field
// (internal/types/msg.go:219-475: m.field(tag) = table.Offset(tag) binary search
// (internal/format/msg.go:227-265) + decode.Decode<Kind>(bytes[:end])).
//
// Mapping (MI355X, wave64):
//   * one group = 64 consecutive records, one record per lane, on one wave (run-time schema) or
//     on P waves that share the fields (generated kernels);
//   * the group's contiguous byte span [ends[base-1], ends[base+63]) is staged into the group's
//     private LDS slab with LDS-DMA (buffer_load_dwordx4 ... lds, 1 KiB per instruction,
//     range-checked by the buffer descriptor) — one fully coalesced HBM read of the stream;
//   * each lane parses its record from LDS.  Two code paths:
//       - the FAST path (schema known at compile time: `Spec` = a generated struct) reads the
//         field table with a few wide LDS reads, checks that it holds exactly the
//         schema's tags in the order a Writer emits them (then the reference's binary search
//         provably lands on the same entries), and decodes every field with straight-line,
//         kind-specialised code the compiler can interleave (ILP across fields);
//       - the GENERIC path (any table, any record) restates the reference step by step:
//         trailer, sortedness check, probe at the expected index or exact binary search,
//         per-kind decode selected at run time.  Records the fast path rejects go here,
//         so results never depend on which path ran;
//   * column writes are lane-strided => coalesced per field;
//   * a wave whose span exceeds its slab parses straight from HBM via range-checked buffer
//     loads (GlobalSrc, generic path) — correctness never depends on record sizes.
#pragma once

#include "spec_device.hpp"

namespace spec {


// The fields a record decode produces: one column per schema field + the status column.
struct FieldSet {
    uint8_t *status;
    uint64_t *errmask; // optional: bit f = field f's <Kind>Err getter errs
    uint64_t *present; // the PRESENT kernels only: bit f = m.HasField(tag f) (internal/types/msg.go:106-111)
    uint32_t nfields;
    uint16_t tags[SPEC_KFIELDS];
    uint8_t kinds[SPEC_KFIELDS];
    uint16_t rank[SPEC_KFIELDS]; // index of the field's tag in the sorted table a writer emits
    void *cols[SPEC_KFIELDS];
};

// Passed by value as the kernel argument (lives in the kernarg segment => scalar loads,
// the per-field loop branches are wave-uniform).
struct DecodeArgs {
    const uint8_t *stream;
    uint64_t stream_len;
    const uint64_t *ends;
    uint64_t n;  // records [r0, n) of the batch are decoded (columns indexed by record)
    uint64_t r0;
    uint32_t head; // bytes before each record (mpx frame head = 4: [u32 BE size][message])
    uint32_t slab; // LDS bytes per wave (0: every wave parses from HBM)
    uint32_t xcd;  // 1: XCD-aware block order (consecutive groups on one XCD's L2)
    FieldSet f;
};

// spec_decode_nested (decode_nested.hip): outer records with one list<message> field.
struct NestedArgs {
    const uint8_t *stream;
    uint64_t stream_len;
    const uint64_t *ends;
    uint64_t n;
    FieldSet outer; // the outer message; its K_LIST field is decoded into item_begin
    FieldSet item;  // the list items
    uint32_t list_tag, list_rank;
    uint32_t *item_begin; // [n + 1]
    uint64_t item_cap;    // item columns hold this many items
    uint64_t *group_base; // workspace: per 64-record group item total, then exclusive offsets
    uint64_t *total;      // device: total items
    uint32_t slab;        // LDS bytes per wave
    uint32_t xcd;         // decode pass: 1 = XCD-aware block order (grid a multiple of 8)
    uint32_t head;        // bytes before each record (DecodeArgs::head; 4: ends are mpx frame ends)
};

constexpr int DEC_WAVES = 4; // waves per block of the nested kernels
constexpr int SLAB_GUARD = 48; // >= the deepest read below a value end (bin256: 33 + 7)

// LDS slab per wave: guard + the 1 KiB DMA chunks a 64-record span needs + pad.  Sized at
// launch from the batch's mean record size with a margin (4 % for flat records; 16 % for
// nested ones, whose item counts vary: on config 4, 4 % left 17.8 % of the groups over the
// slab, 16 % leaves 0.05 %); a wave whose span does not fit is staged in halves or parses
// from HBM, so the margin only affects speed.
constexpr int SLAB_MAX_CHUNKS = 40;
__host__ __device__ inline uint32_t decode_slab_bytes(double avg_record, double margin = 1.04) {
    const double span = avg_record * 64 * margin;
    int chunks = (int)(span / 1024.0) + 1;
    if (chunks > SLAB_MAX_CHUNKS) return 0;
    return (uint32_t)(SLAB_GUARD + chunks * 1024 + 32);
}
// The nested kernels run DEC_WAVES waves per block, each with its slab plus (RANGES mode) a 1 KiB
// item-range window: the block's LDS must stay within gfx950's 160 KiB, so a slab over
// NESTED_SLAB_MAX is not used (0: the groups parse from HBM).
constexpr uint32_t NESTED_SLAB_MAX = 163840 / DEC_WAVES - 1024;
__host__ __device__ inline uint32_t nested_slab_bytes(double avg_record) {
    const uint32_t s = decode_slab_bytes(avg_record, 1.16);
    return s <= NESTED_SLAB_MAX ? s : 0u;
}

// ---- message table lookup --------------------------------------------------------------

// exact reference binary search (offset_small/offset_big), returns end offset or -1
template <class Src>
__device__ __noinline__ long long table_search(const Src s, typename Src::pos_t tstart, uint32_t nent,
                                               bool big, uint32_t tag) {
    int left = 0, right = (int)nent - 1;
    while (left <= right) {
        int mid = (int)((unsigned)(left + right) >> 1);
        uint32_t cur;
        typename Src::pos_t p;
        if (big) {
            p = tstart + (typename Src::pos_t)mid * 6;
            cur = (s.u8(p) << 8) | s.u8(p + 1);
        } else {
            p = tstart + (typename Src::pos_t)mid * 3;
            cur = s.u8(p);
        }
        if (cur < tag) {
            left = mid + 1;
        } else if (cur > tag) {
            right = mid - 1;
        } else {
            if (big)
                return ((long long)s.u8(p + 2) << 24) | (s.u8(p + 3) << 16) | (s.u8(p + 4) << 8) | s.u8(p + 5);
            return (s.u8(p + 1) << 8) | s.u8(p + 2);
        }
    }
    return -1;
}

// ---- value decoders: field slice [lo, e), type at e-1 (internal/decode/...) ------------

struct Val {
    uint64_t v0, v1, v2, v3; // up to 32 bytes of column payload, little-endian
};

// Decode the value ending at e (field slice [lo, e), flen = e - lo; flen <= 0 => zero value)
// from its 16-byte tail window t; bin128/bin256 read their leading bytes from s.
// Straight-line code (selects, no branches): every byte it reads lies within 40 bytes below
// e, which callers keep inside the source even for an empty field.
// The bytes a value's decode reads: its 16-byte tail window, plus for bin128/bin256 the
// leading payload qwords.
struct Win {
    Tail t;
    uint64_t x0, x1, x2;
};

// Kinds whose value, once its type is the one the Writer emits (cross_kind_type), ends in at
// most 8 bytes: type byte + <= 5-byte reverse varint (32-bit ints, string/bytes lengths),
// 4-byte float32, byte, bool.  The fast path reads an 8-byte window for them (2 LDS reads,
// not 3); bytes below the window read as 0, which a <= 5-byte varint never looks at.
template <uint32_t KIND>
__host__ __device__ constexpr bool narrow_kind() {
    return KIND == K_BOOL || KIND == K_BYTE || KIND == K_INT16 || KIND == K_INT32 || KIND == K_UINT16 ||
           KIND == K_UINT32 || KIND == K_FLOAT32 || KIND == K_STRING || KIND == K_BYTES;
}

// Fixed-width payloads (bin64/128/256, float64): NQ payload qwords [e-1-8NQ, e-1) and the
// type byte at e-1, from the NQ+1 aligned qwords that cover them (a 16-byte tail window plus
// separate payload reads would take 3 / 5 / 9 reads for 8 / 16 / 32 bytes; this takes 2 / 3 / 5).
// Packed as a Win: x0.. = leading payload qwords (little-endian), t = the tail view decode_tail_k
// reads (type byte + the last 8 payload bytes, big-endian).
template <int NQ, class Src>
__device__ __forceinline__ Win load_fixed(const Src &s, typename Src::pos_t e) {
    using pos_t = typename Src::pos_t;
    const pos_t p = e - 1 - 8 * NQ;
    const pos_t base = p & ~(pos_t)7;
    const uint32_t sh = 8u * (uint32_t)(p - base);
    uint64_t q[NQ + 1], c[NQ];
#pragma unroll
    for (int j = 0; j <= NQ; j++) q[j] = s.d64(base + 8 * j);
#pragma unroll
    for (int j = 0; j < NQ; j++) c[j] = (q[j] >> sh) | ((q[j + 1] << 1) << (63 - sh));
    const uint32_t type = (uint32_t)(q[NQ] >> sh) & 0xff;
    const uint64_t B = __builtin_bswap64(c[NQ - 1]);
    Win w;
    w.t.q0 = (B << 8) | type;
    w.t.q1 = B >> 56;
    w.x0 = NQ > 1 ? c[0] : 0;
    w.x1 = NQ > 2 ? c[1 % NQ] : 0;
    w.x2 = NQ > 3 ? c[2 % NQ] : 0;
    return w;
}

template <uint32_t KIND, bool NARROW = false, class Src>
__device__ __forceinline__ Win load_win(const Src &s, typename Src::pos_t e) {
    Win w;
    if constexpr (NARROW && narrow_kind<KIND>()) {
        w.t.q0 = __builtin_bswap64(load_le64(s, e - 8)); // BE64([e-8, e))
        w.t.q1 = 0;
        w.x0 = w.x1 = w.x2 = 0;
        return w;
    } else if constexpr (NARROW && (KIND == K_FLOAT64 || KIND == K_BIN64)) {
        return load_fixed<1>(s, e);
    } else if constexpr (NARROW && KIND == K_BIN128) {
        return load_fixed<2>(s, e);
    } else if constexpr (NARROW && KIND == K_BIN256) {
        return load_fixed<4>(s, e);
    }
    w.t = load_tail(s, e);
    w.x0 = w.x1 = w.x2 = 0;
    if constexpr (KIND == K_BIN128) {
        w.x0 = load_le64(s, e - 17);
    } else if constexpr (KIND == K_BIN256) {
        w.x0 = load_le64(s, e - 33);
        w.x1 = load_le64(s, e - 25);
        w.x2 = load_le64(s, e - 17);
    }
    return w;
}

// The type a Writer emits for a column kind, for the kinds whose getter also accepts other
// types (ints of other widths, float32 <-> float64); 0 for kinds that accept one type only.
__host__ __device__ constexpr uint32_t cross_kind_type(uint32_t k) {
    return k == K_INT16 ? T_INT16 : k == K_INT32 ? T_INT32 : k == K_INT64 ? T_INT64
         : k == K_UINT16 ? T_UINT16 : k == K_UINT32 ? T_UINT32 : k == K_UINT64 ? T_UINT64
         : k == K_FLOAT32 ? T_FLOAT32 : k == K_FLOAT64 ? T_FLOAT64 : 0u;
}

// NAT = true: the caller has checked that the value's type byte is cross_kind_type(KIND) (or
// the field is empty), so the cross-width branches fold away; results are those of NAT = false
// for such values.
// okp (optional): set to false when the decoder returns an error (the getter's *Err variant,
// internal/types/msg.go:233-459); a non-empty field only (callers handle flen <= 0).
template <uint32_t KIND, bool NAT = false, class Pos>
__device__ __forceinline__ Val decode_tail_k(const Win &w, Pos lo, Pos e, long long to_stream, bool *okp = nullptr) {
    const Tail &t = w.t;
    Val out = {0, 0, 0, 0};
    bool okv = true;
    const long long flen = (long long)(e - lo);
    constexpr uint32_t NT = cross_kind_type(KIND);
    const uint32_t type = (NAT && NT) ? NT : (uint32_t)t.q0 & 0xff;
    const uint64_t R = tail_r(t);
    const uint32_t R2 = tail_r2(t);
    const long long avail = flen - 1; // bytes before the type byte
    int m;
    if constexpr (KIND == K_BOOL) { // DecodeBool, byte.go:38-51: true iff type == TypeTrue
        out.v0 = ((flen > 0) & (type == T_TRUE)) ? 1 : 0;
    } else if constexpr (KIND == K_BYTE) { // DecodeByte, byte.go:16-34
        okv = (type == T_BYTE) & (flen >= 2);
        out.v0 = okv ? (R & 0xff) : 0;
    } else if constexpr (KIND == K_INT16 | KIND == K_INT32 | KIND == K_INT64) {
        // DecodeInt16/32/64, int.go:16-135: 32-bit routine for Int16/Int32, 64-bit for Int64
        const bool w32 = (type == T_INT16) | (type == T_INT32);
        const uint64_t u = rvarint_bf(R, R2, avail, w32 ? 5 : 10, m);
        const long long x = w32 ? (long long)unzigzag32((uint32_t)u) : (long long)unzigzag64(u);
        bool ok = (flen > 0) & (w32 | (type == T_INT64)) & (m >= 0);
        if (KIND == K_INT16) ok = ok & (x >= -32768) & (x <= 32767);
        if (KIND == K_INT32) ok = ok & (w32 | ((x >= INT32_MIN) & (x <= INT32_MAX)));
        okv = ok;
        out.v0 = ok ? (uint64_t)x : 0;
        if (KIND == K_INT16) out.v0 &= 0xffff;
        if (KIND == K_INT32) out.v0 &= 0xffffffffu;
    } else if constexpr (KIND == K_UINT16 | KIND == K_UINT32 | KIND == K_UINT64) {
        // DecodeUint16/32/64, uint.go:16-125
        const bool w32 = (type == T_UINT16) | (type == T_UINT32);
        const uint64_t x = rvarint_bf(R, R2, avail, w32 ? 5 : 10, m);
        bool ok = (flen > 0) & (w32 | (type == T_UINT64)) & (m >= 0);
        if (KIND == K_UINT16) ok = ok & (x <= 0xffffull);
        if (KIND == K_UINT32) ok = ok & (x <= 0xffffffffull);
        okv = ok;
        out.v0 = ok ? x : 0;
    } else if constexpr (KIND == K_FLOAT32) { // DecodeFloat32, float.go:15-32 (via float64 + range check)
        uint32_t b = (uint32_t)(R & 0xffffffffu);
        const uint32_t ex = (b >> 23) & 0xff;
        const bool inf = (ex == 0xff) & ((b & 0x7fffff) == 0); // +-Inf fails the +-MaxFloat32 check
        b = ex == 0xff ? (b | 0x00400000u) : b;             // NaN: quieted by the float64 round trip
        const uint64_t d = R;
        const uint32_t dx = (uint32_t)(d >> 52) & 0x7ff;
        const bool nan = (dx == 0x7ff) & ((d & 0xfffffffffffffull) != 0);
        // |d| > MaxFloat32 (0x47EFFFFFE0000000) => overflow error => 0
        const bool over = !nan & ((d & 0x7fffffffffffffffull) > 0x47EFFFFFE0000000ull);
        const uint32_t from64 = f64_to_f32_bits_bf(d);
        const bool ok32 = (type == T_FLOAT32) & (flen >= 5) & !inf, ok64 = (type == T_FLOAT64) & (flen >= 9) & !over;
        okv = ok32 | ok64;
        out.v0 = ok32 ? b : (ok64 ? from64 : 0u);
    } else if constexpr (KIND == K_FLOAT64) { // DecodeFloat64, float.go:34-78
        const uint64_t from32 = f32_to_f64_bits_bf((uint32_t)(R & 0xffffffffu));
        const bool ok32 = (type == T_FLOAT32) & (flen >= 5), ok64 = (type == T_FLOAT64) & (flen >= 9);
        okv = ok32 | ok64;
        out.v0 = ok32 ? from32 : (ok64 ? R : 0ull);
    } else if constexpr (KIND == K_BIN64) { // DecodeBin64, bin.go:15-44: raw 8 bytes before the type byte
        okv = (type == T_BIN64) & (flen >= 9);
        out.v0 = okv ? __builtin_bswap64(R) : 0;
    } else if constexpr (KIND == K_BIN128) {
        const bool ok = (type == T_BIN128) & (flen >= 17);
        okv = ok;
        out.v0 = ok ? w.x0 : 0;
        out.v1 = ok ? __builtin_bswap64(R) : 0;
    } else if constexpr (KIND == K_BIN256) {
        const bool ok = (type == T_BIN256) & (flen >= 33);
        okv = ok;
        out.v0 = ok ? w.x0 : 0;
        out.v1 = ok ? w.x1 : 0;
        out.v2 = ok ? w.x2 : 0;
        out.v3 = ok ? __builtin_bswap64(R) : 0;
    } else if constexpr (KIND == K_STRING | KIND == K_BYTES) {
        // DecodeString (string.go:15-70) / DecodeBytes (bytes.go:14-58)
        constexpr bool str = KIND == K_STRING;
        const uint32_t len = (uint32_t)rvarint_bf(R, R2, avail, 5, m);
        const long long end = (long long)(e - 1) - m - (str ? 1 : 0); // skip the NUL for strings
        const long long off = end - (long long)len;
        const bool ok = (type == (str ? T_STRING : T_BYTES)) & (flen > 0) & (m >= 0) & (end >= (long long)lo) &
                        (off >= (long long)lo) & (len != 0);
        okv = (type == (str ? T_STRING : T_BYTES)) & (m >= 0) & (end >= (long long)lo) & (off >= (long long)lo);
        out.v0 = ok ? ((uint64_t)(uint32_t)(off + to_stream) | ((uint64_t)len << 32)) : 0;
    }
    if (okp) *okp = okv;
    return out;
}

// Columns are written once and not read back by the kernel: non-temporal stores.
template <class T>
__device__ __forceinline__ void col_store(T *p, T v) {
    __builtin_nontemporal_store(v, p);
}

template <uint32_t KIND>
__device__ __forceinline__ void store_value_k(void *colp, uint64_t r, const Val &v) {
    uint8_t *col = (uint8_t *)colp;
    if constexpr (KIND == K_BOOL || KIND == K_BYTE) {
        col_store(col + r, (uint8_t)v.v0);
    } else if constexpr (KIND == K_INT16 || KIND == K_UINT16) {
        col_store((uint16_t *)col + r, (uint16_t)v.v0);
    } else if constexpr (KIND == K_INT32 || KIND == K_UINT32 || KIND == K_FLOAT32) {
        col_store((uint32_t *)col + r, (uint32_t)v.v0);
    } else if constexpr (KIND == K_BIN128) {
        col_store((uint64_t *)col + 2 * r, v.v0);
        col_store((uint64_t *)col + 2 * r + 1, v.v1);
    } else if constexpr (KIND == K_BIN256) {
        col_store((uint64_t *)col + 4 * r, v.v0);
        col_store((uint64_t *)col + 4 * r + 1, v.v1);
        col_store((uint64_t *)col + 4 * r + 2, v.v2);
        col_store((uint64_t *)col + 4 * r + 3, v.v3);
    } else {
        col_store((uint64_t *)col + r, v.v0);
    }
}

// run-time kind dispatch for the generic path (wave-uniform switches around ONE shared
// tail-window load, so the generic kernel stays compact)
// returns false when the field is present and its decoder errs (the *Err getter's error)
template <class Src>
__device__ __forceinline__ bool decode_store(const Src &s, uint32_t kind, typename Src::pos_t lo, long long end,
                                             long long to_stream, void *col, uint64_t r) {
    Val v = {0, 0, 0, 0};
    bool ok = true;
    if (end > 0) {
        const typename Src::pos_t e = lo + (typename Src::pos_t)end;
#define SPEC_CASE(K) \
    case K: v = decode_tail_k<K>(load_win<K>(s, e), lo, e, to_stream, &ok); break;
        switch (kind) {
            SPEC_CASE(K_BOOL)
            SPEC_CASE(K_BYTE)
            SPEC_CASE(K_INT16)
            SPEC_CASE(K_INT32)
            SPEC_CASE(K_INT64)
            SPEC_CASE(K_UINT16)
            SPEC_CASE(K_UINT32)
            SPEC_CASE(K_UINT64)
            SPEC_CASE(K_FLOAT32)
            SPEC_CASE(K_FLOAT64)
            SPEC_CASE(K_BIN64)
            SPEC_CASE(K_BIN128)
            SPEC_CASE(K_BIN256)
            SPEC_CASE(K_STRING)
            SPEC_CASE(K_BYTES)
        }
#undef SPEC_CASE
    }
    uint8_t *c = (uint8_t *)col;
    switch (kind) {
    case K_BOOL:
    case K_BYTE: c[r] = (uint8_t)v.v0; break;
    case K_INT16:
    case K_UINT16: ((uint16_t *)c)[r] = (uint16_t)v.v0; break;
    case K_INT32:
    case K_UINT32:
    case K_FLOAT32: ((uint32_t *)c)[r] = (uint32_t)v.v0; break;
    case K_BIN128: store_value_k<K_BIN128>(col, r, v); break;
    case K_BIN256: store_value_k<K_BIN256>(col, r, v); break;
    default: ((uint64_t *)c)[r] = v.v0; break;
    }
    return ok;
}

// ---- record trailer: DecodeMessageTable, internal/decode/msg.go:14-99 -------------------

struct Trailer {
    uint32_t st;     // spec_status
    bool big;
    long long tstart, dstart; // source positions
    uint32_t dsize, tsize;
};

// LIST = false: DecodeMessageTable (internal/decode/msg.go:14-99), 3/6-byte entries;
// LIST = true: DecodeListTable (internal/decode/list.go:14-98), 2/4-byte entries.
template <bool LIST = false, class Src>
__device__ __forceinline__ Trailer parse_trailer(const Src &s, typename Src::pos_t rs, typename Src::pos_t re) {
    Trailer tr = {ST_OK, false, 0, 0, 0, 0};
    long long len = (long long)(re - rs);
    Tail t = load_tail(s, re);
    uint32_t type = (uint32_t)t.q0 & 0xff;
    const uint32_t T_SMALL = LIST ? T_LIST : T_MESSAGE, T_BIG = LIST ? T_BIG_LIST : T_BIG_MESSAGE;
    const uint32_t ESMALL = LIST ? 2u : 3u, EBIG = LIST ? 4u : 6u;
    if (type != T_SMALL && type != T_BIG) {
        tr.st = ST_INVALID_TYPE;
        return tr;
    }
    tr.big = type == T_BIG;
    uint64_t R = tail_r(t);
    uint32_t R2 = tail_r2(t);
    int m1, m2;
    uint32_t tsz = (uint32_t)rvarint<5>(R, R2, len - 1, m1);
    if (m1 < 0) {
        tr.st = ST_INVALID_TABLE_SIZE;
        return tr;
    }
    // the data-size varint ends m1 bytes further down: shift the window
    uint64_t Rs = (R >> (8 * m1)) | ((uint64_t)R2 << (64 - 8 * m1));
    uint32_t R2s = m1 >= 2 ? 0u : (R2 >> (8 * m1));
    uint32_t dsz = (uint32_t)rvarint<5>(Rs, R2s, len - 1 - m1, m2);
    if (m2 < 0) {
        tr.st = ST_INVALID_DATA_SIZE;
        return tr;
    }
    long long tend = (long long)(re - 1) - m1 - m2;
    long long ts = tend - (long long)tsz;
    if (ts < (long long)rs || tsz % (tr.big ? EBIG : ESMALL) != 0) {
        tr.st = ST_INVALID_TABLE;
        return tr;
    }
    if (ts - (long long)dsz < (long long)rs) {
        tr.st = ST_INVALID_DATA;
        return tr;
    }
    tr.tstart = ts;
    tr.dstart = ts - (long long)dsz;
    tr.dsize = dsz;
    tr.tsize = tsz;
    return tr;
}

// ---- generic path: any record, run-time schema -----------------------------------------

// OpenMessageErr of one record: trailer + whether the table's tags are strictly increasing
// (then a probe at a field's expected index finds what the reference's binary search finds).
struct RecInfo {
    Trailer tr;
    bool ok, sorted;
    uint32_t nent;
};

template <class Src>
__device__ __forceinline__ RecInfo rec_open(const Src &s, typename Src::pos_t rs, typename Src::pos_t re) {
    using pos_t = typename Src::pos_t;
    RecInfo ri;
    ri.tr = Trailer{ST_OK, false, 0, 0, 0, 0};
    ri.ok = false;
    ri.sorted = true;
    ri.nent = 0;
    if (re > rs) {
        ri.tr = parse_trailer(s, rs, re);
        ri.ok = ri.tr.st == ST_OK;
        ri.nent = ri.tr.tsize / (ri.tr.big ? 6u : 3u);
    }
    if (ri.ok) {
        // the tags 8 entries at a time, every read of a step issued before any is compared (one
        // dependent read per entry costs a memory round trip per entry when parsing from HBM)
        const pos_t tstart = (pos_t)ri.tr.tstart;
        const uint32_t esz = ri.tr.big ? 6u : 3u;
        uint32_t prev = 0;
        bool sorted = true;
        for (uint32_t i0 = 0; i0 < ri.nent; i0 += 8) {
            uint32_t tg[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t i = i0 + u < ri.nent ? i0 + u : ri.nent - 1;
                const pos_t p = tstart + (pos_t)(i * esz);
                const uint32_t b0 = s.u8(p), b1 = s.u8(p + 1);
                tg[u] = ri.tr.big ? ((b0 << 8) | b1) : b0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t i = i0 + u;
                const bool in = i < ri.nent;
                sorted = sorted & !(in & (i > 0) & (tg[u] <= prev));
                prev = in ? tg[u] : prev;
            }
        }
        ri.sorted = sorted;
    }
    return ri;
}

// m.field(tag) (internal/types/msg.go:466-475): the field's end offset relative to the data
// start, or -1 (absent, or end > dataSize).  k = the tag's index in a Writer's table.
template <class Src>
__device__ __forceinline__ long long rec_field_end(const Src &s, const RecInfo &ri, uint32_t tag, uint32_t k) {
    using pos_t = typename Src::pos_t;
    if (!ri.ok) return -1;
    const pos_t tstart = (pos_t)ri.tr.tstart;
    long long end = -1;
    bool hit = false;
    if (ri.sorted && k < ri.nent) {
        if (ri.tr.big) {
            pos_t p = tstart + (pos_t)k * 6;
            uint32_t tg = (s.u8(p) << 8) | s.u8(p + 1);
            if (tg == tag) {
                end = ((long long)s.u8(p + 2) << 24) | (s.u8(p + 3) << 16) | (s.u8(p + 4) << 8) | s.u8(p + 5);
                hit = true;
            }
        } else {
            pos_t p = tstart + (pos_t)k * 3;
            if (s.u8(p) == tag) {
                end = (s.u8(p + 1) << 8) | s.u8(p + 2);
                hit = true;
            }
        }
    }
    if (!hit) end = table_search(s, tstart, ri.nent, ri.tr.big, tag);
    if (end > (long long)ri.tr.dsize) end = -1; // m.field: end > dataSize => nil
    return end;
}

// Parse record r occupying [rs, re) of the source into fs's columns; to_stream converts a
// source position to a stream offset (string/bytes spans).  Kind K_LIST fields are skipped.
// PRESENT: also fs.present[r], bit f = m.HasField(tag f) on the m of OpenMessageErr: the lookup
// finds the tag and its end lies within the data (an entry with end 0 is present; a record
// that does not open is the empty Message: no bit).
template <bool PRESENT = false, class Src>
__device__ __forceinline__ void decode_record_generic(const Src &s, typename Src::pos_t rs, typename Src::pos_t re,
                                                      uint64_t r, const FieldSet &fs, long long to_stream) {
    using pos_t = typename Src::pos_t;
    const RecInfo ri = rec_open(s, rs, re);
    if (fs.status) fs.status[r] = (uint8_t)ri.tr.st;
    const pos_t dstart = (pos_t)ri.tr.dstart;
    uint64_t errs = 0, pres = 0;
    for (uint32_t f = 0; f < fs.nfields; f++) {
        const uint32_t kind = fs.kinds[f];
        if (kind == K_LIST) continue;
        const long long end = rec_field_end(s, ri, fs.tags[f], fs.rank[f]);
        const bool ok = decode_store(s, kind, dstart, end, to_stream, fs.cols[f], r);
        if (!ok && f < 64) errs |= 1ull << f;
        if constexpr (PRESENT) pres |= (end >= 0 && f < 64) ? 1ull << f : 0ull;
    }
    if (fs.errmask) fs.errmask[r] = errs;
    if constexpr (PRESENT) fs.present[r] = pres;
}

// ---- fast paths: compile-time schema -----------------------------------------------------
// Two of them, over the same Spec and the same value decoders:
//   * register-resident (FastRec, FieldLoad / FieldNat / FieldStore, fast_prepare / fast_finish):
//     the whole record's windows in registers, fields in schema order, list extents.  What the
//     nested decode kernels run on outer records and items (decode_nested_core.hpp): small
//     tables of at most FAST_MAX_FIELDS fields.
//   * batched (WideField, wide_batch, fast_wide): the table walked FAST_BATCH entries at a time,
//     fields in table order.  What every generated flat kernel runs (decode_flat_pair): any
//     field count, small or big tables.

// A run-time schema has no fast path (the nested kernels' marker for "this level is generic").
struct RuntimeSpec {
    static constexpr int N = 0;
    static constexpr bool big = false;
};

// Spec (generated by jit.cpp) provides:
//   N              number of fields (1..SPEC_KFIELDS)
//   kind[f], rank[f]  per schema field
//   stag[k]        k-th tag of the table a Writer emits (strictly increasing)
//   order[k]       the schema field of table entry k (rank's inverse)
//   big            the Writer's tables are big for every record (a tag > 255: IsBigMessage,
//                  internal/format/msg.go:43-61)

// Most fields of the register-resident path, and of the flat decode's ranked tables (fast_wide).
constexpr int FAST_MAX_FIELDS = 24;

// ---- reading table entries from the slab ---------------------------------------------------
// A run of table entries starting at slab position p0, read with a few wide LDS reads and
// re-aligned into qwords: c[j] = bytes [p0+8j, p0+8j+8), each a 64-bit funnel shift of two of the
// NC + 1 aligned qwords covering the run.  (No select between array elements here: in the
// not-yet-unrolled loop LLVM folds `hi ? d[i+1] : d[i]` into a load at a variable index, which
// after unrolling is a 2N-deep v_cndmask chain per dword.)
template <int NC>
__device__ __forceinline__ void table_qwords(const LdsSrc &s, int p0, uint64_t (&c)[NC]) {
    const int base = p0 & ~7;
    const uint32_t sh = 8u * (uint32_t)(p0 & 7);
    uint64_t q[NC + 1];
#pragma unroll
    for (int j = 0; j <= NC; j++) q[j] = s.d64(base + 8 * j);
#pragma unroll
    for (int j = 0; j < NC; j++) c[j] = (q[j] >> sh) | ((q[j + 1] << 1) << (63 - sh));
}
// (The callers pick the entries' bytes out of c[] themselves — a small table's entry is u8 tag |
// u16 end, a big one's u16 tag | u32 end, internal/format/msg.go:138-186, big-endian: with that
// loop in a function of its own the generated kernels come out scheduled differently.)

// ---- the register-resident fast path (nested decode) --------------------------------------

// Unrolled at compile time: field F's kind and table index are constants, so every field
// is straight-line code.  Phase 1 issues every field's LDS reads, phase 2 decodes and
// stores, so the LDS latency is paid once per record, not once per field.
template <class Spec>
struct FastRec {
    Win w[Spec::N];
    int e[Spec::N], lo[Spec::N];
};

template <class Spec, int F>
struct FieldLoad {
    static __device__ __forceinline__ void run(FastRec<Spec> &fr, const LdsSrc &s, int ds, const uint32_t *ends,
                                               uint32_t dsize) {
        if constexpr (F < Spec::N) {
            constexpr uint32_t K = Spec::kind[F];
            const uint32_t end = ends[Spec::rank[F]];
            // end > dataSize => nil; an empty field decodes to zero: read a harmless window
            const bool has = (end <= dsize) & (end > 0);
            if constexpr (K == K_LIST) {
                // list<message> of a nested schema: only its extent [lo, e) (empty if absent)
                fr.lo[F] = ds;
                fr.e[F] = has ? ds + (int)end : ds;
            } else {
                fr.e[F] = has ? ds + (int)end : SLAB_GUARD;
                fr.lo[F] = has ? ds : SLAB_GUARD;
                // narrow windows are valid because fast_prepare only accepts natural-type records
                fr.w[F] = load_win<K, true>(s, fr.e[F]);
            }
            FieldLoad<Spec, F + 1>::run(fr, s, ds, ends, dsize);
        }
    }
};

// true iff every int/float field F is empty or has type cross_kind_type(kind[F])
template <class Spec, int F>
struct FieldNat {
    static __device__ __forceinline__ bool ok(const FastRec<Spec> &fr) {
        if constexpr (F >= Spec::N) {
            return true;
        } else {
            constexpr uint32_t NT = cross_kind_type(Spec::kind[F]);
            bool good = true;
            if constexpr (NT != 0) good = (fr.e[F] <= fr.lo[F]) | (((uint32_t)fr.w[F].t.q0 & 0xff) == NT);
            return good & FieldNat<Spec, F + 1>::ok(fr);
        }
    }
};

// ERR: also collect field F's <Kind>Err outcome into bit F of errs (a present, non-empty field
// whose decoder errs; internal/types/msg.go:233-459)
template <class Spec, int F, bool ERR = false>
struct FieldStore {
    static __device__ __forceinline__ void run(const FastRec<Spec> &fr, long long to_stream, const FieldSet &fs,
                                               uint64_t r, uint64_t &errs) {
        if constexpr (F < Spec::N) {
            constexpr uint32_t K = Spec::kind[F];
            if constexpr (K != K_LIST) {
                bool ok = true;
                const Val v = decode_tail_k<K, true>(fr.w[F], fr.lo[F], fr.e[F], to_stream, ERR ? &ok : nullptr);
                store_value_k<K>(fs.cols[F], r, v);
                if constexpr (ERR && F < 64) errs |= (!ok & (fr.e[F] > fr.lo[F])) ? (1ull << F) : 0ull;
            }
            FieldStore<Spec, F + 1, ERR>::run(fr, to_stream, fs, r, errs);
        }
    }
};

// Fast path, part 1 (LdsSrc only): trailer, table check and every field's window read into
// registers.  Returns false (nothing read into fr, nothing written) when the record needs
// the generic path.  After it returns the record's LDS bytes are no longer needed.
// Compact records (3N + 4 <= 16: list items, small messages): trailer AND table come from the
// one 16-byte tail window — [table 3N][rvarint dataSize, 1-2 bytes][3N][TypeMessage] — so
// the table needs no second round of LDS reads.  Accepts exactly what the general fast path
// accepts, restricted to a 1-2 byte data size (anything else returns false: generic path).
template <class Spec>
__device__ __forceinline__ bool fast_prepare_compact(const LdsSrc &s, int rs, int re, FastRec<Spec> &fr) {
    constexpr int N = Spec::N;
    static_assert(3 * N + 4 <= 16, "compact records only");
    const Tail t = load_tail(s, re);
    const uint32_t type = (uint32_t)t.q0 & 0xff, tsz = (uint32_t)(t.q0 >> 8) & 0xff;
    const uint32_t b3 = (uint32_t)(t.q0 >> 16) & 0xff, b4 = (uint32_t)(t.q0 >> 24) & 0xff;
    const bool two = (b3 & 0x80) != 0; // data size: reverse varint ending at re-3
    const uint32_t L = two ? 2u : 1u;
    const uint32_t dsz = two ? ((b3 & 0x7f) | ((b4 & 0x7f) << 7)) : b3;
    const int ts = re - 2 - (int)L - 3 * N, ds = ts - (int)dsz;
    bool ok = (type == T_MESSAGE) & (tsz == 3u * N) & (!two | ((b4 & 0x80) == 0)) & (ds >= rs);
    // table: shift the 128-bit tail (q1:q0, byte re-1 lowest) right past the trailer; entry
    // N-1-k then sits in bits [24k, 24k + 24) as tag | end_hi | end_lo
    const uint32_t sh = 8u * (2u + L);
    const uint64_t lo = (t.q0 >> sh) | (t.q1 << (64 - sh)), hi = t.q1 >> sh;
    uint32_t ends[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        const int bo = 24 * (N - 1 - j);
        const uint32_t ent =
            (uint32_t)((bo >= 64 ? hi >> (bo - 64) : (lo >> bo) | (bo ? hi << (64 - bo) : 0ull)) & 0xffffff);
        ok = ok & ((ent >> 16) == Spec::stag[j]);
        ends[j] = ent & 0xffff;
    }
    if (!ok) return false;
    FieldLoad<Spec, 0>::run(fr, s, ds, ends, dsz);
    return FieldNat<Spec, 0>::ok(fr);
}

template <class Spec>
__device__ __forceinline__ bool fast_prepare(const LdsSrc &s, int rs, int re, FastRec<Spec> &fr) {
    constexpr int N = Spec::N;
    static_assert(!Spec::big, "small tables only");
    if (re <= rs) return false;
    if constexpr (3 * N + 4 <= 16) return fast_prepare_compact<Spec>(s, rs, re, fr);
    Trailer tr = parse_trailer(s, rs, re);
    if ((tr.st != ST_OK) | tr.big | (tr.tsize != 3u * N)) return false;
    // the table must hold exactly the Writer's tags, so binary search would land on entry rank[f]
    uint64_t c[(3 * N + 7) / 8];
    table_qwords(s, (int)tr.tstart, c);
    auto byte_at = [&](int j) -> uint32_t { return (uint32_t)(c[j >> 3] >> (8 * (j & 7))) & 0xff; };
    bool hit = true;
    uint32_t ends[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        hit = hit & (byte_at(3 * k) == Spec::stag[k]);
        ends[k] = (byte_at(3 * k + 1) << 8) | byte_at(3 * k + 2);
    }
    if (!hit) return false;
    FieldLoad<Spec, 0>::run(fr, s, (int)tr.dstart, ends, tr.dsize);
    // every int/float field holds the type the Writer emits for its kind (or is empty): the
    // decode needs no cross-width branches (a record written under another schema version
    // takes the generic path)
    return FieldNat<Spec, 0>::ok(fr);
}

// Fast path, part 2: decode every field from registers and store the columns.
template <class Spec, bool ERR = false>
__device__ __forceinline__ void fast_finish(const FastRec<Spec> &fr, uint64_t r, const FieldSet &fs,
                                            long long to_stream) {
    uint64_t errs = 0;
    FieldStore<Spec, 0, ERR>::run(fr, to_stream, fs, r, errs);
    if (fs.status) fs.status[r] = ST_OK;
    if constexpr (ERR) fs.errmask[r] = errs;
}

// ---- the batched fast path (flat decode) ----------------------------------------------------
// Every generated flat kernel: any field count, small tables or (a tag > 255) big ones.  The
// trailer is checked (table_accepted); then the table is walked in batches of FAST_BATCH entries:
// the batch's end offsets are read (FullTable: the Writer's whole table, checked tag by tag;
// RankedTable: a subset table, each entry at its popcount index), then the batch's fields'
// windows are read, their types checked (the type a Writer emits for the kind), decoded and stored.
// A record rejected after some batches were stored runs the generic path, which rewrites every
// column and the status, so the result never depends on where the fast path gave up.
constexpr int FAST_BATCH = 8;

template <class Spec, int J0, int K, int NB>
struct WideField {
    static __device__ __forceinline__ void load(Win (&w)[NB], int (&e)[NB], int (&lo)[NB], const LdsSrc &s, int ds,
                                                const uint32_t (&ends)[NB], uint32_t dsize) {
        if constexpr (K < NB) {
            constexpr uint32_t KD = Spec::kind[Spec::order[J0 + K]];
            const bool has = (ends[K] <= dsize) & (ends[K] > 0);
            e[K] = has ? ds + (int)ends[K] : SLAB_GUARD;
            lo[K] = has ? ds : SLAB_GUARD;
            w[K] = load_win<KD, true>(s, e[K]);
            WideField<Spec, J0, K + 1, NB>::load(w, e, lo, s, ds, ends, dsize);
        }
    }
    static __device__ __forceinline__ bool nat(const Win (&w)[NB], const int (&e)[NB], const int (&lo)[NB]) {
        if constexpr (K >= NB) {
            return true;
        } else {
            constexpr uint32_t NT = cross_kind_type(Spec::kind[Spec::order[J0 + K]]);
            bool good = true;
            if constexpr (NT != 0) good = (e[K] <= lo[K]) | (((uint32_t)w[K].t.q0 & 0xff) == NT);
            return good & WideField<Spec, J0, K + 1, NB>::nat(w, e, lo);
        }
    }
    template <bool ERR>
    static __device__ __forceinline__ void store(const Win (&w)[NB], const int (&e)[NB], const int (&lo)[NB],
                                                 long long to_stream, const FieldSet &fs, uint64_t r, uint64_t &errs) {
        if constexpr (K < NB) {
            constexpr int F = Spec::order[J0 + K];
            constexpr uint32_t KD = Spec::kind[F];
            bool ok = true;
            const Val v = decode_tail_k<KD, true>(w[K], lo[K], e[K], to_stream, ERR ? &ok : nullptr);
            store_value_k<KD>(fs.cols[F], r, v);
            if constexpr (ERR && F < 64) errs |= (!ok & (e[K] > lo[K])) ? (1ull << F) : 0ull;
            WideField<Spec, J0, K + 1, NB>::template store<ERR>(w, e, lo, to_stream, fs, r, errs);
        }
    }
};

// The bits a record's decode collects besides its columns: the <Kind>Err outcomes (ERR kernels) and
// the HasField bits (PRESENT kernels), both in schema order.
struct RecMasks {
    uint64_t errs = 0, pres = 0;
};

// Which table a record's batches are read from (wide_batch has the two readers):
// FullTable: the Writer's whole table (table_accepted's full form), rank k is entry k.  PRESENT:
// the kernel collects HasField bits.
template <bool PRESENT>
struct FullTable {
    static constexpr bool ranked = false, present = PRESENT;
};
// RankedTable: a small table of k <= N entries (table_accepted's sparse form; PRESENT kernels).  A
// Writer that skipped some setters leaves a table whose tags are a strictly increasing subset of
// the schema's, so the reference's binary search finds exactly those tags and the entry of the tag
// of rank j sits at index popcount(ranks present below j).  ranks: the ranks the table holds
// (present_ranks).
struct RankedTable {
    static constexpr bool ranked = true;
    uint32_t ranks;
};

// The tags of a schema's Writer table as a 256-bit set (tags <= 255), one word per 64 tags.
template <class Spec>
struct TagSet {
    static constexpr uint64_t word(int w) {
        uint64_t v = 0;
        for (int k = 0; k < Spec::N; k++)
            if ((int)(Spec::stag[k] >> 6) == w) v |= 1ull << (Spec::stag[k] & 63);
        return v;
    }
};

// The ranks (positions in the full Writer table) of the tags a small table at ts holds, nent <= N
// entries; false unless they are strictly increasing and all the schema's.  One byte read per
// entry (unrolled over N, entries past nent read entry 0 and count for nothing).
template <class Spec>
__device__ __forceinline__ bool present_ranks(const LdsSrc &s, int ts, uint32_t nent, uint32_t &ranks) {
    constexpr int N = Spec::N;
    static_assert(N <= 32 && !Spec::big, "rank masks of small tables only");
    uint32_t tag[N];
#pragma unroll
    for (int j = 0; j < N; j++) tag[j] = s.u8(ts + ((uint32_t)j < nent ? 3 * j : 0));
    // the table's tags as a set, kept only for the words the schema has tags in (a tag in
    // another word is foreign)
    constexpr uint64_t set[4] = {TagSet<Spec>::word(0), TagSet<Spec>::word(1), TagSet<Spec>::word(2),
                                 TagSet<Spec>::word(3)};
    constexpr uint32_t words = (set[0] ? 1u : 0u) | (set[1] ? 2u : 0u) | (set[2] ? 4u : 0u) | (set[3] ? 8u : 0u);
    uint64_t have[4] = {0, 0, 0, 0};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const bool in = (uint32_t)j < nent;
        if (j > 0) ok = ok & (!in | (tag[j] > tag[j - 1]));
        ok = ok & (!in | (((words >> (tag[j] >> 6)) & 1u) != 0));
        const uint64_t bit = in ? 1ull << (tag[j] & 63) : 0ull;
#pragma unroll
        for (int w = 0; w < 4; w++)
            if (set[w]) have[w] |= (words == (1u << w) || (tag[j] >> 6) == (uint32_t)w) ? bit : 0ull;
    }
#pragma unroll
    for (int w = 0; w < 4; w++) ok = ok & ((have[w] & ~set[w]) == 0); // no foreign tag
    ranks = 0;
#pragma unroll
    for (int k = 0; k < N; k++) ranks |= (uint32_t)((have[Spec::stag[k] >> 6] >> (Spec::stag[k] & 63)) & 1) << k;
    return ok;
}

// Table ranks [J0, J1) of one record: their end offsets from the table t at ts, the fields'
// windows, type check, decode and store.  false when the record needs the generic path.  m gets the
// batch's error-mask bits (ERR) and HasField bits.
template <class Spec, int J0, int J1, bool ERR, class Table>
__device__ __forceinline__ bool wide_batch(const LdsSrc &s, const Table &t, int ts, int ds, uint32_t dsize, uint64_t r,
                                           const FieldSet &fs, long long to_stream, RecMasks &m) {
    constexpr int NB = J1 - J0;
    uint32_t ends[NB];
    if constexpr (Table::ranked) {
        // each field's ONE entry read from the slab at its popcount index (an absent field reads an
        // entry or the trailer behind the table and drops it)
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const int p = ts + 3 * (int)__builtin_popcount(t.ranks & ((1u << (J0 + k)) - 1u));
            const uint32_t end = (s.u8(p + 1) << 8) | s.u8(p + 2);
            const bool has = ((t.ranks >> (J0 + k)) & 1) != 0;
            ends[k] = has ? end : ~0u; // (~0 > dsize: absent to WideField::load as to m.field)
            m.pres |= (has & (end <= dsize)) ? 1ull << Spec::order[J0 + k] : 0ull;
        }
    } else {
        // the batch's entries, checked tag by tag; the table holds every tag, so HasField(tag) is
        // "its end lies within the data"
        constexpr int ESZ = Spec::big ? 6 : 3;
        uint64_t c[(ESZ * NB + 7) / 8];
        table_qwords(s, ts + ESZ * J0, c);
        auto byte_at = [&](int j) -> uint32_t { return (uint32_t)(c[j >> 3] >> (8 * (j & 7))) & 0xff; };
        bool hit = true;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            if constexpr (Spec::big) {
                hit = hit & (((byte_at(6 * k) << 8) | byte_at(6 * k + 1)) == Spec::stag[J0 + k]);
                ends[k] = (byte_at(6 * k + 2) << 24) | (byte_at(6 * k + 3) << 16) | (byte_at(6 * k + 4) << 8) |
                          byte_at(6 * k + 5);
            } else {
                hit = hit & (byte_at(3 * k) == Spec::stag[J0 + k]);
                ends[k] = (byte_at(3 * k + 1) << 8) | byte_at(3 * k + 2);
            }
        }
        if (!hit) return false;
        if constexpr (Table::present) {
#pragma unroll
            for (int k = 0; k < NB; k++) m.pres |= ends[k] <= dsize ? 1ull << Spec::order[J0 + k] : 0ull;
        }
    }
    Win w[NB];
    int e[NB], lo[NB];
    WideField<Spec, J0, 0, NB>::load(w, e, lo, s, ds, ends, dsize);
    if (!WideField<Spec, J0, 0, NB>::nat(w, e, lo)) return false;
    WideField<Spec, J0, 0, NB>::template store<ERR>(w, e, lo, to_stream, fs, r, m.errs);
    return true;
}

// table ranks [J0, JE) in batches of FAST_BATCH (one wave's part of a record)
template <class Spec, int J0, int JE, bool ERR>
struct WideBatchesTo {
    template <class Table>
    static __device__ __forceinline__ bool run(const LdsSrc &s, const Table &t, int ts, int ds, uint32_t dsize,
                                               uint64_t r, const FieldSet &fs, long long to_stream, RecMasks &m) {
        if constexpr (J0 >= JE) {
            return true;
        } else {
            constexpr int J1 = J0 + FAST_BATCH < JE ? J0 + FAST_BATCH : JE;
            if (!wide_batch<Spec, J0, J1, ERR>(s, t, ts, ds, dsize, r, fs, to_stream, m)) return false;
            return WideBatchesTo<Spec, J1, JE, ERR>::run(s, t, ts, ds, dsize, r, fs, to_stream, m);
        }
    }
};

// Part h of P of a record's fields: table ranks [lo(h), lo(h + 1)); for a pair the boundary is
// the batch boundary near N/2.
template <class Spec, int P>
__host__ __device__ constexpr int flat_part_lo(int h) {
    if (h >= P) return Spec::N;
    // (at most N: for 2..7 fields the rounded-up boundary lay past the table, the generated source
    // did not compile and the schema ran on the generic kernel; the first wave takes all of them)
    if (P == 2) {
        const int mid = ((Spec::N / 2 + FAST_BATCH - 1) / FAST_BATCH) * FAST_BATCH;
        return h == 0 ? 0 : (mid < Spec::N ? mid : Spec::N);
    }
    return (h * Spec::N) / P;
}
// part h (wave-uniform, run-time) -> its compile-time range of ranks
template <class Spec, bool ERR, int P, class Table, int H = 0>
__device__ __forceinline__ bool wide_part_run(const LdsSrc &s, const Table &t, const Trailer &tr, uint64_t r,
                                              const FieldSet &fs, long long to_stream, int h, RecMasks &m) {
    if constexpr (H >= P) {
        return true;
    } else {
        constexpr int J0 = flat_part_lo<Spec, P>(H), J1 = flat_part_lo<Spec, P>(H + 1);
        if (h == H)
            return WideBatchesTo<Spec, J0, J1, ERR>::run(s, t, (int)tr.tstart, (int)tr.dstart, tr.dsize, r, fs,
                                                         to_stream, m);
        return wide_part_run<Spec, ERR, P, Table, H + 1>(s, t, tr, r, fs, to_stream, h, m);
    }
}

// The two trailers the batched fast path takes; every other record runs the generic path.
//   full:   the table is of the size and entry width of the Writer's whole table (wide_batch then
//           checks its tags);
//   sparse: a small table of at most N entries (present_ranks then checks its tags).
// (Written as "none of the reasons to reject": the conjunction of the positive tests compiles to
// other code.)
template <class Spec, bool SPARSE>
__device__ __forceinline__ bool table_accepted(const Trailer &tr) {
    if constexpr (SPARSE)
        return !((tr.st != ST_OK) | tr.big | (tr.tsize > 3u * (uint32_t)Spec::N));
    else
        return !((tr.st != ST_OK) | (tr.big != Spec::big) | (tr.tsize != (Spec::big ? 6u : 3u) * (uint32_t)Spec::N));
}

// Part h of P of record r (slab positions [rs, re)) for wave h of the record's group
// (decode_flat_pair): false when this part needs the generic path.  No status: the group's first
// wave writes it once every part succeeded.  m gets this part's error-mask bits (ERR) and HasField
// bits.
// A PRESENT kernel of a small-table schema of at most FAST_MAX_FIELDS fields takes the sparse form
// (the full table included): every wave of the group reads the whole tag column, since it needs
// the ranks below its own part.  Every other kernel takes the full form; a PRESENT kernel of a
// wide or big-table schema so sends a subset table to the generic path.
template <class Spec, bool ERR = false, int P = 2, bool PRESENT = false>
__device__ __forceinline__ bool fast_wide(const LdsSrc &s, int rs, int re, uint64_t r, const FieldSet &fs,
                                          long long to_stream, int h, RecMasks &m) {
    constexpr bool SPARSE = PRESENT && Spec::N <= FAST_MAX_FIELDS && !Spec::big;
    if (re <= rs) return false;
    const Trailer tr = parse_trailer(s, rs, re);
    if (!table_accepted<Spec, SPARSE>(tr)) return false;
    if constexpr (SPARSE) {
        RankedTable t;
        if (!present_ranks<Spec>(s, (int)tr.tstart, tr.tsize / 3u, t.ranks)) return false;
        return wide_part_run<Spec, ERR, P>(s, t, tr, r, fs, to_stream, h, m);
    } else {
        return wide_part_run<Spec, ERR, P>(s, FullTable<PRESENT>{}, tr, r, fs, to_stream, h, m);
    }
}

// ---- staging a span of the stream into LDS -------------------------------------------------
// One primitive for every kernel that parses from LDS (flat, nested, validate, tree rows): a
// wave-uniform span of the stream is copied into a slab with LDS-DMA (buffer_load_dwordx4 ... lds:
// 16 bytes per lane, 1 KiB per instruction, range-checked by the buffer descriptor), by one wave or
// by the P waves of a group, which take the 1 KiB chunks round-robin.
//   * origin: the span start rounded down to 16 bytes of the stream offset;
//   * extent: whole 1 KiB chunks (what they hold past the span is never looked at);
//   * AUX: the cache policy of the loads (the builtin's aux operand: 0 default, 2 = nt);
//   * the 16-byte granule straddling the stream end comes back zeroed (whole-access range check)
//     and is refilled bytewise by the wave that issued it.
// Measured and not kept (DESIGN.md 3.1 "request shape"): nt on the stream, an origin on a 128-byte
// line of the address, a last chunk with its upper lanes masked.
constexpr int STREAM_AUX = 0;

struct Staged {
    uint64_t origin;   // stream offset of the slab's first staged byte (a multiple of 16)
    uint32_t granules; // 16-byte granules covering the span: stream bytes [origin, origin + 16 granules)
    __device__ __forceinline__ uint32_t chunks() const { return (granules + 63) >> 6; }
    // LDS bytes the staging writes (whole chunks)
    __device__ __forceinline__ uint32_t bytes() const { return chunks() * 1024; }
};

// The staging of stream bytes [lo, hi) (wave-uniform; hi <= lo stages nothing).
__device__ __forceinline__ Staged stage_plan(uint64_t lo, uint64_t hi) {
    Staged st;
    st.origin = lo & ~15ull;
    st.granules = hi > st.origin ? (uint32_t)((hi - st.origin + 15) >> 4) : 0;
    return st;
}

// Wave `part` of `parts` issues its chunks of st into dst (16-byte aligned LDS, room for
// st.bytes()); nothing is waited for.
template <int AUX>
__device__ __forceinline__ void stage_issue(__amdgpu_buffer_rsrc_t rsrc, uint8_t *dst, const Staged &st, int lane,
                                            int part = 0, int parts = 1) {
    // (wave-uniform values the compiler cannot prove uniform: a scalar loop, the LDS address in M0)
    const uint32_t n = __builtin_amdgcn_readfirstlane(st.chunks());
    for (uint32_t c = __builtin_amdgcn_readfirstlane((uint32_t)part); c < n; c += (uint32_t)parts)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + c * 1024), 16,
                                                 (uint32_t)st.origin + c * 1024 + lane * 16, 0, 0, AUX);
}

// Once the wave's own loads have landed (s_waitcnt vmcnt(0)): the one refill of the granule that
// straddles stream_len, by the wave that issued it.  The wave's later LDS reads see it; other
// waves of the group after their barrier.
__device__ __forceinline__ void stage_fix_tail(__amdgpu_buffer_rsrc_t rsrc, uint8_t *dst, const Staged &st,
                                               uint64_t stream_len, int lane, int part = 0, int parts = 1) {
    const uint64_t tail = stream_len & ~15ull; // (origin is a multiple of 16: granules start on multiples of 16)
    if (tail < stream_len && tail >= st.origin && tail < st.origin + st.bytes() &&
        (int)(((tail - st.origin) >> 10) % (uint32_t)parts) == part) {
        if (lane < 16 && tail + lane < stream_len)
            dst[(tail - st.origin) + lane] = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rsrc, (uint32_t)(tail + lane), 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// Issue, wait, refill: st's bytes are in dst when this returns (for a group of waves: this wave's
// chunks; the slab is whole after the group's barrier).
template <int AUX>
__device__ __forceinline__ void stage_span(__amdgpu_buffer_rsrc_t rsrc, uint8_t *dst, const Staged &st,
                                           uint64_t stream_len, int lane, int part = 0, int parts = 1) {
    stage_issue<AUX>(rsrc, dst, st, lane, part, parts);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stage_fix_tail(rsrc, dst, st, stream_len, lane, part, parts);
}

// One wave's group of 64 consecutive records: per-lane record bounds and the wave's span, staged
// (if it fits) at slab + SLAB_GUARD.
struct Group {
    uint64_t rec_lo, rec_hi; // this lane's record [rec_lo, rec_hi) in the stream
    Staged st;               // the span's staging (wave-uniform)
    bool in_lds;             // span fits the slab (wave-uniform)
    // the lane's record in slab positions, and slab position -> stream offset
    __device__ __forceinline__ int rs() const { return SLAB_GUARD + (int)(rec_lo - st.origin); }
    __device__ __forceinline__ int re() const { return SLAB_GUARD + (int)(rec_hi - st.origin); }
    __device__ __forceinline__ long long to_stream() const { return (long long)st.origin - SLAB_GUARD; }
};

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return __builtin_amdgcn_readfirstlane((uint32_t)v) |
           ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32);
}

// ends[] of group g, as (lo, hi) per lane: lo = ends[r-1] (0 for record 0), hi = ends[r].
__device__ __forceinline__ void load_group_ends(const DecodeArgs &a, uint64_t base, int lane, uint64_t &lo,
                                                uint64_t &hi) {
    const uint64_t r = base + lane;
    const uint64_t last = a.n - 1;
    hi = a.ends[r < last ? r : last];
    lo = (r == 0 ? 0 : a.ends[(r - 1) < last ? r - 1 : last]) + a.head;
}

// The group of lanes [l0, l1) of the 64 records from `base` (the whole group: 0, 64).  The slab
// keeps 16 bytes past the staged chunks: a parser reads up to 7 bytes past a record end.
__device__ __forceinline__ Group make_group(uint64_t n, uint64_t base, uint64_t lo, uint64_t hi, uint32_t slab,
                                            int l0 = 0, int l1 = 64) {
    Group gr;
    gr.rec_lo = lo;
    gr.rec_hi = hi < lo ? lo : hi; // malformed ends: treat as empty
    const int nrec = (int)(n - base < 64 ? n - base : 64);
    const int last = (l1 < nrec ? l1 : nrec) - 1;
    const uint64_t span_lo = uniform64(__shfl(lo, l0));
    const uint64_t span_hi = uniform64(__shfl(hi, last < 0 ? 0 : last));
    gr.st = stage_plan(span_lo, span_hi);
    gr.in_lds = slab > 0 && l0 <= last && span_hi >= span_lo && SLAB_GUARD + (uint64_t)gr.st.bytes() + 16 <= (uint64_t)slab;
    return gr;
}

// ---- the flat decode's kernel bodies ---------------------------------------------------------
// Which path a schema's records take, by the kernel that decodes them:
//   run-time schema (decode_flat.hip: decode_flat_kernel, decode_flat_present_kernel; every
//   schema with the generated kernels switched off)
//       decode_flat_runtime: a group per wave -> decode_record_generic for every record;
//   generated, plain or _err (jit.cpp: spec_decode_flat[_wide][_err]_pair_jit), and generated
//   _present of a schema of more than FAST_MAX_FIELDS fields or with a tag > 255
//       decode_flat_pair: a group per P waves -> fast_wide, full form (FullTable);
//   generated _present, small tables, at most FAST_MAX_FIELDS fields
//       decode_flat_pair -> fast_wide, sparse form (present_ranks, RankedTable);
//   and under every generated kernel: a record fast_wide rejects, or a group whose span does
//   not fit the slab -> decode_record_generic.

// Block b's place among the grid's blocks.  Blocks are dealt round-robin to the 8 XCDs: with
// a.xcd = 1, block b takes the b/8-th slot of XCD b%8's contiguous share, so neighbouring groups
// (which share the narrow columns' cache lines) are written through one L2.
__device__ __forceinline__ uint64_t flat_block(const DecodeArgs &a) {
    uint64_t blk = blockIdx.x;
    if (a.xcd) {
        const uint64_t per = (gridDim.x + 7) / 8;
        blk = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    }
    return blk;
}

// Opens the group of the 64 records from base (< a.n): this lane's record bounds from ends[] (one
// load per lane, the lower bound from the lane below) and the group's span.
__device__ __forceinline__ Group open_group(const DecodeArgs &a, uint64_t base, int lane) {
    const uint64_t r = base + lane;
    const uint64_t hi = a.ends[r < a.n ? r : a.n - 1];
    uint64_t lo = __shfl_up(hi, 1);
    if (lane == 0) lo = r == 0 ? 0 : a.ends[r - 1];
    lo += a.head;
    return make_group(a.n, base, lo, hi, a.slab);
}

// Run-time schema: one group per wave (blockDim / 64 groups per block): stage, decode every
// record on the generic path, done.  It writes a.f.errmask when that is set
// (spec_decode_flat_errors).  PRESENT: with the HasField masks (a.f.present,
// spec_decode_flat_present).
template <bool PRESENT = false>
__device__ __forceinline__ void decode_flat_runtime(const DecodeArgs &a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const uint64_t blk = flat_block(a);
    const uint64_t base = a.r0 + (blk * (blockDim.x >> 6) + wave) * 64;
    if (base >= a.n) return;
    const uint64_t r = base + lane;
    const bool valid = r < a.n;
    uint8_t *slab = smem + wave * a.slab;
    __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(a.stream, a.stream_len);
    const Group cur = open_group(a, base, lane);
    if (cur.in_lds) {
        stage_span<STREAM_AUX>(rsrc, slab + SLAB_GUARD, cur.st, a.stream_len, lane);
        if (!valid) return;
        LdsSrc s{(lds_u8 *)slab};
        decode_record_generic<PRESENT>(s, cur.rs(), cur.re(), r, a.f, cur.to_stream());
    } else if (valid) {
        GlobalSrc s{a.stream, a.stream_len};
        decode_record_generic<PRESENT>(s, (long long)cur.rec_lo, (long long)cur.rec_hi, r, a.f, 0);
    }
}

// Generated kernels: a group of 64 records on a wave PAIR (a 128-thread block): both waves stage
// the group's span once in the block's slab (each issues half the LDS-DMA chunks), each decodes
// half of the fields (fast_wide), wave 1 hands its verdict to wave 0 through LDS, and wave 0
// writes the status — or, where either half needs it, runs the generic path over the whole
// record (it rewrites every column).  Same LDS per 64 records, twice the waves: one wave's LDS
// and memory latency overlaps the other's decode.  ERR: every wave's mask bits, OR-ed by wave 0.
// P waves per group in general (P parts of the fields; jit.cpp FLAT_WAVES).
// PRESENT: also the HasField masks (a.f.present, spec_decode_flat_present), every wave's bits OR-ed
// by wave 0 like the error bits.
template <class Spec, bool ERR = false, int P = 2, bool PRESENT = false>
__device__ __forceinline__ void decode_flat_pair(const DecodeArgs &a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const uint64_t blk = flat_block(a);
    const uint64_t base = a.r0 + blk * 64;
    if (base >= a.n) return; // (block-uniform)
    const uint64_t r = base + lane;
    const bool valid = r < a.n;
    uint8_t *slab = smem;
    uint32_t *xch = (uint32_t *)(smem + a.slab);
    __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(a.stream, a.stream_len);
    const Group cur = open_group(a, base, lane);
    if (!cur.in_lds) {
        if (wave == 0 && valid) {
            GlobalSrc s{a.stream, a.stream_len};
            decode_record_generic<PRESENT>(s, (long long)cur.rec_lo, (long long)cur.rec_hi, r, a.f, 0);
        }
        return;
    }
    stage_span<STREAM_AUX>(rsrc, slab + SLAB_GUARD, cur.st, a.stream_len, lane, wave, P);
    __syncthreads(); // the slab is whole
    LdsSrc s{(lds_u8 *)slab};
    const int rs = cur.rs(), re = cur.re();
    const long long to_stream = cur.to_stream();
    RecMasks mine;
    const bool ok = valid && fast_wide<Spec, ERR, P, PRESENT>(s, rs, re, r, a.f, to_stream, wave, mine);
    // waves 1 .. P-1: verdicts at slab + 256 (w - 1), ERR: mask bits after them (512 B per wave),
    // PRESENT: HasField bits after those (512 B per wave)
    uint64_t *xerr = (uint64_t *)(xch + 64 * (P - 1));
    uint64_t *xpres = xerr + (ERR ? 64 * (P - 1) : 0);
    if (wave > 0) {
        xch[64 * (wave - 1) + lane] = ok ? 1u : 0u;
        if constexpr (ERR) xerr[64 * (wave - 1) + lane] = mine.errs;
        if constexpr (PRESENT) xpres[64 * (wave - 1) + lane] = mine.pres;
    }
    __syncthreads(); // the other waves' verdicts (and their column stores) are in
    if (wave == 0 && valid) {
        bool all = ok;
        uint64_t m = mine.errs, pm = mine.pres;
#pragma unroll
        for (int w = 1; w < P; w++) {
            all = all && xch[64 * (w - 1) + lane] != 0;
            if constexpr (ERR) m |= xerr[64 * (w - 1) + lane];
            if constexpr (PRESENT) pm |= xpres[64 * (w - 1) + lane];
        }
        if (all) {
            if (a.f.status) a.f.status[r] = ST_OK;
            if constexpr (ERR) a.f.errmask[r] = m;
            if constexpr (PRESENT) a.f.present[r] = pm;
        } else {
            decode_record_generic<PRESENT>(s, rs, re, r, a.f, to_stream);
        }
    }
}

// Launch shape of the flat decode's wave-per-group kernels: per-wave slab, grid.
struct DecodeLaunch {
    uint32_t slab; // bytes per wave = dynamic LDS per block
    unsigned blocks;
};

// One group per wave, one wave per block (packs the most slabs per CU: LDS is the occupancy
// limit), the grid rounded up to 8 equal XCD shares (the kernels' a.xcd block order).
__host__ inline DecodeLaunch decode_launch(uint64_t nrec, double avg_record) {
    DecodeLaunch L;
    L.slab = decode_slab_bytes(avg_record);
    L.blocks = (unsigned)(((nrec + 63) / 64 + 7) / 8 * 8);
    return L;
}

} // namespace spec

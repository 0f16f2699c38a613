// jit_tree.cpp — the schema-tree kernels compiled at run time (jit_module.hpp): the generated
// readers, one kernel per decode group, and the generated size passes and writers of the encoder.
//
// For every group root x (the records or a list table) whose message tables qualify (direct
// tags unique and <= 255), a kernel spec_tree_group_<x> whose row code is the generated reader
// of internal/lang/generator/message.go:97-186 with every tag, kind, rank and column index a
// constant: tree_open checks the table against the schema's tag set once, every getter is then
// one table read and a kind-specialised decode; a row whose table does not qualify (unsorted,
// big, foreign tags) runs the run-time reader (tree_message_row), so results never depend on
// which path ran.  Structs are the generated Decode (struct.go:75-113), members last-first.
#include <sstream>
#include <string>
#include <vector>
#include <cstdio>

#include "jit_module.hpp"
#include "spec_internal.hpp"
#include "tree_internal.hpp"

namespace {

using namespace spec::jit;
using spec::TreeDesc;
using spec::TField;
using spec::TTable;

bool tree_table_ok(const TreeDesc &D, uint32_t t) {
    const TTable &T = D.t[t];
    if (T.shape != spec::SHAPE_MESSAGE) return true;
    if (T.nd > 64) return false;
    bool seen[256] = {false};
    for (uint32_t k = 0; k < T.nd; k++) {
        const uint32_t tag = D.f[D.direct[T.d0 + k]].tag;
        if (tag > 255 || seen[tag]) return false;
        seen[tag] = true;
    }
    return true;
}

bool tree_group_ok(const TreeDesc &D, uint32_t x) {
    const TTable &T = D.t[x];
    // a group of more than 24 tables (sub-messages decoded with their owner) runs the run-time
    // kernel: its generated reader is inlined per source and wave variant
    if (T.gn > 24) return false;
    for (uint32_t g = 0; g < T.gn; g++)
        if (!tree_table_ok(D, D.group[T.g0 + g])) return false;
    return true;
}

std::string col_expr(int c) {
    if (c < 0) return "(void *)nullptr";
    return "B.cols[" + std::to_string(c) + "]";
}

// the members of struct field sf, last first, decoded below OFF down to LB (depth d variables)
void gen_struct_members(std::ostringstream &o, const TreeDesc &D, uint32_t sf, const std::string &LB,
                        const std::string &OFF, int d, const std::string &ind) {
    const TField &F = D.f[sf];
    for (int k = (int)F.nmem - 1; k >= 0; k--) {
        const uint32_t mi = D.members[F.mem0 + k];
        const TField &M = D.f[mi];
        if (M.kind == spec::K_STRUCT) {
            const std::string S = "S" + std::to_string(d + 1), Z = "dz" + std::to_string(d + 1),
                              O2 = "off" + std::to_string(d + 1);
            o << ind << "if (" << OFF << " > " << LB << ") { // inner struct, field " << mi << "\n"
              << ind << "  long long " << S << "; uint32_t " << Z << ";\n"
              << ind << "  sst = struct_open(s, " << LB << ", " << OFF << ", " << S << ", " << Z << ");\n"
              << ind << "  if (sst != ST_OK) break;\n"
              << ind << "  long long " << O2 << " = " << S << " + " << Z << ";\n";
            gen_struct_members(o, D, mi, S, O2, d + 1, ind + "  ");
            o << ind << "  " << OFF << " = " << S << ";\n" << ind << "}\n";
        } else {
            o << ind << "{ Val v; int n; const bool ok = decode_value_kn<" << (int)M.kind << ">(s, " << LB << ", " << OFF
              << ", 0, v, n);\n"
              << ind << "  if (" << col_expr(M.col) << ") store_value_k<" << (int)M.kind << ">(" << col_expr(M.col)
              << ", row, v);\n"
              << ind << "  if (!ok) { sst = ST_INVALID_VALUE; break; }\n"
              << ind << "  " << OFF << " -= n; }\n";
        }
    }
}

// sst = the generated Decode of struct field sf over [LO, E) (tree_core.hpp tree_struct)
void gen_struct(std::ostringstream &o, const TreeDesc &D, uint32_t sf, const std::string &LO, const std::string &E,
                const std::string &ind) {
    const TField &F = D.f[sf];
    for (uint32_t i = sf + 1; i < F.send; i++) {
        const TField &M = D.f[i];
        if (M.kind == spec::K_STRUCT || M.col < 0) continue;
        o << ind << "if (" << col_expr(M.col) << ") store_value_k<" << (int)M.kind << ">(" << col_expr(M.col)
          << ", row, Val{0, 0, 0, 0});\n";
    }
    o << ind << "if (" << E << " > " << LO << ") do {\n"
      << ind << "  long long S0; uint32_t dz0;\n"
      << ind << "  sst = struct_open(s, " << LO << ", " << E << ", S0, dz0);\n"
      << ind << "  if (sst != ST_OK) break;\n"
      << ind << "  long long off0 = S0 + dz0;\n";
    gen_struct_members(o, D, sf, "S0", "off0", 0, ind + "  ");
    o << ind << "} while (0);\n";
}

// a message table's row: lo/hi expressions, its status column written (root: a panicked range
// is ST_PANIC)
// sel (the root table of a wave pair, gen_pair_rows): only the direct fields k with sel[k] are
// decoded, and the table's status and *Err bits go to ro (RowOut) for the pair's exchange
void gen_message_table(std::ostringstream &o, const TreeDesc &D, uint32_t t, const std::string &lo,
                       const std::string &hi, bool root, const std::vector<char> *sel = nullptr,
                       const std::string &fallback = "tree_message_fallback", const std::string &on_bad = "") {
    const TTable &T = D.t[t];
    auto skip = [&](uint32_t k) { return sel && !(*sel)[k]; };
    uint64_t m[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < T.nd; k++) {
        const uint32_t tag = D.f[D.direct[T.d0 + k]].tag;
        m[tag >> 6] |= 1ull << (tag & 63);
    }
    o << "  { // table " << t << "\n"
      << "    const long long tlo = " << lo << ", thi = " << hi << ";\n"
      << "    const TOpen o = tree_open<" << T.nd << ", 0x" << std::hex << m[0] << "ull, 0x" << m[1] << "ull, 0x" << m[2]
      << "ull, 0x" << m[3] << "ull" << std::dec << ">(s, tlo, thi);\n";
    if (!on_bad.empty()) o << "    if (o.st != ST_OK) { " << on_bad << " } // the owner field's *Err bit\n";
    o << "    uint32_t st;\n"
      << "    if (o.fast) {\n"
      << "      st = o.st;\n"
      << "      const long long ds = o.ds;\n"
      << "      uint64_t *errp = " << (T.err_col >= 0 ? "(uint64_t *)" + col_expr(T.err_col) : std::string("nullptr"))
      << ";\n"
      << "      uint64_t errs = 0;\n";
    // HASMASK (a table with an optional field): bit k = the lookup found field k, end >= 0 (not
    // the scalars' end <= 0 "no value" test: an entry with end 0 is present)
    const bool hm = T.has_col >= 0;
    if (hm) o << "      uint64_t has = 0;\n";
    // the scalar fields first, as straight-line code (the kernel runs only with every column
    // present): every table read and value window of the table issued before any decode, so
    // the LDS round trips overlap; windows are read for the type a Writer emits, and a field of
    // another accepted type (ints of another width, float32 <-> float64) is decoded again
    // with the general window below
    bool any_nt = false;
    for (uint32_t k = 0; k < T.nd; k++) {
        const TField &F = D.f[D.direct[T.d0 + k]];
        if (F.kind < spec::K_BOOL || F.kind > spec::K_BYTES || skip(k)) continue;
        o << "      const long long end" << k << " = tree_end<" << F.rank << ">(s, o);\n"
          << "      const long long e" << k << " = end" << k << " > 0 ? ds + end" << k << " : ds;\n"
          << "      const Win w" << k << " = load_win<" << (int)F.kind << ", true>(s, e" << k << ");\n";
    }
    o << "      bool slow = false;\n";
    for (uint32_t k = 0; k < T.nd; k++) {
        const TField &F = D.f[D.direct[T.d0 + k]];
        if (F.kind < spec::K_BOOL || F.kind > spec::K_BYTES || skip(k)) continue;
        const uint32_t nt = spec::cross_kind_type(F.kind);
        o << "      bool ok" << k << " = true;\n"
          << "      Val v" << k << " = decode_tail_k<" << (int)F.kind << ", true>(w" << k << ", ds, e" << k << ", 0, &ok" << k
          << ");\n";
        if (nt) {
            any_nt = true;
            o << "      const bool nat" << k << " = end" << k << " <= 0 || ((uint32_t)w" << k << ".t.q0 & 0xff) == " << nt
              << "u;\n"
              << "      slow |= !nat" << k << ";\n";
        }
    }
    if (any_nt) {
        o << "      if (slow) {\n";
        for (uint32_t k = 0; k < T.nd; k++) {
            const TField &F = D.f[D.direct[T.d0 + k]];
            if (F.kind < spec::K_BOOL || F.kind > spec::K_BYTES || !spec::cross_kind_type(F.kind) || skip(k)) continue;
            o << "        if (!nat" << k << ") v" << k << " = decode_tail_k<" << (int)F.kind << ">(load_win<" << (int)F.kind
              << ">(s, e" << k << "), ds, e" << k << ", 0, &ok" << k << ");\n";
        }
        o << "      }\n";
    }
    for (uint32_t k = 0; k < T.nd; k++) {
        const TField &F = D.f[D.direct[T.d0 + k]];
        if (F.kind < spec::K_BOOL || F.kind > spec::K_BYTES || skip(k)) continue;
        const std::string bit = k < 64 ? "(1ull << " + std::to_string(k) + ")" : "0ull";
        o << "      store_value_k<" << (int)F.kind << ">(" << col_expr(F.col) << ", row, v" << k << ");\n"
          << "      errs |= (ok" << k << " || end" << k << " <= 0) ? 0ull : " << bit << ";\n";
        if (hm) o << "      has |= end" << k << " >= 0 ? " << bit << " : 0ull;\n";
    }
    for (uint32_t k = 0; k < T.nd; k++) {
        const uint32_t fi = D.direct[T.d0 + k];
        const TField &F = D.f[fi];
        if ((F.kind >= spec::K_BOOL && F.kind <= spec::K_BYTES) || skip(k)) continue;
        const std::string bit = k < 64 ? "(1ull << " + std::to_string(k) + ")" : "0ull";
        o << "      { // field " << fi << " tag " << F.tag << " kind " << (int)F.kind << "\n"
          << "        const long long end = tree_end<" << F.rank << ">(s, o);\n";
        if (hm) o << "        has |= end >= 0 ? " << bit << " : 0ull;\n";
        switch (F.kind) {
        case spec::K_MESSAGE:
            o << "        const long long e = end >= 0 ? ds + end : ds;\n"
              << "        store_u8(" << col_expr(F.present) << ", row, end >= 0 ? 1u : 0u);\n"
              << "        gr[" << D.t[F.table].gslot << " * 64] = end >= 0 ? make_uint2((uint32_t)ds, (uint32_t)e) : make_uint2(0, 0);\n";
            // (its *Err bit — the sub-message's trailer invalid — is set by the sub-table's own
            // tree_open over the same range, gen_sub_tables: the trailer is parsed once)
            break;
        case spec::K_LIST:
            o << "        const long long e = end >= 0 ? ds + end : ds;\n"
              << "        store_u8(" << col_expr(F.present) << ", row, end >= 0 ? 1u : 0u);\n"
              << "        uint32_t cnt = 0;\n"
              << "        uint4 h = make_uint4(0, 0, 0, 0);\n"
              << "        if (e > ds) {\n"
              << "          const Trailer lt = parse_trailer<true>(s, ds, e);\n"
              << "          if (lt.st == ST_OK) {\n"
              << "            cnt = lt.tsize / (lt.big ? 4u : 2u);\n"
              << "            h = make_uint4((uint32_t)lt.tstart, (uint32_t)lt.dstart, lt.dsize, cnt | (lt.big ? 0x80000000u : 0u));\n"
              << "          } else {\n"
              << "            errs |= " << bit << ";\n"
              << "          }\n"
              << "        }\n"
              << "        B.cnt[" << F.table << "][row] = cnt;\n"
              << "        B.lh[" << F.table << "][row] = h;\n";
            break;
        case spec::K_STRUCT:
            o << "        const long long e = end >= 0 ? ds + end : ds;\n"
              << "        uint32_t sst = ST_OK;\n";
            gen_struct(o, D, fi, "ds", "e", "        ");
            o << "        if (sst == ST_PANIC) st = ST_PANIC;\n"
              << "        if (sst != ST_OK) errs |= " << bit << ";\n";
            break;
        case spec::K_ANY:
            o << "        const long long e = end >= 0 ? ds + end : ds;\n"
              << "        long long n = 0;\n"
              << "        uint2 sp = make_uint2(0, 0);\n"
              << "        if (e > ds) {\n"
              << "          if (type_size_inl(s, ds, e, n)) {\n"
              << "            if (n < 0) st = ST_PANIC;\n"
              << "            else if (n > 0 && n <= e - ds) sp = make_uint2((uint32_t)(e - n), (uint32_t)n);\n"
              << "          } else {\n"
              << "            errs |= " << bit << ";\n"
              << "          }\n"
              << "        }\n"
              << "        if (" << col_expr(F.col) << ") ((uint2 *)" << col_expr(F.col) << ")[row] = sp;\n"
              << "        store_u8(" << col_expr(F.present) << ", row, sp.y ? s.u8((long long)sp.x + sp.y - 1) : 0u);\n";
            break;
        default:
            break;
        }
        o << "      }\n";
    }
    if (sel) {
        o << "      (void)errp;\n      ro.errs = errs;\n" << (hm ? "      ro.has = has;\n" : "")
          << "    } else {\n"
          << "      st = " << fallback << "(s, D, B, " << t << "u, row, tlo, thi, gr);\n"
          << "    }\n"
          << "    ro.st = st;\n    ro.fast = o.fast ? 1u : 0u;\n"
          << "  }\n";
        return;
    }
    o << "      if (errp) errp[row] = errs;\n";
    if (hm) o << "      if (" << col_expr(T.has_col) << ") ((uint64_t *)" << col_expr(T.has_col) << ")[row] = has;\n";
    o << "    } else {\n"
      << "      st = " << fallback << "(s, D, B, " << t << "u, row, tlo, thi, gr);\n"
      << "    }\n"
      << "    store_u8(" << col_expr(T.status_col) << ", row, " << (root ? "panic ? (uint32_t)ST_PANIC : st" : "st")
      << ");\n"
      << "  }\n";
}

// an eager writer's table in the Writer's tie-sorted order over the present fields (e<k> marks),
// then its trailer; `data`, `nf`, `big` in scope
void gen_table_trailer(std::ostringstream &o, const TreeDesc &D, const TTable &T) {
    o << "  if (!big) {\n";
    for (uint32_t j = 0; j < T.nd; j++) {
        const uint32_t fi = D.sorted[T.d0 + j], slot = D.sslot[T.d0 + j];
        if (D.f[fi].tag > 255) continue; // a present one makes the table big
        o << "    if (e" << slot << " != 0xffffffffu) em.put_n(" << D.f[fi].tag << "u | ((uint64_t)__builtin_bswap16((uint16_t)e"
          << slot << ") << 8), 3);\n";
    }
    o << "  } else {\n";
    for (uint32_t j = 0; j < T.nd; j++) {
        const uint32_t fi = D.sorted[T.d0 + j], slot = D.sslot[T.d0 + j];
        o << "    if (e" << slot << " != 0xffffffffu) { em.be(" << D.f[fi].tag << "u, 2); em.be(e" << slot << ", 4); }\n";
    }
    o << "  }\n"
      << "  em.rvarint(data);\n  em.rvarint((uint64_t)nf * (big ? 6 : 3));\n"
      << "  em.put1(big ? T_BIG_MESSAGE : T_MESSAGE);\n  em.finish();\n";
}

// The generated Write() of a message table (internal/lang/generator/message.go:319-439,
// internal/writer/writer.go:376-553) for one row at start: every column read issued before the
// first byte is written, then the fields in write order (constant kinds, heaps and tags), the
// table in the Writer's tie-sorted order over the present fields, the trailer.  Sub-messages and
// list elements are children written by their tables' later launches into the gaps skipped here.
// the column reads of direct field k of table T issued before the first byte (values; a
// sub-message's or list's presence; a sub-message's size)
// An optional direct field (SPEC_TREE_FIELD_OPTIONAL) in the generated writers: a compile-time
// fact per field.  Its presence test is bit k of the row's HASMASK word `hw` (gen_has_word: a
// table of up to 64 fields has one word), or the run-time lookup for a wider table; its column
// reads, its size and its bytes all sit behind the test, so an absent field's columns are never
// read.  An unflagged field's code is what it was.
std::string has_expr(const TreeDesc &D, const TTable &T, uint32_t k) {
    if (T.nd <= 64) return "((hw >> " + std::to_string(k) + ") & 1)";
    return "has_bit(B, D, D.t[" + std::to_string(&T - D.t) + "], row, " + std::to_string(k) + "u)";
}
void gen_has_word(std::ostringstream &o, const TTable &T, const char *ind) {
    if (T.has_col >= 0 && T.nd <= 64)
        o << ind << "const uint64_t hw = ((const uint64_t *)" << col_expr(T.has_col) << ")[row];\n" << ind << "(void)hw;\n";
}
// the load of a column element into v (declared here); of an optional field only when present
void gen_load(std::ostringstream &o, const std::string &v, int kind, int col, const std::string &opt, const char *ind) {
    if (opt.empty()) {
        o << ind << "uint64_t " << v << "[4];\n" << ind << "load_value_k<" << kind << ">(" << col_expr(col) << ", row, " << v
          << ");\n";
        return;
    }
    o << ind << "uint64_t " << v << "[4] = {0, 0, 0, 0};\n"
      << ind << "if (" << opt << ") load_value_k<" << kind << ">(" << col_expr(col) << ", row, " << v << ");\n";
}

void gen_field_loads(std::ostringstream &o, const TreeDesc &D, const TTable &T, uint32_t k, bool eager, const char *ind) {
    const TField &F = D.f[D.direct[T.d0 + k]];
    const std::string opt = F.opt ? has_expr(D, T, k) : std::string();
    if ((F.kind >= spec::K_BOOL && F.kind <= spec::K_BYTES) || F.kind == spec::K_ANY) {
        if (eager) gen_load(o, "a" + std::to_string(k), F.kind, F.col, opt, ind);
    } else if (F.kind == spec::K_MESSAGE || F.kind == spec::K_LIST)
        o << ind << "const uint32_t pr" << k << " = ((const uint8_t *)" << col_expr(F.present) << ")[row];\n";
    if (F.kind == spec::K_MESSAGE) o << ind << "const uint32_t sz" << k << " = B.size[" << F.table << "][row];\n";
    // a struct's member values (every scalar member of its subtree: gen_struct_emit)
    if (F.kind == spec::K_STRUCT && eager) {
        const uint32_t fi = D.direct[T.d0 + k];
        for (uint32_t i = fi + 1; i < F.send; i++)
            if (D.f[i].kind != spec::K_STRUCT) gen_load(o, "m" + std::to_string(i), D.f[i].kind, D.f[i].col, opt, ind);
    }
    // a list's element range [begin[row], begin[row + 1]) (the size pass checked BEGIN)
    if (F.kind == spec::K_LIST)
        o << ind << "const uint32_t j0_" << k << " = ((const uint32_t *)" << col_expr(D.t[F.table].begin_col) << ")[row], j1_" << k
          << " = ((const uint32_t *)" << col_expr(D.t[F.table].begin_col) << ")[row + 1];\n";
}

// struct field sf's EncodeXxxTo (internal/lang/generator/struct.go:115-142) from its loaded
// members m<i>: the members in declaration order (an inner struct is its own EncodeXxxTo in
// place), then EncodeStruct's rvarint(data size) | TypeStruct (tree_core.hpp emit_struct)
void gen_struct_emit(std::ostringstream &o, const TreeDesc &D, uint32_t sf, int d, const std::string &ind) {
    const TField &F = D.f[sf];
    o << ind << "{ const uint64_t ss" << d << " = em.pos;\n";
    for (uint32_t k = 0; k < F.nmem; k++) {
        const uint32_t mi = D.members[F.mem0 + k];
        const TField &M = D.f[mi];
        if (M.kind == spec::K_STRUCT) {
            gen_struct_emit(o, D, mi, d + 1, ind + "  ");
        } else {
            const bool heap = M.kind == spec::K_STRING || M.kind == spec::K_BYTES;
            o << ind << "  emit_value_k<" << (int)M.kind << ">(em, m" << mi << ", "
              << (heap ? "B.heaps[" + std::to_string(M.col) + "], B.heap_lens[" + std::to_string(M.col) + "]" : "nullptr, 0")
              << ");\n";
        }
    }
    o << ind << "  em.rvarint(em.pos - ss" << d << ");\n" << ind << "  em.put1(T_STRUCT);\n" << ind << "}\n";
}

// the size expression of a scalar value v (a loaded column element) of kind K (encode_core.hpp
// field_size rules)
std::string value_size_expr(int K, const std::string &v) {
    if (K == spec::K_BOOL) return "1";
    if (K == spec::K_BYTE) return "2";
    if (K == spec::K_INT16) return "(vlen32(zigzag32((int16_t)" + v + "[0])) + 1)";
    if (K == spec::K_INT32) return "(vlen32(zigzag32((int32_t)" + v + "[0])) + 1)";
    if (K == spec::K_INT64) return "(vlen64(zigzag64((int64_t)" + v + "[0])) + 1)";
    if (K == spec::K_UINT16 || K == spec::K_UINT32 || K == spec::K_UINT64) return "(vlen64(" + v + "[0]) + 1)";
    if (K == spec::K_FLOAT32) return "5";
    if (K == spec::K_FLOAT64 || K == spec::K_BIN64) return "9";
    if (K == spec::K_BIN128) return "17";
    if (K == spec::K_BIN256) return "33";
    const std::string len = "(uint64_t)(uint32_t)(" + v + "[0] >> 32)";
    if (K == spec::K_STRING) return "(" + len + " + vlen32((uint32_t)(" + v + "[0] >> 32)) + 2)";
    return "(" + len + " + vlen32((uint32_t)(" + v + "[0] >> 32)) + 1)"; // BYTES
}

// struct field sf's encoded size (tree_core.hpp struct_size) from its loaded members m<i>, into
// the variable `var` (declared here); a data size past MAX_SIZE sets err
void gen_struct_size(std::ostringstream &o, const TreeDesc &D, uint32_t sf, const std::string &var, const std::string &ind) {
    const TField &F = D.f[sf];
    o << ind << "uint64_t " << var << " = 0;\n" << ind << "{\n";
    for (uint32_t k = 0; k < F.nmem; k++) {
        const uint32_t mi = D.members[F.mem0 + k];
        const TField &M = D.f[mi];
        if (M.kind == spec::K_STRUCT) {
            gen_struct_size(o, D, mi, var + "_" + std::to_string(k), ind + "  ");
            o << ind << "  " << var << " += " << var << "_" << k << ";\n";
        } else {
            o << ind << "  " << var << " += " << value_size_expr(M.kind, "m" + std::to_string(mi)) << ";\n";
            if (M.kind == spec::K_STRING || M.kind == spec::K_BYTES)
                o << ind << "  { const uint32_t off = (uint32_t)m" << mi << "[0], len = (uint32_t)(m" << mi << "[0] >> 32);\n"
                  << ind << "    if ((uint64_t)len > MAX_SIZE || (uint64_t)off + len > B.heap_lens[" << M.col << "]) err = true; }\n";
        }
    }
    o << ind << "  if (" << var << " > MAX_SIZE) err = true;\n"
      << ind << "  " << var << " += vlen64(" << var << ") + 1;\n" << ind << "}\n";
}

// direct field k of table T in write order: its bytes through em (children: the gaps they fill,
// their rows' positions), then its end mark (e<k> or ends_[k] = em.pos - start), nf, bigtag
void gen_field_write(std::ostringstream &o, const TreeDesc &D, const TTable &T, uint32_t k, bool eager) {
    const uint32_t fi = D.direct[T.d0 + k];
    const TField &F = D.f[fi];
    auto load = [&](const char *ind) { gen_load(o, "a" + std::to_string(k), F.kind, F.col, "", ind); };
    // (an optional field: the whole block behind its presence test; a wide table's load sits inside)
    const std::string open = F.opt ? "  if (" + has_expr(D, T, k) + ") {\n" : "  {\n";
    const std::string ev = eager ? "e" + std::to_string(k) : "ends_[" + std::to_string(k) + "]";
    const std::string mark = "    " + ev + " = (uint32_t)(em.pos - start);\n    nf++;\n" +
                             (F.tag > 255 ? "    bigtag = true;\n" : "");
    if (eager) o << "  uint32_t e" << k << " = 0xffffffffu; // field " << fi << " tag " << F.tag << "\n";
    else o << "  ends_[" << k << "] = 0xffffffffu; // field " << fi << " tag " << F.tag << "\n";
    if (F.kind >= spec::K_BOOL && F.kind <= spec::K_BYTES) {
        const bool heap = F.kind == spec::K_STRING || F.kind == spec::K_BYTES;
        o << open;
        if (!eager) load("    ");
        o << "    emit_value_k<" << (int)F.kind << ">(em, a" << k << ", "
          << (heap ? "B.heaps[" + std::to_string(F.col) + "], B.heap_lens[" + std::to_string(F.col) + "]" : "nullptr, 0")
          << ");\n" << mark << "  }\n";
    } else if (F.kind == spec::K_ANY) {
        if (!eager) load("  ");
        o << "  if ((uint32_t)(a" << k << "[0] >> 32)) {\n    emit_value_k<" << (int)F.kind << ">(em, a" << k
          << ", B.heaps[" << F.col << "], B.heap_lens[" << F.col << "]);\n" << mark << "  }\n";
    } else if (F.kind == spec::K_STRUCT) {
        if (F.opt) {
            o << open;
            if (eager) gen_struct_emit(o, D, fi, 0, "    ");
            else o << "    emit_struct(em, B, D, " << fi << "u, row);\n";
            o << mark << "  }\n";
        } else {
            if (eager) gen_struct_emit(o, D, fi, 0, "  ");
            else o << "  emit_struct(em, B, D, " << fi << "u, row);\n";
            o << "  {\n" << mark << "  }\n";
        }
    } else if (F.kind == spec::K_MESSAGE) {
        o << "  if (pr" << k << ") {\n    B.pos[" << F.table << "][row] = em.pos;\n    em.skip(sz" << k << ");\n" << mark
          << "  } else {\n    B.pos[" << F.table << "][row] = ~0ull; // absent: its row is not written\n  }\n";
    } else if (F.kind == spec::K_LIST) {
        const int y = F.table;
        o << "  if (!pr" << k << ") { // absent: rows in its range (if any) are not written\n"
          << "    for (uint32_t j = j0_" << k << "; j < j1_" << k << "; j++) B.pos[" << y << "][j] = ~0ull;\n  }\n";
        o << "  if (pr" << k << ") {\n"
          << "    emit_list(em, B, " << y << "u, j0_" << k << ", j1_" << k << ");\n"
          << mark << "  }\n";
    }
}

// The generated Write() of a message table (internal/lang/generator/message.go:319-439,
// internal/writer/writer.go:376-553) for one row at start: every column read issued before the
// first byte is written, then the fields in write order (constant kinds, heaps and tags), the
// table in the Writer's tie-sorted order over the present fields, the trailer.  Sub-messages and
// list elements are children written by their tables' later launches into the gaps skipped here.
void gen_write_table(std::ostringstream &o, const TreeDesc &D, uint32_t t) {
    const TTable &T = D.t[t];
    // a table of more than 64 direct fields loads each value where it is written (all of them in
    // flight at once would hold ~4 registers per field), and its writer is a function of its own:
    // inlined into the level-fused kernel, hiprtc spent minutes allocating registers over it
    const bool eager = T.nd <= 64;
    // (and out of line in a tree of many tables too: 114 writers inlined into the one level-fused
    // kernel took hiprtc 13 minutes)
    const bool inl = eager && D.ntables <= 32;
    o << "template <class E>\n__device__ " << (inl ? "__forceinline__" : "__noinline__") << " void gen_wrow_" << t
      << "(E &em, const TreeDesc &D, const TreeBufs &B, uint64_t row, uint64_t start) {\n";
    gen_has_word(o, T, "  ");
    for (uint32_t k = 0; k < T.nd; k++) gen_field_loads(o, D, T, k, eager, "  ");
    o << "  uint32_t nf = 0;\n  bool bigtag = false;\n";
    // field ends: registers (e<k>), or for a wide table an array the table loop reads at run time
    if (!eager) o << "  uint32_t ends_[" << T.nd << "];\n";
    for (uint32_t k = 0; k < T.nd; k++) gen_field_write(o, D, T, k, eager);
    // IsBigMessage (internal/format/msg.go:43-61), the table (encode/msg.go:58-72), the trailer
    o << "  const uint64_t data = em.pos - start;\n"
      << "  const bool big = bigtag || (nf > 0 && data > 65535);\n";
    if (!eager) {
        // the wide table's entries in a run-time loop over the Writer's order (tree.hip layout:
        // sorted[], sslot[]): a third of the unrolled code
        o << "  for (uint32_t j = 0; j < " << T.nd << "u; j++) {\n"
          << "    const uint32_t e = ends_[D.sslot[" << T.d0 << "u + j]];\n"
          << "    if (e == 0xffffffffu) continue;\n"
          << "    const uint32_t tag = D.f[D.sorted[" << T.d0 << "u + j]].tag;\n"
          << "    if (!big) em.put_n(tag | ((uint64_t)__builtin_bswap16((uint16_t)e) << 8), 3);\n"
          << "    else { em.be(tag, 2); em.be(e, 4); }\n  }\n"
          << "  em.rvarint(data);\n  em.rvarint((uint64_t)nf * (big ? 6 : 3));\n"
          << "  em.put1(big ? T_BIG_MESSAGE : T_MESSAGE);\n  em.finish();\n}\n";
    } else {
        gen_table_trailer(o, D, T);
        o << "}\n";
    }
    // a row no owner placed (its own owner absent or unplaced): its children are not written either
    o << "__device__ __forceinline__ void gen_unplace_" << t << "(const TreeDesc &D, const TreeBufs &B, uint64_t row) {\n";
    for (uint32_t k = 0; k < T.nd; k++) {
        const TField &F = D.f[D.direct[T.d0 + k]];
        if (F.kind == spec::K_MESSAGE) {
            o << "  B.pos[" << F.table << "][row] = ~0ull;\n";
        } else if (F.kind == spec::K_LIST) {
            o << "  { bool lerr = false; uint32_t j0, j1; list_span(B, D, " << F.table << "u, row, j0, j1, lerr);\n"
              << "    for (uint32_t j = j0; j < j1; j++) B.pos[" << F.table << "][j] = ~0ull; }\n";
        }
    }
    o << "}\n";
}

bool tree_tile(const TreeDesc &D);
void tile_cuts(const TreeDesc &D, uint32_t *cut);

// The generated writer's size pass for a message table (tree.hip tree_size_kernel with constant
// kinds, columns and tags): every column read first, then the encoded sizes, IsBigMessage.
void gen_size_table(std::ostringstream &o, const TreeDesc &D, uint32_t t) {
    const TTable &T = D.t[t];
    o << "__device__ __forceinline__ void gen_srow_" << t
      << "(const TreeDesc &D, const TreeBufs &B, uint32_t x, uint64_t row, bool &err) {\n"
      << "  {\n";
    // (a table of more than 64 fields reads its HASMASK words per optional field: has_expr)
    gen_has_word(o, T, "    ");
    for (uint32_t k = 0; k < T.nd; k++) {
        const TField &F = D.f[D.direct[T.d0 + k]];
        if ((F.kind >= spec::K_BOOL && F.kind <= spec::K_BYTES) || F.kind == spec::K_ANY)
            gen_load(o, "a" + std::to_string(k), F.kind, F.col, F.opt ? has_expr(D, T, k) : std::string(), "    ");
        else if (F.kind == spec::K_MESSAGE || F.kind == spec::K_LIST)
            o << "    const uint32_t pr" << k << " = ((const uint8_t *)" << col_expr(F.present) << ")[row];\n";
        if (F.kind == spec::K_STRUCT) gen_field_loads(o, D, T, k, true, "    ");
        if (F.kind == spec::K_LIST)
            o << "    const uint32_t j0_" << k << " = ((const uint32_t *)" << col_expr(D.t[F.table].begin_col) << ")[row], j1_" << k
              << " = ((const uint32_t *)" << col_expr(D.t[F.table].begin_col) << ")[row + 1];\n";
    }
    // the records' table under the record-tile writer (gen_tile): also each field block's end
    // offset (B.tblk, inclusive prefix over the blocks) and the present direct fields (B.tmask)
    const bool tile = t == 0 && tree_tile(D);
    uint32_t cut[spec::TREE_TILE_W + 1];
    if (tile) tile_cuts(D, cut);
    o << "    uint64_t data = 0;\n    uint32_t nf = 0;\n    bool bigtag = false;\n"
      << (tile ? "    uint64_t bm = 0;\n" : "");
    for (uint32_t k = 0; k < T.nd; k++) {
        const uint32_t fi = D.direct[T.d0 + k];
        const TField &F = D.f[fi];
        const std::string tg = (F.tag > 255 ? " bigtag = true;" : "") +
                               (tile ? " bm |= 1ull << " + std::to_string(k) + ";" : std::string());
        for (int bl = 0; tile && bl < spec::TREE_TILE_W; bl++) // blocks ending before field k
            if (cut[bl + 1] == k) o << "    const uint64_t tb" << bl << " = data;\n";
        if (F.opt) o << "    if (" << has_expr(D, T, k) << ") { // optional: sized when present\n";
        switch (F.kind) {
        case spec::K_MESSAGE:
            o << "    if (pr" << k << ") { data += B.size[" << F.table << "][row]; nf++;" << tg << " }\n";
            break;
        case spec::K_LIST:
            o << "    if (pr" << k << ") { data += list_total(B, " << F.table << "u, j0_" << k << ", j1_" << k << ", err); nf++;" << tg
              << " }\n";
            break;
        case spec::K_STRUCT:
            gen_struct_size(o, D, fi, "st" + std::to_string(k), "    ");
            o << "    data += st" << k << "; nf++;" << tg << "\n";
            break;
        case spec::K_ANY:
            o << "    { const uint32_t off = (uint32_t)a" << k << "[0], len = (uint32_t)(a" << k << "[0] >> 32);\n"
              << "      if ((uint64_t)len > MAX_SIZE || (uint64_t)off + len > B.heap_lens[" << F.col << "]) err = true;\n"
              << "      if (len) { data += len; nf++;" << tg << " } }\n";
            break;
        case spec::K_STRING:
        case spec::K_BYTES:
            o << "    { const uint32_t off = (uint32_t)a" << k << "[0], len = (uint32_t)(a" << k << "[0] >> 32);\n"
              << "      if ((uint64_t)len > MAX_SIZE || (uint64_t)off + len > B.heap_lens[" << F.col << "]) err = true;\n"
              << "      data += (uint64_t)len + vlen32(len) + " << (F.kind == spec::K_STRING ? 2 : 1) << "; nf++;" << tg << " }\n";
            break;
        default: {
            const int K = F.kind;
            std::string sz;
            if (K == spec::K_BOOL) sz = "1";
            else if (K == spec::K_BYTE) sz = "2";
            else if (K == spec::K_INT16) sz = "vlen32(zigzag32((int16_t)a" + std::to_string(k) + "[0])) + 1";
            else if (K == spec::K_INT32) sz = "vlen32(zigzag32((int32_t)a" + std::to_string(k) + "[0])) + 1";
            else if (K == spec::K_INT64) sz = "vlen64(zigzag64((int64_t)a" + std::to_string(k) + "[0])) + 1";
            else if (K == spec::K_UINT16 || K == spec::K_UINT32 || K == spec::K_UINT64)
                sz = "vlen64(a" + std::to_string(k) + "[0]) + 1";
            else if (K == spec::K_FLOAT32) sz = "5";
            else if (K == spec::K_FLOAT64 || K == spec::K_BIN64) sz = "9";
            else if (K == spec::K_BIN128) sz = "17";
            else sz = "33";
            o << "    data += " << sz << "; nf++;" << tg << "\n";
        }
        }
        if (F.opt) o << "    }\n";
    }
    if (tile) {
        for (int bl = 0; bl < spec::TREE_TILE_W; bl++)
            if (cut[bl + 1] == T.nd) o << "    const uint64_t tb" << bl << " = data;\n";
        for (int bl = 0; bl < spec::TREE_TILE_W; bl++) o << "    B.tblk[row * " << spec::TREE_TILE_W << " + " << bl << "] = (uint32_t)tb" << bl << ";\n";
        o << "    B.tmask[row] = bm;\n";
    }
    // IsBigMessage (internal/format/msg.go:43-61), encodeMessageTable sizes
    o << "    const bool big = bigtag || (nf > 0 && data > 65535);\n"
      << "    const uint64_t tsize = (uint64_t)nf * (big ? 6 : 3);\n"
      << "    if (data > MAX_SIZE) err = true;\n"
      << "    const uint64_t total = data + tsize + vlen64(data) + vlen64(tsize) + 1;\n"
      << "    if (total > 0xffffffffull) err = true;\n"
      << "    B.size[x][row] = (uint32_t)total;\n"
      << "  }\n}\n";
}

// The sub-message tables of group root x after its root table's code, each over the range its
// owner field left in its slot; a sub-table whose trailer is invalid sets its owner field's *Err
// bit (the owner's getter would have failed on the same trailer): on a wave group's root through
// ro (pair), else into the owner's ERRMASK column, which the owner's code stored before.
void gen_sub_tables(std::ostringstream &o, const TreeDesc &D, uint32_t x, int pair_w, const uint32_t *tw,
                    const std::string &fb) {
    const TTable &T = D.t[x];
    for (uint32_t g = 1; g < T.gn; g++) {
        const uint32_t y = D.group[T.g0 + g];
        if (pair_w >= 0 && tw[y] != (uint32_t)pair_w) continue;
        const TTable &Y = D.t[y], &Pt = D.t[Y.parent];
        std::string bad;
        uint32_t k = 0;
        while (k < Pt.nd && D.direct[Pt.d0 + k] != Y.field) k++;
        if (Pt.err_col >= 0 && k < 64) {
            const std::string bit = "(1ull << " + std::to_string(k) + ")";
            bad = pair_w >= 0 && Y.parent == x ? "ro.errs |= " + bit + ";"
                                               : "((uint64_t *)" + col_expr(Pt.err_col) + ")[row] |= " + bit + ";";
        }
        const std::string r = "gr[" + std::to_string(Y.gslot) + " * 64]";
        gen_message_table(o, D, y, "(long long)" + r + ".x", "(long long)" + r + ".y", false, nullptr, fb, bad);
    }
}

// ---- the root group on a wave pair (tree_decode_core.hpp tree_rows_pair) ----
// A cost per field, about its LDS reads and VALU: the pair split balances these.
uint32_t tree_table_cost(const TreeDesc &D, uint32_t t);
uint32_t tree_field_cost(const TreeDesc &D, uint32_t fi) {
    const TField &F = D.f[fi];
    switch (F.kind) {
    case spec::K_STRING: case spec::K_BYTES: case spec::K_BIN128: case spec::K_BIN256: return 3;
    case spec::K_STRUCT: return 2 + 2 * (F.send - fi - 1);
    case spec::K_ANY: return 5;
    case spec::K_LIST: return 5;
    case spec::K_MESSAGE: return 3 + tree_table_cost(D, F.table);
    default: return 2;
    }
}
uint32_t tree_table_cost(const TreeDesc &D, uint32_t t) {
    const TTable &T = D.t[t];
    uint32_t c = 4;
    for (uint32_t k = 0; k < T.nd; k++) c += tree_field_cost(D, D.direct[T.d0 + k]);
    return c;
}

// Group root x split over P waves: sel[w][k] = wave w decodes root field k (with the sub-message
// tables below it, which need the range it finds).  Heaviest first, each to the least loaded
// wave.  false when the root has too few fields to split.
bool pair_split(const TreeDesc &D, uint32_t x, int P, std::vector<char> *sel, uint32_t *table_wave) {
    const TTable &T = D.t[x];
    if (T.shape != spec::SHAPE_MESSAGE || T.nd < (uint32_t)(2 * P)) return false;
    std::vector<uint32_t> ks(T.nd);
    for (uint32_t k = 0; k < T.nd; k++) ks[k] = k;
    std::stable_sort(ks.begin(), ks.end(), [&](uint32_t a, uint32_t b) {
        return tree_field_cost(D, D.direct[T.d0 + a]) > tree_field_cost(D, D.direct[T.d0 + b]);
    });
    uint32_t load[4] = {0, 0, 0, 0};
    for (int w = 0; w < P; w++) sel[w].assign(T.nd, 0);
    for (uint32_t k : ks) {
        int w = 0;
        for (int v = 1; v < P; v++)
            if (load[v] < load[w]) w = v;
        sel[w][k] = 1;
        load[w] += tree_field_cost(D, D.direct[T.d0 + k]);
    }
    for (uint32_t g = 1; g < T.gn; g++) {
        const uint32_t y = D.group[T.g0 + g];
        uint32_t a = y;
        while (D.t[a].parent != x) a = D.t[a].parent;
        table_wave[y] = 0;
        for (uint32_t k = 0; k < T.nd; k++)
            if (D.direct[T.d0 + k] == D.t[a].field)
                for (int w = 0; w < P; w++)
                    if (sel[w][k]) table_wave[y] = (uint32_t)w;
    }
    return true;
}

// spec_tree_group_<x>p<P>: the group's row code split over P waves (pair_split).  The waves
// share one set of range slots: a sub-message table's slot is written and read by the wave that
// owns it (a row on the run-time path has every wave write every slot, with the same values).
void gen_pair_rows(std::ostringstream &o, const TreeDesc &D, uint32_t x, int P) {
    std::vector<char> sel[4];
    uint32_t tw[spec::TREE_MAX_T] = {};
    if (!pair_split(D, x, P, sel, tw)) return;
    const TTable &T = D.t[x];
    const std::string fn = "gen_pair_" + std::to_string(x) + "_" + std::to_string(P) + "_w";
    for (int w = 0; w < P; w++) {
        o << "template <class Src>\n__device__ __forceinline__ void " << fn << w
          << "(const Src &s, const TreeDesc &D, const TreeBufs &B, uint64_t row, long long lo, long long hi, uint2 *gr, "
             "RowOut &ro) {\n";
        const std::string fb = "tree_message_fallback_p<" + std::to_string(P) + ">";
        gen_message_table(o, D, x, "lo", "hi", true, &sel[w], fb);
        gen_sub_tables(o, D, x, w, tw, fb);
        o << "}\n";
    }
    std::ostringstream call;
    call << "      switch (threadIdx.x >> 6) {\n";
    for (int w = 0; w < P; w++)
        call << "      case " << w << ": " << fn << w << "(s, D, B, row, lo, hi, gr, ro); break;\n";
    call << "      default: break;\n      }\n";
    // P waves of one block per SIMD... and as many blocks per CU as the LDS holds (four for
    // pkg1): registers for 8 / 4 waves per SIMD-pair budget -> at most 512 / P VGPRs
    o << "extern \"C\" __global__ __launch_bounds__(" << 64 * P << ") __attribute__((amdgpu_waves_per_eu(" << P
      << "))) void spec_tree_group_" << x << "p" << P
      << "(const TreeDesc *Dp, const TreeBufs *Bp, uint32_t x, uint32_t slab, uint32_t slots, uint32_t rpw) {\n"
      << "  const TreeDesc &D = *Dp;\n"
      << "  const TreeBufs &B = *Bp;\n"
      << "  const uint64_t rows = dec_rows(D, B, x);\n"
      << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
      << "  uint2 *gr = (uint2 *)(smem + slab) + (threadIdx.x & 63);\n"
      << "  uint4 *xch = (uint4 *)(smem + slab + slots);\n"
      << "  (void)rpw;\n"
      << "  tree_rows_pair<" << P << (T.has_col >= 0 ? ", true" : "") << ">(B, x, rows, slab, xch,\n"
      << "    [&](const TreeLds &s, uint64_t row, long long lo, long long hi, RowOut &ro) {\n"
      << call.str() << "    },\n"
      << "    [&](const GlobalSrc &s, uint64_t row, long long lo, long long hi, RowOut &ro) {\n"
      << call.str() << "    },\n"
      << "    [&](uint64_t row, bool panic, const RowOut &a, const RowOut &b) {\n"
      << "      uint64_t *errp = " << (T.err_col >= 0 ? "(uint64_t *)" + col_expr(T.err_col) : std::string("nullptr")) << ";\n"
      << "      if (a.fast && errp) errp[row] = a.errs | b.errs;\n"
      << (T.has_col >= 0 ? "      if (a.fast && " + col_expr(T.has_col) + ") ((uint64_t *)" + col_expr(T.has_col) +
                               ")[row] = a.has | b.has;\n"
                         : std::string())
      << "      const uint32_t st = a.st == ST_PANIC || b.st == ST_PANIC ? (uint32_t)ST_PANIC : a.st;\n"
      << "      store_u8(" << col_expr(T.status_col) << ", row, panic ? (uint32_t)ST_PANIC : st);\n"
      << "    });\n"
      << "}\n";
}

// ---- the record-tile writer (tree_core.hpp MkL, tile_copy_out) ----
// spec_tree_write_tile: one workgroup of TILE_W waves per 64 consecutive records.  Depth 0: the
// records' direct fields are split into TILE_W contiguous blocks, wave w writing block w of all
// 64 records (so a wave runs one block's code, no divergence) at the block's offset, which the
// size pass left per record with the record's present fields (B.tblk, B.tmask), and their table
// entries at (popcount of the present fields before them in the Writer's order); the last wave
// writes the trailer.  Depth d > 0: the tile's rows of every table at depth d (a
// contiguous row range per table, from the records' range through BEGIN columns) over all lanes,
// through the tables' generated writers.  A barrier between depths (children placed by their
// owners).  Everything goes to an LDS image of the tile's output range, stored once with 16-byte
// stores; the bytes of a range longer than the image past its first cap bytes are stored straight
// to HBM (a loop of passes over windows of the range tripled the kernel's compile time).
constexpr int TILE_W = spec::TREE_TILE_W;

bool tree_tile(const TreeDesc &D) {
    if (D.ntables > 32 || D.t[0].shape != spec::SHAPE_MESSAGE) return false;
    for (uint32_t t = 0; t < D.ntables; t++)
        if (D.t[t].shape == spec::SHAPE_MESSAGE && D.t[t].nd > 64) return false;
    return true;
}

// a records' field's share of its wave's time in the tile writer, in scalar fields (fitted to
// per-wave clocks measured on pkg1: a list ≈ 5, a string ≈ 2)
uint32_t tile_field_cost(const TreeDesc &D, const TField &F) {
    switch (F.kind) {
    case spec::K_STRING: case spec::K_BYTES: case spec::K_ANY: return 2;
    case spec::K_BIN128: return 2;
    case spec::K_BIN256: return 3;
    case spec::K_STRUCT: return 1 + (F.send - 1u - (uint32_t)(&F - D.f));
    case spec::K_LIST: return 5;
    case spec::K_MESSAGE: return 1;
    default: return 1;
    }
}

// the records' direct fields in TILE_W contiguous blocks of about equal cost: block b is
// [cut[b], cut[b + 1])
void tile_cuts(const TreeDesc &D, uint32_t *cut) {
    const TTable &T = D.t[0];
    std::vector<uint32_t> cost(T.nd);
    uint32_t total = 0;
    for (uint32_t k = 0; k < T.nd; k++) total += cost[k] = tile_field_cost(D, D.f[D.direct[T.d0 + k]]);
    uint32_t k = 0, acc = 0;
    cut[0] = 0;
    for (int b = 0; b < TILE_W; b++) {
        // fields while below the block's share of the total, the last one only if that lands closer
        const int64_t target = (int64_t)total * (b + 1) / TILE_W;
        while (k < T.nd && (b == TILE_W - 1 || ((int64_t)acc < target &&
                                                 (int64_t)(acc + cost[k]) - target <= target - (int64_t)acc)))
            acc += cost[k++];
        cut[b + 1] = k;
    }
    cut[TILE_W] = T.nd;
}

void gen_tile(std::ostringstream &o, const TreeDesc &D) {
    const TTable &T = D.t[0];
    uint32_t cut[TILE_W + 1];
    tile_cuts(D, cut);
    // PRE[k]: the direct fields before k in the Writer's table order; BIGM: tags past 255
    std::vector<uint64_t> pre(T.nd, 0);
    uint64_t bigm = 0, seen = 0;
    for (uint32_t j = 0; j < T.nd; j++) {
        const uint32_t slot = D.sslot[T.d0 + j];
        pre[slot] = seen;
        seen |= 1ull << slot;
    }
    for (uint32_t k = 0; k < T.nd; k++)
        if (D.f[D.direct[T.d0 + k]].tag > 255) bigm |= 1ull << k;
    // block b of a record: its offset and the record's data size and present fields from the size
    // pass (gen_size_table: B.tblk, B.tmask), so the waves need not meet before writing
    for (int b = 0; b < TILE_W; b++) {
        o << "template <class Mk>\n__device__ __forceinline__ void gen_troot_" << b
          << "(const Mk &mk, const TreeDesc &D, const TreeBufs &B, uint64_t row) {\n"
          << "  const uint64_t start = B.offsets[row];\n"
          << "  const uint64_t off = " << (b ? "B.tblk[row * " + std::to_string(TILE_W) + " + " + std::to_string(b - 1) + "]" : "0")
          << ", data = B.tblk[row * " << TILE_W << " + " << TILE_W - 1 << "];\n"
          << "  const uint64_t m = B.tmask[row];\n";
        gen_has_word(o, T, "  ");
        for (uint32_t k = cut[b]; k < cut[b + 1]; k++) gen_field_loads(o, D, T, k, true, "  ");
        if (b == 0) o << "  if (B.ends_out) B.ends_out[row] = start + B.size[0][row];\n";
        o << "  const bool big = (m & 0x" << std::hex << bigm << std::dec << "ull) != 0 || (m != 0 && data > 65535);\n"
          // (block 0 of a framed record starts with its head, B.frame_head bytes below the message)
          << (b ? "  auto em = mk(start + off);\n"
                : "  const uint32_t fh = B.frame_head;\n  auto em = mk(start - fh);\n"
                  "  if (fh) em.be(B.size[0][row], 4);\n")
          << "  uint32_t nf = 0;\n  bool bigtag = false;\n";
        for (uint32_t k = cut[b]; k < cut[b + 1]; k++) gen_field_write(o, D, T, k, true);
        o << "  em.finish();\n  const uint64_t tb = start + data;\n";
        for (uint32_t k = cut[b]; k < cut[b + 1]; k++) {
            const uint32_t tag = D.f[D.direct[T.d0 + k]].tag;
            o << "  if (e" << k << " != 0xffffffffu) {\n"
              << "    const uint64_t p = tb + (big ? 6u : 3u) * (uint32_t)__popcll(m & 0x" << std::hex << pre[k] << std::dec
              << "ull);\n"
              << "    if (!big) em.put_at(p, " << (tag & 0xff) << "u | ((uint64_t)__builtin_bswap16((uint16_t)e" << k
              << ") << 8), 3);\n"
              << "    else em.put_at(p, " << (((tag & 0xff) << 8) | (tag >> 8)) << "u | ((uint64_t)__builtin_bswap32(e" << k
              << ") << 16), 6);\n  }\n";
        }
        if (b == TILE_W - 1)
            o << "  { const uint32_t nt = (uint32_t)__popcll(m) * (big ? 6u : 3u);\n"
              << "    auto tr = mk(tb + nt);\n    tr.rvarint(data);\n    tr.rvarint(nt);\n"
              << "    tr.put1(big ? T_BIG_MESSAGE : T_MESSAGE);\n    tr.finish(); }\n";
        o << "  (void)nf; (void)bigtag;\n}\n";
    }
    // the rows of tables 1.. at their placed positions: a message row's column reads and its
    // position issued together (one round trip), the position checked after them
    for (uint32_t x = 1; x < D.ntables; x++) {
        const TTable &X = D.t[x];
        o << "template <class Mk>\n__device__ __forceinline__ void gen_trow_" << x
          << "(const Mk &mk, const TreeDesc &D, const TreeBufs &B, uint64_t row) {\n";
        if (X.shape == spec::SHAPE_MESSAGE) {
            // (the row's HASMASK word and the loads behind it are issued with the position, before the
            // unplaced-row test: in bounds, bind_columns requires the column wherever the table has
            // rows; the mask of a row no owner placed is read and ignored)
            gen_has_word(o, X, "  ");
            for (uint32_t k = 0; k < X.nd; k++) gen_field_loads(o, D, X, k, true, "  ");
            o << "  const uint64_t start = B.pos[" << x << "][row];\n"
              << "  if (start == ~0ull) { gen_unplace_" << x << "(D, B, row); return; }\n"
              << "  auto em = mk(start);\n  uint32_t nf = 0;\n  bool bigtag = false;\n";
            for (uint32_t k = 0; k < X.nd; k++) gen_field_write(o, D, X, k, true);
            o << "  const uint64_t data = em.pos - start;\n"
              << "  const bool big = bigtag || (nf > 0 && data > 65535);\n";
            gen_table_trailer(o, D, X);
        } else if (X.shape == spec::SHAPE_VALUE && D.f[X.field].elem >= spec::K_BOOL && D.f[X.field].elem <= spec::K_BYTES) {
            const TField &F = D.f[X.field];
            const bool heap = F.elem == spec::K_STRING || F.elem == spec::K_BYTES;
            o << "  uint64_t a[4];\n  load_value_k<" << (int)F.elem << ">(" << col_expr(F.col) << ", row, a);\n"
              << "  const uint64_t start = B.pos[" << x << "][row];\n  if (start == ~0ull) return;\n"
              << "  auto em = mk(start);\n  emit_value_k<" << (int)F.elem << ">(em, a, "
              << (heap ? "B.heaps[" + std::to_string(F.col) + "], B.heap_lens[" + std::to_string(F.col) + "]" : "nullptr, 0")
              << ");\n  em.finish();\n";
        } else if (X.shape == spec::SHAPE_STRUCT) { // a list of structs: the element's EncodeXxxTo
            const TField &F = D.f[X.field];
            for (uint32_t i = X.field + 1u; i < F.send; i++)
                if (D.f[i].kind != spec::K_STRUCT)
                    o << "  uint64_t m" << i << "[4];\n  load_value_k<" << (int)D.f[i].kind << ">(" << col_expr(D.f[i].col)
                      << ", row, m" << i << ");\n";
            o << "  const uint64_t start = B.pos[" << x << "][row];\n  if (start == ~0ull) return;\n"
              << "  auto em = mk(start);\n";
            gen_struct_emit(o, D, X.field, 0, "  ");
            o << "  em.finish();\n";
        } else {
            o << "  const uint64_t start = B.pos[" << x << "][row];\n  if (start == ~0ull) return;\n"
              << "  auto em = mk(start);\n  emit_row_shaped(em, D, B, " << x << "u, row);\n";
        }
        o << "}\n";
    }
    int depth[spec::TREE_MAX_T] = {0}, maxd = 0;
    for (uint32_t x = 1; x < D.ntables; x++) {
        depth[x] = depth[D.t[x].parent] + 1;
        maxd = std::max(maxd, depth[x]);
    }
    o << "template <class Mk>\n__device__ __forceinline__ void gen_tile_body(const Mk &mk, const TreeDesc &D, const TreeBufs &B, "
         "uint64_t r0, uint64_t r1) {\n"
      << "  const uint64_t row = r0 + (threadIdx.x & 63);\n"
      << "  if (row < r1) switch (threadIdx.x >> 6) {\n";
    for (int b = 0; b < TILE_W; b++) o << "  case " << b << ": gen_troot_" << b << "(mk, D, B, row); break;\n";
    o << "  }\n  __syncthreads();\n  const uint64_t lo0 = r0, hi0 = r1;\n";
    for (uint32_t x = 1; x < D.ntables; x++) {
        const TTable &X = D.t[x];
        // (an owner range that is empty reads no BEGIN: the column may be absent then)
        if (X.rel == spec::REL_MANY)
            o << "  const bool ne" << x << " = hi" << X.parent << " > lo" << X.parent << ";\n"
              << "  const uint64_t lo" << x << " = ne" << x << " ? ((const uint32_t *)" << col_expr(X.begin_col) << ")[lo"
              << X.parent << "] : 0, hi" << x << " = ne" << x << " ? ((const uint32_t *)" << col_expr(X.begin_col) << ")[hi"
              << X.parent << "] : 0;\n";
        else
            o << "  const uint64_t lo" << x << " = lo" << X.parent << ", hi" << x << " = hi" << X.parent << ";\n";
    }
    // depth d: the tables' row ranges laid end to end, index i to thread i mod blockDim, one
    // loop per table over this thread's indices in its segment (an if-chain over the tables
    // inside one loop took the register coalescer minutes)
    for (int d = 1; d <= maxd; d++) {
        o << "  { // depth " << d << "\n    uint64_t base = 0;\n";
        for (uint32_t x = 1; x < D.ntables; x++)
            if (depth[x] == d)
                o << "    const uint64_t c" << x << " = hi" << x << " - lo" << x << ", b" << x << " = base;\n    base += c" << x << ";\n"
                  << "    for (uint64_t i = (uint32_t)(threadIdx.x - b" << x << ") % blockDim.x; i < c" << x
                  << "; i += blockDim.x)\n      gen_trow_" << x << "(mk, D, B, lo" << x << " + i);\n";
        o << "    (void)base;\n  }\n  __syncthreads();\n";
    }
    o << "}\n"
      << "extern \"C\" __global__ __launch_bounds__(" << TILE_W * 64
      << ") __attribute__((amdgpu_waves_per_eu(" << spec::TREE_TILE_WPE
      << "))) void spec_tree_write_tile(const TreeDesc *Dp, const TreeBufs *Bp, "
         "uint32_t cap) {\n"
      << "  const TreeDesc &D = *Dp;\n  const TreeBufs &B = *Bp;\n"
      << "  if (!B.out || *B.err || *B.total > B.out_cap) return;\n"
      << "  const uint64_t n = B.rows[0], r0 = (uint64_t)blockIdx.x * 64;\n  if (r0 >= n) return;\n"
      << "  const uint64_t r1 = r0 + 64 < n ? r0 + 64 : n;\n"
      << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
      << "  TileU8 *img = (TileU8 *)smem;\n"
      // (the image starts at the first record's frame head, B.frame_head bytes below its message)
      << "  const uint64_t org = B.offsets[r0] - B.frame_head, fin = B.offsets[r1 - 1] + B.size[0][r1 - 1];\n"
      // (out + sh 16-byte aligned: the image's chunks are the output's)
      << "  const uint64_t sh = org - (((unsigned long long)B.out + org) & 15);\n"
      // (the image starts zeroed: the rows OR their dwords into it, tree_core.hpp LSink::word)
      << "  tile_clear(img, fin - sh < cap ? (uint32_t)(fin - sh) : cap);\n  __syncthreads();\n"
      << "  gen_tile_body(MkL{img, B.out, sh, cap}, D, B, r0, r1);\n"
      << "  tile_copy_out(B.out, img, sh, org, fin < sh + cap ? fin : sh + cap);\n"
      << "}\n";
}

std::string generate_tree(const TreeDesc &D, bool *has) {
    std::ostringstream o;
    o << "#include \"tree_decode_core.hpp\"\nusing namespace spec;\n";
    for (uint32_t t = 0; t < D.ntables; t++)
        if (D.t[t].shape == spec::SHAPE_MESSAGE) {
            gen_write_table(o, D, t);
            gen_size_table(o, D, t);
        }
    // level-fused launches (tree_core.hpp TableSet): blockIdx.y = the set's table
    o << "extern \"C\" __global__ __launch_bounds__(256) void spec_tree_size_set(const TreeDesc *Dp, const TreeBufs *Bp, "
         "TableSet s) {\n"
      << "  const TreeDesc &D = *Dp;\n  const TreeBufs &B = *Bp;\n  bool err = false;\n"
      << "  const uint32_t x = s.t[blockIdx.y];\n  const uint64_t rows = B.rows[x];\n"
      << "  switch (x) {\n";
    for (uint32_t t = 0; t < D.ntables; t++) {
        const TTable &X = D.t[t];
        if (X.shape == spec::SHAPE_MESSAGE) {
            o << "  case " << t << ": for (uint64_t row = grid_first(); row < rows; row += grid_stride()) gen_srow_" << t
              << "(D, B, x, row, err); break;\n";
            continue;
        }
        // list elements: scalars, strings, bytes and structs with constant kinds (value_size /
        // struct_size's rules); other elements (any) by the run-time rule below
        const TField &F = D.f[X.field];
        const bool val = X.shape == spec::SHAPE_VALUE && F.elem >= spec::K_BOOL && F.elem <= spec::K_BYTES;
        if (!val && X.shape != spec::SHAPE_STRUCT) continue;
        o << "  case " << t << ":\n    for (uint64_t row = grid_first(); row < rows; row += grid_stride()) {\n";
        if (val) {
            o << "      uint64_t a[4];\n      load_value_k<" << (int)F.elem << ">(" << col_expr(F.col) << ", row, a);\n"
              << "      const uint64_t total = " << value_size_expr(F.elem, "a") << ";\n";
            if (F.elem == spec::K_STRING || F.elem == spec::K_BYTES)
                o << "      { const uint32_t off = (uint32_t)a[0], len = (uint32_t)(a[0] >> 32);\n"
                  << "        if ((uint64_t)len > MAX_SIZE || (uint64_t)off + len > B.heap_lens[" << F.col << "]) err = true; }\n";
        } else {
            for (uint32_t i = X.field + 1u; i < F.send; i++)
                if (D.f[i].kind != spec::K_STRUCT)
                    o << "      uint64_t m" << i << "[4];\n      load_value_k<" << (int)D.f[i].kind << ">(" << col_expr(D.f[i].col)
                      << ", row, m" << i << ");\n";
            gen_struct_size(o, D, X.field, "total", "      ");
        }
        o << "      if (total > 0xffffffffull) err = true;\n      B.size[x][row] = (uint32_t)total;\n    }\n    break;\n";
    }
    o << "  default:\n"
      << "    for (uint64_t row = grid_first(); row < rows; row += grid_stride()) {\n"
      << "      const uint64_t total = size_row_shaped(D, B, x, row, err);\n"
      << "      if (total > 0xffffffffull) err = true;\n"
      << "      B.size[x][row] = (uint32_t)total;\n"
      << "    }\n  }\n  if (err) *B.err = 1;\n}\n";
    // the level-fused writer: where the record-tile writer does not apply
    if (!tree_tile(D)) {
        o << "extern \"C\" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void spec_tree_write_set("
             "const TreeDesc *Dp, const TreeBufs *Bp, TableSet s) {\n"
          << "  const TreeDesc &D = *Dp;\n  const TreeBufs &B = *Bp;\n"
          << "  if (!B.out || *B.err || *B.total > B.out_cap) return;\n"
          << "  const uint32_t x = s.t[blockIdx.y];\n  const uint64_t rows = B.rows[x];\n"
          << "  switch (x) {\n";
        for (uint32_t t = 0; t < D.ntables; t++)
            if (D.t[t].shape == spec::SHAPE_MESSAGE)
                o << "  case " << t << ":\n"
                  << "    for (uint64_t row = grid_first(); row < rows; row += grid_stride()) {\n"
                  // a row outside its owners' BEGIN ranges is not written, and neither is anything
                  // under it: its children's positions are marked unplaced (they may hold stale
                  // workspace bytes otherwise, and the next depth's writer would emit at them)
                  << (D.t[t].rel == spec::REL_MANY
                          ? "      if (!list_row_covered(D, B, x, row)) { gen_unplace_" + std::to_string(t) +
                                "(D, B, row); continue; }\n"
                          : std::string())
                  << "      const uint64_t start = x == 0 ? B.offsets[row] : B.pos[x][row];\n"
                  << "      if (start == ~0ull) { gen_unplace_" << t << "(D, B, row); continue; }\n"
                  << "      if (x == 0 && B.ends_out) B.ends_out[row] = start + B.size[0][row];\n"
                  // the records' rows are long: 16-byte chunk stores (BEmit16); the shorter rows of
                  // the tables below them keep the dword emitter (measured on pkg1: records 170 ->
                  // 134 us with BEmit16, the depth-1 tables 159 -> 180 us)
                  // (a framed record: its head is the first append of its emitter, which owns
                  // [start - 4, end))
                  << (t == 0 ? "      const uint32_t fh = B.frame_head;\n"
                               "      BEmit16 em{B.out, start - fh, start - fh};\n"
                               "      if (fh) em.be(B.size[0][row], 4);\n"
                             : "      BEmit em{{B.out}, start, start};\n")
                  << "      gen_wrow_" << t << "(em, D, B, row, start);\n"
                  << "    }\n    break;\n";
        o << "  default:\n"
          << "    for (uint64_t row = grid_first(); row < rows; row += grid_stride()) write_row_shaped(D, B, x, row);\n"
          << "  }\n}\n";
    }
    for (uint32_t x = 0; x < D.ntables; x++) {
        const TTable &T = D.t[x];
        has[x] = false;
        if (T.groot != x || !tree_group_ok(D, x)) continue;
        has[x] = true;
        o << "template <class Src>\n__device__ __forceinline__ void gen_row_" << x
          << "(const Src &s, const TreeDesc &D, const TreeBufs &B, uint64_t row, long long lo, long long hi, bool panic, "
             "uint2 *gr) {\n";
        if (T.shape == spec::SHAPE_VALUE) {
            const TField &F = D.f[T.field];
            o << "  Val v; int n;\n"
              << "  const bool ok = decode_value_kn<" << (int)F.elem << ">(s, lo, hi, 0, v, n);\n"
              << "  if (" << col_expr(F.col) << ") store_value_k<" << (int)F.elem << ">(" << col_expr(F.col) << ", row, v);\n"
              << "  store_u8(" << col_expr(T.status_col) << ", row, panic ? ST_PANIC : (ok ? ST_OK : ST_INVALID_VALUE));\n";
        } else if (T.shape == spec::SHAPE_STRUCT) {
            o << "  uint32_t sst = ST_OK;\n";
            gen_struct(o, D, T.field, "lo", "hi", "  ");
            o << "  store_u8(" << col_expr(T.status_col) << ", row, panic ? (uint32_t)ST_PANIC : sst);\n";
        } else {
            gen_message_table(o, D, x, "lo", "hi", true);
            gen_sub_tables(o, D, x, -1, nullptr, "tree_message_fallback");
        }
        // the group's kernel over rows staged in LDS, and spec_tree_group_<x>g: rows from HBM alone
        const std::string sym = "extern \"C\" __global__ __launch_bounds__(256) void spec_tree_group_" + std::to_string(x);
        const char *head =
            "(const TreeDesc *Dp, const TreeBufs *Bp, uint32_t x, uint32_t slab, uint32_t wave_bytes, uint32_t rpw) {\n"
            "  const TreeDesc &D = *Dp;\n"
            "  const TreeBufs &B = *Bp;\n"
            "  const uint64_t rows = dec_rows(D, B, x);\n"
            "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
            "  uint2 *gr = (uint2 *)(smem + (threadIdx.x >> 6) * wave_bytes + slab) + (threadIdx.x & 63);\n";
        o << "}\n"
          << sym << head
          << "  tree_rows(B, x, rows, slab, wave_bytes, rpw,\n"
          << "            [&](const TreeLds &s, uint64_t row, long long lo, long long hi, bool panic) {\n"
          << "              gen_row_" << x << "(s, D, B, row, lo, hi, panic, gr);\n"
          << "            },\n"
          << "            [&](const GlobalSrc &s, uint64_t row, long long lo, long long hi, bool panic) {\n"
          << "              gen_row_" << x << "(s, D, B, row, lo, hi, panic, gr);\n"
          << "            });\n"
          << "}\n"
          << sym << "g" << head
          << "  tree_rows_global(B, x, rows, [&](const GlobalSrc &s, uint64_t row, long long lo, long long hi, bool panic) {\n"
          << "    gen_row_" << x << "(s, D, B, row, lo, hi, panic, gr);\n"
          << "  });\n"
          << "}\n";
        // (4 waves per 64 rows: 110 vs 100 us for pkg1 — registers cap it at 3 waves per SIMD,
        // so 3 slabs per CU instead of 4)
        if (x == 0) gen_pair_rows(o, D, x, 2);
    }
    // level-fused list groups: the groups one decode level holds (lists owned by the previous
    // level's groups, rows from HBM) in ONE launch, blockIdx.y picking the group — each group is
    // a chain of dependent loads per row, so side by side their latencies overlap
    // (one launch for all of them: split by register budget — lists of values / structs at ~40
    // VGPRs, lists of messages at ~120 — the two launches ran back to back, 75.5 vs 70.5 us for
    // pkg1; amdgpu_waves_per_eu 6 or 8 spills: 86-87 us)
    {
        o << "extern \"C\" __global__ __launch_bounds__(256) void spec_tree_group_set"
          << "(const TreeDesc *Dp, const TreeBufs *Bp, TableSet ts, uint32_t wave_bytes) {\n"
          << "  const TreeDesc &D = *Dp;\n  const TreeBufs &B = *Bp;\n"
          << "  const uint32_t x = ts.t[blockIdx.y];\n  const uint64_t rows = dec_rows(D, B, x);\n"
          << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
          << "  uint2 *gr = (uint2 *)(smem + (threadIdx.x >> 6) * wave_bytes) + (threadIdx.x & 63);\n"
          << "  switch (x) {\n";
        for (uint32_t x = 1; x < D.ntables; x++)
            if (has[x])
                o << "  case " << x << ":\n"
                  << "    tree_rows_global(B, x, rows, [&](const GlobalSrc &s, uint64_t row, long long lo, long long hi, "
                     "bool panic) {\n"
                  << "      gen_row_" << x << "(s, D, B, row, lo, hi, panic, gr);\n"
                  << "    });\n    break;\n";
        o << "  default: break;\n  }\n}\n";
    }
    if (tree_tile(D)) gen_tile(o, D);
    return o.str();
}

// The kernels generate_tree(D, has) defined, by tree_internal.hpp TreeFn
static_assert(spec::TREE_FN_COUNT <= MODULE_MAX_FN, "Module::fn holds a tree's kernels");
std::vector<Kernel> tree_kernel_list(const TreeDesc &D, const bool *has) {
    std::vector<Kernel> v = {{spec::TREE_FN_SIZE_SET, "spec_tree_size_set"}, {spec::TREE_FN_GROUP_SET, "spec_tree_group_set"}};
    if (tree_tile(D)) v.push_back({spec::TREE_FN_WRITE_TILE, "spec_tree_write_tile"});
    else v.push_back({spec::TREE_FN_WRITE_SET, "spec_tree_write_set"});
    for (uint32_t x = 0; x < D.ntables; x++) {
        if (!has[x]) continue;
        const std::string name = "spec_tree_group_" + std::to_string(x);
        v.push_back({spec::TREE_FN_GROUP + (int)x, name});
        v.push_back({spec::TREE_FN_GROUP_HBM + (int)x, name + "g"});
        std::vector<char> sel[4];
        uint32_t tw[spec::TREE_MAX_T];
        if (x == 0 && pair_split(D, x, 2, sel, tw)) v.push_back({spec::TREE_FN_GROUP_PAIR + (int)x, name + "p2"});
    }
    return v;
}

} // namespace

namespace spec {

long long jit_compile_only_tree(const TreeDesc &D) {
    bool has[TREE_MAX_T];
    return compile_only(true, TREE, [&] { return generate_tree(D, has); });
}

// The kernels of a tree's generated module by tree_internal.hpp TreeFn: a group kernel for each
// group root that has one (nullptr where the run-time kernel runs), one of the encoder's two
// writers (nullptr for the other); nullptr when the JIT is off or failed.
const hipFunction_t *jit_tree_kernels(const TreeDesc &D) {
    if (!enabled()) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    // a repeated tree is found by its descriptor's bytes, without regenerating the source (every
    // spec_encode_tree call looks its kernels up)
    const Module *m = nullptr;
    if (!recall_module(dev, &D, sizeof(TreeDesc), &m)) {
        bool has[TREE_MAX_T];
        const std::string src = generate_tree(D, has);
        char key[48]; // (the source by its hash, as in the disk cache: the text is tens of kilobytes)
        snprintf(key, sizeof key, "tree:%d:%016llx", dev, (unsigned long long)source_hash(src));
        m = find_module(key, TREE, [&] { return load_module(compile_source(src, TREE), tree_kernel_list(D, has)); });
        remember_module(dev, &D, sizeof(TreeDesc), m);
    }
    return m ? m->fn : nullptr;
}

} // namespace spec

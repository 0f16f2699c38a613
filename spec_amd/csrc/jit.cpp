// jit.cpp — schema-specialised decode and encode kernels, compiled at run time with hiprtc.
//
// The reference decodes through GENERATED code: `spec generate` emits one Go reader per
// schema whose getters call Message.<Kind>(tag) with constant tags
// (internal/lang/generator/message.go:97-186).  This is the MI355X analogue: the first time
// a schema is decoded, decode_core.hpp's kernel body is instantiated for that schema (field
// count, kinds, tags and table order as compile-time constants) and compiled for gfx950
// with hiprtc; the code object is loaded with hipModuleLoadData and cached per (device,
// schema).  The generated kernel keeps the generic path for every record its fast path
// rejects, so results are identical to the precompiled kernel's.
//
// Every flat schema whose Writer table is strictly increasing has a generated kernel, whatever
// its field count or tags (has_flat_fast_path).  A schema with repeated tags or a list field, and every schema
// under SPEC_AMD_JIT=0, runs the precompiled run-time kernel (decode_flat.hip).
//
// Encode: the generated Write() (internal/lang/generator/message.go:319-439) likewise —
// encode_core.hpp's size and write bodies over SpecEnc<schema> (every column load of a
// record issued at once, the table built from registers); any schema of 1..ENC_MAX_FIELDS
// non-list fields.
#include <sstream>
#include <string>
#include <vector>
#include <cstring>

#include "jit_module.hpp"
#include "spec_internal.hpp"

namespace {

using namespace spec::jit;

// The kernels of a generated module, by program (flat_kernels / nested_kernels have their names)
// (the errmask variants: spec_decode_flat_errors; the present variants: spec_decode_flat_present)
enum DecodeFn { DEC_PAIR, DEC_PAIR_ERR, DEC_PAIR_PRESENT, DEC_PAIR_PRESENT_ERR };
enum EncodeFn { ENC_SIZE, ENC_WRITE, ENC_WRITE_FRAMES };
enum NestedFn { NEST_PAIR, NEST_RANGES };
enum NestedEncFn { NENC_SIZE, NENC_WRITE, NENC_WRITE_FRAMES, NENC_WRITE_PAIR, NENC_WRITE_PAIR_FRAMES };

// 1..max_fields fields, none a list if !lists, and the Writer's table (spec_internal.hpp
// table_order) strictly increasing with tags in 1..max_tag (max_tag 0: any order, any tags)
bool schema_fits(const spec_schema *s, uint32_t max_fields, bool lists, uint32_t max_tag) {
    if (s->nfields == 0 || s->nfields > max_fields) return false;
    for (uint32_t f = 0; !lists && f < s->nfields; f++)
        if (s->fields[f].kind == SPEC_KIND_LIST) return false;
    uint8_t order[SPEC_KFIELDS];
    if (max_tag) spec::table_order(s, order);
    for (uint32_t k = 0, below = 0; max_tag && k < s->nfields; k++) {
        const uint32_t tag = s->fields[order[k]].tag;
        if (tag <= below || tag > max_tag) return false;
        below = tag;
    }
    return true;
}

// The flat decoder's fast path (decode_core.hpp fast_wide, the batched path): any field count,
// tags <= 255 (small tables) or with a tag > 255 (every table big), no list field.
bool has_flat_fast_path(const spec_schema *s) { return schema_fits(s, SPEC_KFIELDS, false, 0xffff); }
// The nested decoder's fast path (decode_core.hpp fast_prepare, register-resident), per level:
// tags <= 255, at most FAST_MAX_FIELDS fields; a level without one is decoded generically.
bool has_fast_path(const spec_schema *s) { return schema_fits(s, spec::FAST_MAX_FIELDS, true, 255); }
// A schema-specialised encoder exists for 1..ENC_MAX_FIELDS fields without list fields.
constexpr uint32_t ENC_MAX_FIELDS = 32;
bool has_encoder(const spec_schema *s) { return schema_fits(s, ENC_MAX_FIELDS, false, 0); }

std::string key_of(const spec_schema *s, int device, Prog p) {
    std::ostringstream k;
    k << (p == ENCODE || p == NESTED_ENC ? "enc:" : "dec:") << device << ':';
    for (uint32_t f = 0; f < s->nfields; f++) k << s->fields[f].tag << '/' << (int)s->fields[f].kind << ',';
    return k.str();
}

bool any_big_tag(const spec_schema *s) { // a tag > 255: IsBigMessage forced, every table big
    bool big = false;
    for (uint32_t f = 0; f < s->nfields; f++) big = big || s->fields[f].tag > 255;
    return big;
}

// "struct <name> {" with N, kind[] and, each by its declaration, a[i] for i < N: the schema constants
// the kernel bodies are instantiated over
void emit_arrays(std::ostringstream &o, const char *name, const spec_schema *s,
                 std::initializer_list<std::pair<const char *, const uint16_t *>> arrays) {
    o << "struct " << name << " {\n  static constexpr int N = " << s->nfields << ";\n"
      << "  static constexpr uint32_t kind[N] = {";
    for (uint32_t f = 0; f < s->nfields; f++) o << (f ? "," : "") << (int)s->fields[f].kind;
    for (const auto &a : arrays) {
        o << "};\n  static constexpr " << a.first << "[N] = {";
        for (uint32_t i = 0; i < s->nfields; i++) o << (i ? "," : "") << (int)a.second[i];
    }
}

// struct <name> { N, kind[], rank[], stag[], order[], big }: the fast-path schema of decode_core.hpp
void emit_spec(std::ostringstream &o, const char *name, const spec_schema *s) {
    uint16_t order[SPEC_KFIELDS], sorted[SPEC_KFIELDS], rank[SPEC_KFIELDS];
    spec::table_order(s, order);
    for (uint32_t k = 0; k < s->nfields; k++) sorted[k] = s->fields[order[k]].tag, rank[order[k]] = (uint16_t)k;
    emit_arrays(o, name, s, {{"int rank", rank}, {"uint32_t stag", sorted}, {"int order", order}});
    o << "};\n  static constexpr bool big = " << (any_big_tag(s) ? "true" : "false") << ";\n};\n";
}

// waves per 64-record group of the flat decode (decode_core.hpp decode_flat_pair)
constexpr int FLAT_WAVES = 2;

// wide schemas and big tables get kernels of their own names (traces tell them apart); their
// _present kernels read full tables only (decode_core.hpp fast_wide)
bool flat_wide(const spec_schema *s) { return s->nfields > (uint32_t)spec::FAST_MAX_FIELDS || any_big_tag(s); }

std::string generate_decode(const spec_schema *s) {
    std::ostringstream o;
    o << "#include \"decode_core.hpp\"\n";
    emit_spec(o, "GenSpec", s);
    const char *w = flat_wide(s) ? "_wide" : "";
    // the wave-pair kernel (decode_core.hpp decode_flat_pair): every schema's launch, plain and with
    // the error masks; then spec_decode_flat_present: the HasField masks, further instantiations in
    // the same module (the first two keep their code; build()'s precompile of a schema covers these)
    const int P = FLAT_WAVES;
    for (const char *present : {"", "_present"})
        for (const char *err : {"", "_err"})
            o << "extern \"C\" __global__ __launch_bounds__(" << 64 * P << ") void spec_decode_flat" << w << present << err
              << "_pair_jit(spec::DecodeArgs a) {\n"
              << "  spec::decode_flat_pair<GenSpec, " << (*err ? "true" : "false") << ", " << P
              << (*present ? ", true" : "") << ">(a);\n}\n";
    return o.str();
}

// The nested decode's wave group (decode_nested_core.hpp nested_decode_pair): waves per group
// and item rounds of 64 per wave in flight.
constexpr int NESTED_WAVES = 2, NESTED_U = 1;

// Nested decode after the index kernels: outer and item fast paths where the schema has one.
std::string generate_nested(const spec_nested_schema *s) {
    std::ostringstream o;
    o << "#include \"decode_nested_core.hpp\"\n";
    const bool fo = has_fast_path(&s->outer), fi = has_fast_path(&s->item);
    if (fo) emit_spec(o, "GenOuter", &s->outer);
    if (fi) emit_spec(o, "GenItem", &s->item);
    const std::string specs = std::string(fo ? "GenOuter" : "spec::RuntimeSpec") + ", " +
                              (fi ? "GenItem" : "spec::RuntimeSpec");
    o << "extern \"C\" __global__ __launch_bounds__(64) void spec_decode_nested3_jit(spec::NestedArgs a) {\n"
      << "  spec::nested_decode_body<" << specs << ", true>(a);\n}\n"
      << "extern \"C\" __global__ __launch_bounds__(" << 64 * NESTED_WAVES
      << ") void spec_decode_nested_pair_jit(spec::NestedArgs a) {\n"
      << "  spec::nested_decode_pair<" << specs << ", " << NESTED_U << ", " << NESTED_WAVES << ">(a);\n}\n";
    return o.str();
}

// The generated Write() of internal/lang/generator/message.go:319-439 as constants: fields in
// write order, the Writer's table order, IsBigMessage forced by a tag > 255.
void emit_enc_spec(std::ostringstream &o, const char *name, const spec_schema *s) {
    uint16_t order[SPEC_KFIELDS], tag[SPEC_KFIELDS];
    spec::table_order(s, order);
    for (uint32_t f = 0; f < s->nfields; f++) tag[f] = s->fields[f].tag;
    emit_arrays(o, name, s, {{"uint32_t tag", tag}, {"int order", order}});
    o << "};\n  static constexpr bool big_forced = " << (any_big_tag(s) ? "true" : "false") << ";\n};\n";
}

// Nested encode: SpecEnc for the outer schema (its list field handled by the nested encoder's
// hooks) and for the item schema, RuntimeEnc for a side without a specialised encoder.
bool has_outer_encoder(const spec_schema *s) { return s->nfields > 0 && s->nfields <= ENC_MAX_FIELDS; }
bool nested_wide(const spec_nested_schema *s) {
    return s->outer.nfields > (uint32_t)SPEC_KFIELDS || s->item.nfields > (uint32_t)SPEC_KFIELDS;
}
bool has_nested_encoder(const spec_nested_schema *s) {
    return !nested_wide(s) && (has_outer_encoder(&s->outer) || has_encoder(&s->item));
}

std::string generate_nested_encode(const spec_nested_schema *s) {
    std::ostringstream o;
    o << "#include \"encode_nested_core.hpp\"\n";
    const bool fo = has_outer_encoder(&s->outer), fi = has_encoder(&s->item);
    if (fo) emit_enc_spec(o, "GenOuter", &s->outer);
    if (fi) emit_enc_spec(o, "GenItem", &s->item);
    o << "using OP = " << (fo ? "spec::SpecEnc<GenOuter>" : "spec::RuntimeEnc") << ";\n"
      << "using IP = " << (fi ? "spec::SpecEnc<GenItem>" : "spec::RuntimeEnc") << ";\n";
    auto kernel = [&](int threads, const char *name, const char *body) {
        o << "extern \"C\" __global__ __launch_bounds__(" << threads << ") void spec_encode_nested_" << name
          << "_jit(spec::NestedEncodeArgs a) {\n"
          << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
          << "  spec::nested_enc_" << body << "(a, smem);\n}\n";
    };
    kernel(256, "size", "size_body<OP, IP>");
    kernel(256, "write", "write_body<OP, IP>");
    // spec_encode_nested_frames: the same write passes with the 4-byte mpx frame head per record,
    // further instantiations in the same module (the unframed kernels' code does not change)
    kernel(256, "write_frames", "write_body<OP, IP, 4>");
    if (fo) { // the write pass on wave pairs (needs the outer list field at a constant index)
        kernel(512, "write_pair", "write_pair_body<OP, IP>");
        kernel(512, "write_pair_frames", "write_pair_body<OP, IP, 4>");
    }
    return o.str();
}

std::string generate_encode(const spec_schema *s) {
    std::ostringstream o;
    o << "#include \"encode_core.hpp\"\n";
    emit_enc_spec(o, "GenEnc", s);
    o << "using P = spec::SpecEnc<GenEnc>;\n"
      << "extern \"C\" __global__ __launch_bounds__(256) void spec_encode_size_jit(spec::EncodeArgs a) {\n"
      << "  spec::encode_size_body<P>(a);\n}\n"
      << "extern \"C\" __global__ __launch_bounds__(256) void spec_encode_write_jit(spec::EncodeArgs a) {\n"
      << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
      << "  spec::encode_write_body<P>(a, smem);\n}\n"
      // spec_encode_flat_frames: the same write pass with the 4-byte mpx frame head per record,
      // a second instantiation in the same module (the unframed kernel's code does not change)
      << "extern \"C\" __global__ __launch_bounds__(256) void spec_encode_write_frames_jit(spec::EncodeArgs a) {\n"
      << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n"
      << "  spec::encode_write_body<P, spec::EncodeArgs, 4>(a, smem);\n}\n";
    return o.str();
}

// The kernels of each program's module (the nested encoder's pair kernels: only with a
// specialised outer encoder)
std::vector<Kernel> flat_kernels(const spec_schema *s, Prog p) {
    if (p == ENCODE)
        return {{ENC_SIZE, "spec_encode_size_jit"}, {ENC_WRITE, "spec_encode_write_jit"},
                {ENC_WRITE_FRAMES, "spec_encode_write_frames_jit"}};
    const std::string n = flat_wide(s) ? "spec_decode_flat_wide_" : "spec_decode_flat_";
    return {{DEC_PAIR, n + "pair_jit"}, {DEC_PAIR_ERR, n + "err_pair_jit"},
            {DEC_PAIR_PRESENT, n + "present_pair_jit"}, {DEC_PAIR_PRESENT_ERR, n + "present_err_pair_jit"}};
}
std::vector<Kernel> nested_kernels(Prog p) {
    if (p == NESTED) return {{NEST_PAIR, "spec_decode_nested_pair_jit"}, {NEST_RANGES, "spec_decode_nested3_jit"}};
    return {{NENC_SIZE, "spec_encode_nested_size_jit"},
            {NENC_WRITE, "spec_encode_nested_write_jit"},
            {NENC_WRITE_FRAMES, "spec_encode_nested_write_frames_jit"},
            {NENC_WRITE_PAIR, "spec_encode_nested_write_pair_jit", true},
            {NENC_WRITE_PAIR_FRAMES, "spec_encode_nested_write_pair_frames_jit", true}};
}

const Module *lookup(const spec_schema *s, Prog p) {
    if (!enabled() || s->nfields > SPEC_KFIELDS) return nullptr; // wide schemas: generic kernels
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    // the last few (device, program, schema) answers of this thread: a repeated call (every
    // launch of a steady-state loop, one per device in spec_shard_decode) skips building the key
    // string and the locked map lookup
    struct Hit {
        bool valid = false;
        int dev = 0, prog = 0;
        uint32_t nfields = 0;
        spec_field f[SPEC_KFIELDS];
        const Module *e = nullptr;
    };
    thread_local Hit hits[8];
    thread_local unsigned next = 0;
    const size_t fb = (size_t)s->nfields * sizeof(spec_field);
    for (const Hit &h : hits)
        if (h.valid && h.dev == dev && h.prog == (int)p && h.nfields == s->nfields && memcmp(h.f, s->fields, fb) == 0)
            return h.e;
    const Module *e = nullptr;
    if (p == ENCODE ? has_encoder(s) : has_flat_fast_path(s))
        e = find_module(key_of(s, dev, p), p, [&] {
            return load_module(compile_source(p == ENCODE ? generate_encode(s) : generate_decode(s), p), flat_kernels(s, p));
        });
    Hit &h = hits[next++ & 7];
    h.valid = true;
    h.dev = dev;
    h.prog = (int)p;
    h.nfields = s->nfields;
    memcpy(h.f, s->fields, fb);
    h.e = e;
    return e;
}

// a nested kernel is worth compiling when the outer or the item schema has a fast path
// (a half of more than SPEC_KFIELDS fields: the nested schema is decoded in field chunks by the
// run-time kernels, capi.hip nested_decode_chunks, never by a generated kernel: nested_wide)
bool has_nested_fast_path(const spec_nested_schema *s) {
    return !nested_wide(s) && (has_fast_path(&s->outer) || has_fast_path(&s->item));
}

// p: NESTED or NESTED_ENC
const Module *lookup_nested(const spec_nested_schema *s, Prog p) {
    if (!enabled() || !(p == NESTED ? has_nested_fast_path(s) : has_nested_encoder(s))) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const std::string k = key_of(&s->outer, dev, p) + "|" + key_of(&s->item, dev, p) + (p == NESTED ? "" : "|n");
    return find_module(k, p, [&] {
        return load_module(compile_source(p == NESTED ? generate_nested(s) : generate_nested_encode(s), p),
                           nested_kernels(p));
    });
}

} // namespace

namespace spec {

long long jit_compile_only(const spec_schema *s, double) {
    return compile_only(has_flat_fast_path(s), DECODE, [&] { return generate_decode(s); });
}
long long jit_compile_only_encode(const spec_schema *s) {
    return compile_only(has_encoder(s), ENCODE, [&] { return generate_encode(s); });
}
long long jit_compile_only_nested(const spec_nested_schema *s) {
    return compile_only(has_nested_fast_path(s), NESTED, [&] { return generate_nested(s); });
}
long long jit_compile_only_nested_encode(const spec_nested_schema *s) {
    return compile_only(has_nested_encoder(s), NESTED_ENC, [&] { return generate_nested_encode(s); });
}

// (the answer is jit_launch_decode_flat's for a batch of that mean record size: a batch whose
// 64-record span has no LDS slab launches the generic kernel whatever the schema)
int jit_prepare_decode_flat(const spec_schema *schema, double avg_record) {
    return decode_slab_bytes(avg_record) != 0 && lookup(schema, DECODE) ? 1 : 0;
}

int jit_prepare_encode_flat(const spec_schema *schema) { return lookup(schema, ENCODE) ? 1 : 0; }

int jit_launch_decode_flat(const spec_schema *schema, const DecodeArgs &a, double avg_record, hipStream_t stream) {
    if (decode_slab_bytes(avg_record) == 0) return 0; // records too large for LDS: generic kernel
    const Module *m = lookup(schema, DECODE);
    if (!m) return 0;
    if (a.n <= a.r0) return 1;
    // a wave pair per 64 records, one slab per pair (+ 256 B exchange, + 512 B per kind of mask),
    // the groups in 8 equal XCD shares
    DecodeArgs args = a;
    args.slab = decode_slab_bytes(avg_record);
    args.xcd = 1;
    const uint64_t groups = ((a.n - a.r0 + 63) / 64 + 7) / 8 * 8;
    const int fn = a.f.present ? (a.f.errmask ? DEC_PAIR_PRESENT_ERR : DEC_PAIR_PRESENT)
                               : (a.f.errmask ? DEC_PAIR_ERR : DEC_PAIR);
    const unsigned xch = 256 + (a.f.errmask ? 512 : 0) + (a.f.present ? 512 : 0);
    return launch_module(m->fn[fn], (unsigned)groups, 64 * FLAT_WAVES, args.slab + (FLAT_WAVES - 1) * xch, stream, &args,
                         sizeof args);
}

int jit_launch_encode(const spec_schema *schema, const EncodeArgs &a, bool write, hipStream_t stream) {
    const Module *m = lookup(schema, ENCODE);
    if (!m) return 0;
    // (the framed write pass, a.frame_head: the framed instantiation of the same kernel)
    const int fn = !write ? ENC_SIZE : a.frame_head ? ENC_WRITE_FRAMES : ENC_WRITE;
    return launch_module(m->fn[fn], (unsigned)a.nblocks, ENC_BLOCK, write ? (unsigned)enc_write_lds_bytes() : 0, stream, &a,
                         sizeof a);
}

int jit_launch_nested(const spec_nested_schema *schema, const NestedArgs &a, int mode, hipStream_t stream) {
    if (a.slab == 0) return 0; // records too large for LDS: generic kernel
    const Module *m = lookup_nested(schema, NESTED);
    if (!m) return 0;
    unsigned grid = (unsigned)((a.n + 63) / 64);
    if (a.xcd) grid = (grid + 7) / 8 * 8; // 8 equal XCD shares
    const bool ranges = mode == NESTED_RANGES; // a wave per group; else a wave pair (nested_decode_pair)
    // LDS: the slab, then the ranges' window or the pair's posted lists (4 words per record)
    const size_t lds = a.slab + (ranges ? NESTED_RANGE_BYTES : 1024u);
    return launch_module(m->fn[ranges ? NEST_RANGES : NEST_PAIR], grid, ranges ? 64 : 64 * NESTED_WAVES, (unsigned)lds,
                         stream, &a, sizeof a);
}

int jit_launch_nested_encode(const spec_nested_schema *schema, const NestedEncodeArgs &a, bool write,
                             hipStream_t stream) {
    const Module *m = lookup_nested(schema, NESTED_ENC);
    if (!m) return 0;
    NestedEncodeArgs args = a;
    args.xcd = write ? 1u : 0u;
    const unsigned lds = (unsigned)(write ? nenc_write_lds_bytes() : nenc_size_lds_bytes());
    const unsigned grid = (unsigned)(args.xcd ? (a.nblocks + 7) / 8 * 8 : a.nblocks);
    // the write pass on wave pairs when the size pass left its item prefixes (nested_enc_write_pair_body)
    const bool pair = write && m->fn[NENC_WRITE_PAIR] && a.item_pre && a.wave_ok;
    // (the framed write pass, a.frame_head: the framed instantiation of the same kernel)
    const int fn = !write         ? NENC_SIZE
                   : a.frame_head ? (pair ? NENC_WRITE_PAIR_FRAMES : NENC_WRITE_FRAMES)
                                  : (pair ? NENC_WRITE_PAIR : NENC_WRITE);
    return launch_module(m->fn[fn], grid, pair ? 2 * NENC_BLOCK : NENC_BLOCK, lds, stream, &args, sizeof args);
}

} // namespace spec

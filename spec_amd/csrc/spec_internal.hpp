// spec_internal.hpp — kernel argument blocks and launcher declarations shared by the HIP
// translation units of libspec_amd.so (not part of the public C ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/spec_amd.h"
#include "decode_core.hpp"
#include "encode_core.hpp"
#include "encode_nested_core.hpp"
#include "decode_nested_core.hpp"

namespace spec {

// The hiprtc modules take spec::EncodeArgs by value as a raw parameter buffer, and the precompiled
// kernels' argument segments are these blocks: their layouts do not move.
static_assert(sizeof(EncodeArgs) == 1880 && sizeof(WideEncodeArgs) == 128, "flat encode argument blocks");
static_assert(sizeof(PresentEncodeArgs) == 1896 && sizeof(WidePresentEncodeArgs) == 144,
              "flat encode argument blocks with a presence mask");

// Table order a Writer produces for this schema: messageStack.insert over the tags in write
// order, insertion sort where an equal tag written later moves before the earlier one
// (internal/writer/stack_msg.go:37-61).  order[j] = schema index of the j-th table entry.
// The insertion moves a new entry left past every entry whose tag is >= its own, so the result
// is the unique order by (tag ascending, write index descending): sorted in O(n log n) here
// (a 1024-field schema in reverse tag order cost ~0.5 M swaps per call as an insertion sort).
// The one definition behind EncFields::order, the wide field set's inv_order, FieldSet::rank and
// the order[] constants of the schema-specialised kernels (jit.cpp).
template <class T>
void table_order(const spec_schema *s, T *order) {
    uint32_t key[SPEC_MAX_FIELDS]; // tag << 16 | (0xffff - index): ascending = the Writer's order
    for (uint32_t f = 0; f < s->nfields; f++) key[f] = (uint32_t)s->fields[f].tag << 16 | (0xffffu - f);
    std::sort(key, key + s->nfields);
    for (uint32_t j = 0; j < s->nfields; j++) order[j] = (T)(0xffffu - (key[j] & 0xffffu));
}

// The tree encoder's record-tile writer (jit_tree.cpp gen_tile): waves per workgroup (= field blocks of
// the records' table) and waves per SIMD the kernel is compiled for (amdgpu_waves_per_eu, its
// register budget): 4 WPE / W workgroups per CU share the LDS, per workgroup the image of the
// tile's output range and a dummy dword
constexpr int TREE_TILE_W = 4, TREE_TILE_WPE = 4;
constexpr uint32_t TREE_TILE_IMG = ((163840u / (4u * TREE_TILE_WPE / TREE_TILE_W)) - 32u) & ~15u;

// encode_nested.hip
int launch_nested_encode(const spec_nested_schema *schema, const NestedEncodeArgs &a, bool write,
                         hipStream_t stream);
// jit.cpp: schema-specialised nested encode pass 1 (write=false) or 3; 1 launched, 0 use the
// precompiled kernel, <0 HIP error.
int jit_launch_nested_encode(const spec_nested_schema *schema, const NestedEncodeArgs &a, bool write,
                             hipStream_t stream);
long long jit_compile_only_nested_encode(const spec_nested_schema *schema);
int launch_decode_flat(DecodeArgs a, double avg_record, hipStream_t stream);
// lz4_device.hip
int launch_lz4_decompress(const uint8_t *src, uint64_t src_len, const spec_lz4_block *blocks, uint64_t nblocks,
                          uint8_t *slots, uint64_t slot, uint32_t *sizes, uint8_t *status, hipStream_t stream);
int launch_lz4_pack(const uint8_t *slots, uint64_t slot, const uint32_t *sizes, uint64_t nblocks, uint8_t *out,
                    uint64_t out_cap, uint64_t *offsets, uint64_t *total, hipStream_t stream);
// xxHash32 of the frame content: data != null appends data[0, len); digest != null writes the digest
int launch_lz4_content(spec_lz4_content *c, const uint8_t *data, uint64_t len, uint32_t *digest, hipStream_t stream);
// lz4_compress.hip: data[0, len) as blocks of an LZ4 frame at out (header: the 7 header bytes,
// little-endian, written with SPEC_LZ4_OPEN); the workspace is lz4c::workspace_layout(len, block_max)
int launch_lz4_compress_frame(const uint8_t *data, uint64_t len, uint32_t block_max, uint32_t flags, uint64_t header,
                              const uint32_t *content_digest, uint8_t *out, uint64_t *total, void *workspace,
                              hipStream_t stream);
// frames_write.hip
int launch_frames_write(const uint8_t *stream_bytes, uint64_t stream_len, const uint64_t *ends, uint64_t n,
                        uint8_t *frames, uint64_t *frame_ends, hipStream_t stream);
// frames_device.hip
size_t frames_index_device_workspace(uint64_t len);
int launch_frames_index_device(const uint8_t *buf, uint64_t len, uint64_t *ends, uint64_t cap, uint64_t *count,
                               uint64_t *consumed, int32_t *status, void *ws, hipStream_t stream);
int device_cus(); // CUs of the current device (cached)
void note_hip_error(hipError_t e); // capi.hip: remembered for spec_last_hip_error()
// capi.hip: bytes copied to the device on st from a pooled pinned slot of the current device (no
// host wait: the pool grows while every slot's copy is in flight; not graph-capturable)
hipError_t pinned_upload(void *dst, const void *src, size_t bytes, hipStream_t st);
int launch_parse(DecodeArgs a, uint32_t *sizes, uint32_t root, double avg_record, hipStream_t stream);
int launch_nested_index(NestedArgs a, double avg_record, hipStream_t stream);
int launch_nested_decode(const spec_nested_schema *schema, NestedArgs a, double avg_record, hipStream_t stream);
int launch_nested_onepass(const spec_nested_schema *schema, NestedArgs a, double avg_record, hipStream_t stream);
// jit.cpp: the nested decode pass after the index kernels, specialised to the outer and item
// schemas; 1 launched, 0 use the precompiled kernel, <0 HIP error.  a.slab must be set.
// mode: NESTED_GROUPS (a wave pair per group, items found by an owner search) or NESTED_RANGES
// (a wave per group, items from ranges precomputed into LDS by their records' lanes).  The other
// values are spec_set_nested_mode's only (decode_nested.hip): NESTED_HALVES (as GROUPS, slabs for
// half a group), NESTED_TAILCOUNT (as GROUPS, the count pass from each record's last 64 bytes),
// NESTED_XCD (as TAILCOUNT with an XCD-aware block order for the decode pass: the default)
enum { NESTED_GROUPS = 1, NESTED_RANGES = 2, NESTED_HALVES = 3, NESTED_TAILCOUNT = 4, NESTED_XCD = 5 };
int jit_launch_nested(const spec_nested_schema *schema, const NestedArgs &a, int mode, hipStream_t stream);
long long jit_compile_only_nested(const spec_nested_schema *schema);
// jit.cpp: schema-specialised decode kernel (hiprtc); returns 1 if launched, 0 if the caller
// should launch the generic kernel, <0 on a HIP error.
int jit_launch_decode_flat(const spec_schema *schema, const DecodeArgs &a, double avg_record, hipStream_t stream);
int jit_prepare_decode_flat(const spec_schema *schema, double avg_record);
int jit_prepare_encode_flat(const spec_schema *schema); // 1: jit_launch_encode will launch, 0: it will not
void jit_set_enabled(int on); // jit_module.cpp
long long jit_compile_only(const spec_schema *schema, double avg_record);
long long jit_compile_only_encode(const spec_schema *schema);
// capi.hip: spec_encode_flat's passes (ENC_PASS_SIZE: sizes + scan into the workspace, heaps
// checked; ENC_PASS_WRITE: the write pass over a workspace the size pass filled), every end
// offset + ends_base (shard.hip: a shard's first byte in the whole batch).  frame_head = 4
// (spec_encode_flat_frames): every record behind its u32 BE size, ends[] the frame ends.
enum { ENC_PASS_SIZE = 1, ENC_PASS_WRITE = 2 };
int encode_flat_passes(const spec_schema *schema, const void *const *columns, const uint8_t *const *heaps,
                       const uint64_t *heap_lens, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *ends,
                       uint64_t ends_base, void *workspace, size_t workspace_size, uint64_t *total, int passes,
                       hipStream_t stream, uint32_t frame_head = 0);
// encode_flat.hip: the flat encoder's passes over any of the four argument blocks (EncodeArgs,
// WideEncodeArgs, PresentEncodeArgs, WidePresentEncodeArgs): sizes + scan; write.  0, or -1 on a
// HIP error.  The framed instantiations are chosen from a.frame_head, the schema-specialised
// kernels (jit_launch_encode) tried for EncodeArgs alone.
template <class A>
int launch_encode_size(const spec_schema *schema, const A &a, hipStream_t stream);
template <class A>
int launch_encode_write(const spec_schema *schema, const A &a, hipStream_t stream);
// pass 2 of the flat and nested encoders: one workgroup, block_sums[0, nblocks) -> exclusive
// offsets and the total; frame_head bytes more for each of the n records
void launch_encode_scan(uint64_t *block_sums, uint64_t nblocks, uint64_t *total, uint64_t n, uint32_t frame_head,
                        hipStream_t stream);
// jit.cpp: schema-specialised encode pass 1 (write=false) or 3; 1 launched, 0 use the
// precompiled kernel, <0 HIP error.
int jit_launch_encode(const spec_schema *schema, const EncodeArgs &a, bool write, hipStream_t stream);

// jit_tree.cpp: the kernels of a tree's generated module (tree.hip, tree_decode.hip)
struct TreeDesc;
const hipFunction_t *jit_tree_kernels(const TreeDesc &D);
long long jit_compile_only_tree(const TreeDesc &D);
// tree.hip: spec_encode_tree (frame_head 0) / spec_encode_tree_frames (4)
int encode_tree_passes(const spec_tree *tree, const void *const *columns, const uint8_t *const *heaps,
                       const uint64_t *heap_lens, const uint64_t *rows, uint8_t *out, uint64_t out_cap, uint64_t *ends,
                       void *workspace, size_t workspace_size, uint64_t *total, void *stream, uint32_t frame_head);

} // namespace spec

// encode_flat.hip — bulk encode of SoA columns into flat spec messages (gfx950).
//
// Replaces, per record, the generated Write() sequence over the Writer stack machine:
//   w := spec.NewMessageWriterBuffer(buf)                       writer_msg.go:26-31
//   w.Field(tag).<Kind>(v) for each field in schema order         internal/writer/msg.go:99-211
//     -> ValueWriter.<Kind> -> encode.Encode<Kind> (internal/encode/...) + pushData
//     -> writer.field(tag): insertion-sorted table entry {tag, end - message.start}
//                                                                 internal/writer/writer.go:409-436,
//                                                                 internal/writer/stack_msg.go:37-61
//   w.Build() -> endMessage -> encode.EncodeMessageTable          internal/writer/writer.go:520-553,
//                                                                 internal/encode/msg.go:15-77
// The table order depends only on the schema's tags, so the host computes it once
// (`order`, same insertion-sort tie rule); per record only the sizes vary.
//
// Three launches, no host sync:
//   1. encode_size_kernel<Enc, A>        : per-record encoded size, per-block sums (reads only the
//                            columns that affect sizes: varint and string/bytes columns)
//   2. encode_scan_kernel<HEAD>          : exclusive scan of block sums (one workgroup) + total
//   3. encode_write_kernel<Enc, A, HEAD> : per-block scan of recomputed sizes -> record offsets; each
//                            lane emits its record into the wave's LDS slab (dword-merging byte
//                            emitter), then the wave copies the slab to HBM with 16-byte
//                            stores; ends[] written coalesced.  A wave whose output span does
//                            not fit the slab emits straight to HBM.
// Passes 1 and 3 are, for schemas jit.cpp accepts, schema-specialised kernels compiled at run
// time (all column loads of a record issued together, the table emitted from registers).
//
// The variants are the instantiations of those three templates.  A, the argument block
// (encode_core.hpp EncodeArgsT<Fields>), is chosen by the C ABI entry point: narrow or wide by
// the schema's field count, dense or present by the call (spec_encode_flat_present*); Enc follows
// from it (RuntimeEncT<A::kPresent>).  HEAD is chosen at launch from a.frame_head: 0, or 4
// (spec_encode_flat*_frames), where every record leaves as its mpx frame [u32 BE size][message]
// (mpx/conn_writer.go:84-97), the head emitted into the slab with the record; pass 1 is shared,
// pass 2 adds the heads to the block sums.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/spec_amd.h"
#include "encode_core.hpp"
#include "spec_internal.hpp"

namespace spec {

// Kernel bodies: encode_core.hpp (RuntimeEncT here; jit.cpp instantiates them per schema).

template <class Enc, class A>
__global__ __launch_bounds__(ENC_BLOCK) void encode_size_kernel(A a) {
    encode_size_body<Enc>(a);
}

template <int HEAD>
__global__ __launch_bounds__(1024) void encode_scan_kernel(uint64_t *block_sums, uint64_t nblocks, uint64_t *total,
                                                           uint64_t n) {
    scan_block_sums<HEAD>(block_sums, nblocks, total, n);
}

template <class Enc, class A, int HEAD>
__global__ __launch_bounds__(ENC_BLOCK) void encode_write_kernel(A a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<Enc, A, HEAD>(a, smem);
}

constexpr int FRAME_HEAD = 4;

void launch_encode_scan(uint64_t *block_sums, uint64_t nblocks, uint64_t *total, uint64_t n, uint32_t frame_head,
                        hipStream_t stream) {
    hipLaunchKernelGGL(frame_head ? encode_scan_kernel<FRAME_HEAD> : encode_scan_kernel<0>, dim3(1), dim3(1024), 0,
                       stream, block_sums, nblocks, total, n);
}

// The narrow dense block alone has schema-specialised kernels (jit_launch_encode: 1 launched, 0 use
// the kernel here, < 0 a HIP error).
template <class A>
static int try_jit(const spec_schema *schema, const A &a, bool write, hipStream_t stream) {
    if constexpr (std::is_same_v<A, EncodeArgs>) return jit_launch_encode(schema, a, write, stream);
    return 0;
}

template <class A>
int launch_encode_size(const spec_schema *schema, const A &a, hipStream_t stream) {
    const int j = a.nblocks ? try_jit(schema, a, false, stream) : 1;
    if (j < 0) return -1;
    if (j == 0)
        hipLaunchKernelGGL((encode_size_kernel<RuntimeEncT<A::kPresent>, A>), dim3((unsigned)a.nblocks), dim3(ENC_BLOCK),
                           0, stream, a);
    launch_encode_scan(a.block_sums, a.nblocks, a.total, a.n, a.frame_head, stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class A>
int launch_encode_write(const spec_schema *schema, const A &a, hipStream_t stream) {
    if (!a.nblocks) return 0;
    using Enc = RuntimeEncT<A::kPresent>;
    const int j = try_jit(schema, a, true, stream);
    if (j < 0) return -1;
    if (j == 0)
        hipLaunchKernelGGL((a.frame_head ? encode_write_kernel<Enc, A, FRAME_HEAD> : encode_write_kernel<Enc, A, 0>),
                           dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), enc_write_lds_bytes(), stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

#define SPEC_ENCODE_LAUNCHERS(A)                                                                   \
    template int launch_encode_size<A>(const spec_schema *, const A &, hipStream_t);              \
    template int launch_encode_write<A>(const spec_schema *, const A &, hipStream_t);
SPEC_ENCODE_LAUNCHERS(EncodeArgs)
SPEC_ENCODE_LAUNCHERS(WideEncodeArgs)
SPEC_ENCODE_LAUNCHERS(PresentEncodeArgs)
SPEC_ENCODE_LAUNCHERS(WidePresentEncodeArgs)
#undef SPEC_ENCODE_LAUNCHERS

} // namespace spec

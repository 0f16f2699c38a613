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
//   1. encode_size_kernel  : per-record encoded size, per-block sums (reads only the columns
//                            that affect sizes: varint and string/bytes columns)
//   2. encode_scan_kernel  : exclusive scan of block sums (one workgroup) + total
//   3. encode_write_kernel : per-block scan of recomputed sizes -> record offsets; each lane
//                            emits its record into the wave's LDS slab (dword-merging byte
//                            emitter), then the wave copies the slab to HBM with 16-byte
//                            stores; ends[] written coalesced.  A wave whose output span does
//                            not fit the slab emits straight to HBM.
// Passes 1 and 3 are, for schemas jit.cpp accepts, schema-specialised kernels compiled at run
// time (all column loads of a record issued together, the table emitted from registers).
//
// spec_encode_flat_frames (EncodeArgs::frame_head = 4) runs the same three launches with the
// framed instantiations of passes 2 and 3: every record leaves as its mpx frame
// [u32 BE size][message] (mpx/conn_writer.go:84-97), the head emitted into the slab with the
// record.  Pass 1 is shared; pass 2 adds the heads to the block sums.
#include <hip/hip_runtime.h>

#include "../../include/spec_amd.h"
#include "encode_core.hpp"
#include "spec_internal.hpp"

namespace spec {

// Kernel bodies: encode_core.hpp (RuntimeEnc here; jit.cpp instantiates them per schema).

__global__ __launch_bounds__(ENC_BLOCK) void encode_size_kernel(EncodeArgs a) { encode_size_body<RuntimeEnc>(a); }

__global__ __launch_bounds__(1024) void encode_scan_kernel(EncodeArgs a) { scan_block_sums(a.block_sums, a.nblocks, a.total); }

__global__ __launch_bounds__(ENC_BLOCK) void encode_write_kernel(EncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimeEnc>(a, smem);
}

// Schemas with more than SPEC_KFIELDS fields: the same bodies over a field set in device memory
// (RuntimeEnc reads it through WideEncFields' pointers; no schema-specialised kernel).
__global__ __launch_bounds__(ENC_BLOCK) void encode_wide_size_kernel(WideEncodeArgs a) {
    encode_size_body<RuntimeEnc>(a);
}

__global__ __launch_bounds__(1024) void encode_wide_scan_kernel(WideEncodeArgs a) {
    scan_block_sums(a.block_sums, a.nblocks, a.total);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_wide_write_kernel(WideEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimeEnc>(a, smem);
}

// The framed encoders: frame heads counted by the scan, written by the write pass.
constexpr int FRAME_HEAD = 4;

__global__ __launch_bounds__(1024) void encode_scan_frames_kernel(EncodeArgs a) {
    scan_block_sums<FRAME_HEAD>(a.block_sums, a.nblocks, a.total, a.n);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_write_frames_kernel(EncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimeEnc, EncodeArgs, FRAME_HEAD>(a, smem);
}

__global__ __launch_bounds__(1024) void encode_wide_scan_frames_kernel(WideEncodeArgs a) {
    scan_block_sums<FRAME_HEAD>(a.block_sums, a.nblocks, a.total, a.n);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_wide_write_frames_kernel(WideEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimeEnc, WideEncodeArgs, FRAME_HEAD>(a, smem);
}

// spec_encode_flat_present[_frames]: the same bodies over a field set with a per-record presence
// mask (RuntimePresentEnc: only the fields of a record's mask are written), narrow and wide, plain
// and framed.  The scans are the dense encoders' (scan_block_sums<0|4>).
__global__ __launch_bounds__(ENC_BLOCK) void encode_present_size_kernel(PresentEncodeArgs a) {
    encode_size_body<RuntimePresentEnc>(a);
}

__global__ __launch_bounds__(1024) void encode_present_scan_kernel(uint64_t *block_sums, uint64_t nblocks,
                                                                    uint64_t *total) {
    scan_block_sums(block_sums, nblocks, total);
}

__global__ __launch_bounds__(1024) void encode_present_scan_frames_kernel(uint64_t *block_sums, uint64_t nblocks,
                                                                           uint64_t *total, uint64_t n) {
    scan_block_sums<FRAME_HEAD>(block_sums, nblocks, total, n);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_present_write_kernel(PresentEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimePresentEnc>(a, smem);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_present_write_frames_kernel(PresentEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimePresentEnc, PresentEncodeArgs, FRAME_HEAD>(a, smem);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_wide_present_size_kernel(WidePresentEncodeArgs a) {
    encode_size_body<RuntimePresentEnc>(a);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_wide_present_write_kernel(WidePresentEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimePresentEnc>(a, smem);
}

__global__ __launch_bounds__(ENC_BLOCK) void encode_wide_present_write_frames_kernel(WidePresentEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    encode_write_body<RuntimePresentEnc, WidePresentEncodeArgs, FRAME_HEAD>(a, smem);
}

template <class A, class SizeK>
static int launch_present_size(const A &a, SizeK size_kernel, hipStream_t stream) {
    if (a.nblocks) hipLaunchKernelGGL(size_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), 0, stream, a);
    if (a.frame_head)
        hipLaunchKernelGGL(encode_present_scan_frames_kernel, dim3(1), dim3(1024), 0, stream, a.block_sums, a.nblocks,
                           a.total, a.n);
    else
        hipLaunchKernelGGL(encode_present_scan_kernel, dim3(1), dim3(1024), 0, stream, a.block_sums, a.nblocks, a.total);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_encode_present_size(const PresentEncodeArgs &a, hipStream_t stream) {
    return launch_present_size(a, encode_present_size_kernel, stream);
}

int launch_encode_wide_present_size(const WidePresentEncodeArgs &a, hipStream_t stream) {
    return launch_present_size(a, encode_wide_present_size_kernel, stream);
}

int launch_encode_present_write(const PresentEncodeArgs &a, hipStream_t stream) {
    if (!a.nblocks) return 0;
    hipLaunchKernelGGL(a.frame_head ? encode_present_write_frames_kernel : encode_present_write_kernel,
                       dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), enc_write_lds_bytes(), stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_encode_wide_present_write(const WidePresentEncodeArgs &a, hipStream_t stream) {
    if (!a.nblocks) return 0;
    hipLaunchKernelGGL(a.frame_head ? encode_wide_present_write_frames_kernel : encode_wide_present_write_kernel,
                       dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), enc_write_lds_bytes(), stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_encode_wide_size(const WideEncodeArgs &a, hipStream_t stream) {
    if (a.nblocks) hipLaunchKernelGGL(encode_wide_size_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), 0, stream, a);
    if (a.frame_head) hipLaunchKernelGGL(encode_wide_scan_frames_kernel, dim3(1), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL(encode_wide_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_encode_wide_write(const WideEncodeArgs &a, hipStream_t stream) {
    if (!a.nblocks) return 0;
    if (a.frame_head)
        hipLaunchKernelGGL(encode_wide_write_frames_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK),
                           enc_write_lds_bytes(), stream, a);
    else
        hipLaunchKernelGGL(encode_wide_write_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), enc_write_lds_bytes(),
                           stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_encode_size(const spec_schema *schema, const EncodeArgs &a, hipStream_t stream) {
    int j = a.nblocks ? jit_launch_encode(schema, a, false, stream) : 1;
    if (j < 0) return -1;
    if (j == 0) hipLaunchKernelGGL(encode_size_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), 0, stream, a);
    if (a.frame_head) hipLaunchKernelGGL(encode_scan_frames_kernel, dim3(1), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL(encode_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_encode_write(const spec_schema *schema, const EncodeArgs &a, hipStream_t stream) {
    if (!a.nblocks) return 0;
    int j = jit_launch_encode(schema, a, true, stream);
    if (j < 0) return -1;
    if (j == 0 && a.frame_head)
        hipLaunchKernelGGL(encode_write_frames_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), enc_write_lds_bytes(),
                           stream, a);
    else if (j == 0)
        hipLaunchKernelGGL(encode_write_kernel, dim3((unsigned)a.nblocks), dim3(ENC_BLOCK), enc_write_lds_bytes(),
                           stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace spec

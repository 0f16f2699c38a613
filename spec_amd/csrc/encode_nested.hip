// encode_nested.hip — bulk encode of messages with a list<message> field (BASELINE config 4):
// the precompiled kernels (schema read from the kernel arguments, RuntimeEnc policies) and the
// launcher, which prefers the schema-specialised kernels of jit.cpp.  Device code and the
// algorithm: encode_nested_core.hpp.  Three launches, no host sync: sizes -> scan of block
// sums -> write.
// spec_encode_nested_frames (NestedEncodeArgs::frame_head = 4) runs the same three launches with
// the framed instantiations of the scan and the write pass: the unframed kernels do not change.
#include <hip/hip_runtime.h>

#include "encode_nested_core.hpp"
#include "spec_internal.hpp"

namespace spec {

namespace {

__global__ __launch_bounds__(NENC_BLOCK) void nested_enc_size_kernel(NestedEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    nested_enc_size_body<RuntimeEnc, RuntimeEnc>(a, smem);
}

__global__ __launch_bounds__(NENC_BLOCK) void nested_enc_write_kernel(NestedEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    nested_enc_write_body<RuntimeEnc, RuntimeEnc>(a, smem);
}

// the framed encoder: the head in front of every record (the shared scan, encode_flat.hip
// launch_encode_scan, adds 4 more bytes per record to every block sum)
__global__ __launch_bounds__(NENC_BLOCK) void nested_enc_write_frames_kernel(NestedEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    nested_enc_write_body<RuntimeEnc, RuntimeEnc, 4>(a, smem);
}

} // namespace

int launch_nested_encode(const spec_nested_schema *schema, const NestedEncodeArgs &a, bool write,
                         hipStream_t stream) {
    if (a.nblocks) {
        const int j = jit_launch_nested_encode(schema, a, false, stream);
        if (j < 0) return -1;
        if (j == 0)
            hipLaunchKernelGGL(nested_enc_size_kernel, dim3((unsigned)a.nblocks), dim3(NENC_BLOCK),
                               nenc_size_lds_bytes(), stream, a);
    }
    launch_encode_scan(a.block_sums, a.nblocks, a.total, a.n, a.frame_head, stream);
    if (write && a.nblocks) {
        const int j = jit_launch_nested_encode(schema, a, true, stream);
        if (j < 0) return -1;
        if (j == 0 && a.frame_head)
            hipLaunchKernelGGL(nested_enc_write_frames_kernel, dim3((unsigned)a.nblocks), dim3(NENC_BLOCK),
                               nenc_write_lds_bytes(), stream, a);
        else if (j == 0)
            hipLaunchKernelGGL(nested_enc_write_kernel, dim3((unsigned)a.nblocks), dim3(NENC_BLOCK),
                               nenc_write_lds_bytes(), stream, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace spec

// decode_flat.hip — the precompiled (run-time schema) decode kernels and their launcher.
// The device code lives in decode_core.hpp; schema-specialised variants of the same body
// are compiled at run time by jit.cpp.
#include <hip/hip_runtime.h>

#include "decode_core.hpp"
#include "spec_internal.hpp"

namespace spec {

__global__ __launch_bounds__(256) void decode_flat_kernel(DecodeArgs a) { decode_flat_runtime(a); }

// spec_decode_flat_present / spec_decode_frames_present on a run-time schema: the same body with
// the HasField masks (a.f.present)
__global__ __launch_bounds__(256) void decode_flat_present_kernel(DecodeArgs a) {
    decode_flat_runtime<true>(a);
}

int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cus[dev] = v;
    }
    return cus[dev];
}

int launch_decode_flat(DecodeArgs a, double avg_record, hipStream_t stream) {
    if (a.n <= a.r0) return 0;
    const DecodeLaunch L = decode_launch(a.n - a.r0, avg_record);
    a.slab = L.slab;
    a.xcd = 1; // XCD-aware contiguous shares of the groups (decode_core.hpp flat_block)
    if (a.f.present) hipLaunchKernelGGL(decode_flat_present_kernel, dim3(L.blocks), dim3(64), L.slab, stream, a);
    else hipLaunchKernelGGL(decode_flat_kernel, dim3(L.blocks), dim3(64), L.slab, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace spec

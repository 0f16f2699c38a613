// frames_write.hip — spec_frames_write: the mpx frame writer on the device (mpx/conn_writer.go:
// 84-97: every message goes out as `[u32 big-endian size][message]`).  Record k of a batch
// ([ends[k-1], ends[k]) of the stream) lands at ends[k-1] + 4k of the output with its head in
// front: a copy whose shift grows by 4 with every record.
//
// One wave takes a group of 64 consecutive records:
//   * the group's source span is staged into LDS with the primitive every decode kernel uses
//     (decode_core.hpp stage_span: LDS-DMA, 1 KiB per instruction);
//   * the group's output range is assembled in a second LDS image whose origin is the 16-byte
//     granule of the OUTPUT ADDRESS that holds the range's first byte: lane k writes head k and
//     copies record k in destination-aligned dwords (two source dwords and a funnel shift: the
//     source / destination phase differs per record); records over 1 KiB go wave-wide instead;
//   * the image goes out in 16-byte stores; the first and last granule, which the neighbouring
//     groups share, bytewise and only inside the group's own range.
// A group whose span does not fit its slab (or its image) is copied record by record from HBM to
// HBM.  A group with malformed ends (decreasing, or past the stream) writes nothing.
#include <hip/hip_runtime.h>

#include "spec_internal.hpp"

namespace spec {

namespace {

constexpr uint32_t FW_CHUNKS = 18;                   // 1 KiB chunks of the source slab
constexpr uint32_t FW_SRC = FW_CHUNKS * 1024 + 16;   // + the dword read past a record's last byte
constexpr uint32_t FW_IMG = FW_CHUNKS * 1024 + 256 + 16; // the span, 64 heads, the origin's phase
constexpr uint32_t FW_LANE = 1024;                   // records up to this are copied by their own lane

struct FwArgs {
    const uint8_t *stream;
    uint64_t stream_len;
    const uint64_t *ends;
    uint64_t n;
    uint8_t *frames;
    uint64_t *frame_ends;
};

__device__ __forceinline__ uint32_t lds_dword_at(const uint8_t *l, uint32_t o) { // any byte offset
    const uint32_t *w = (const uint32_t *)l;
    return __builtin_amdgcn_alignbyte(w[(o >> 2) + 1], w[o >> 2], o & 3);
}

__global__ __launch_bounds__(64) void frames_write_kernel(FwArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t slab[FW_SRC];
    __shared__ __attribute__((aligned(16))) uint8_t img[FW_IMG];
    const int lane = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * 64;
    const uint32_t cnt = (uint32_t)(a.n - base < 64 ? a.n - base : 64);
    const uint64_t r = base + lane;
    const bool valid = (uint32_t)lane < cnt;
    const uint64_t hi = a.ends[valid ? r : a.n - 1];
    uint64_t lo = __shfl_up(hi, 1);
    if (lane == 0) lo = base == 0 ? 0 : a.ends[base - 1];
    if (__ballot(valid && (hi < lo || hi > a.stream_len))) return; // malformed ends: nothing written
    if (!valid) lo = hi;
    const uint64_t fstart = lo + 4 * r; // this record's head in the output
    if (valid && a.frame_ends) a.frame_ends[r] = hi + 4 * (r + 1);
    const uint64_t span_lo = uniform64(__shfl(lo, 0)), span_hi = uniform64(__shfl(hi, (int)cnt - 1));
    const uint64_t out_lo = span_lo + 4 * base, out_hi = span_hi + 4 * (base + cnt);
    const uint32_t size = (uint32_t)(hi - lo);
    const uint32_t phase = (uint32_t)(((uintptr_t)a.frames + out_lo) & 15); // out_lo's place in its granule
    const Staged st = stage_plan(span_lo, span_hi);
    const bool in_lds = st.bytes() + 16 <= FW_SRC && phase + (out_hi - out_lo) <= FW_IMG;

    if (!in_lds) { // HBM to HBM, a record at a time
        if (valid)
            for (uint32_t b = 0; b < 4; b++) a.frames[fstart + b] = (uint8_t)(size >> (8 * (3 - b)));
        for (uint32_t k = 0; k < cnt; k++) {
            const uint64_t s = uniform64(__shfl(lo, (int)k)), d = uniform64(__shfl(fstart, (int)k)) + 4;
            const uint32_t len = __builtin_amdgcn_readfirstlane((uint32_t)__shfl((int)size, (int)k));
            for (uint32_t i = lane; i < len; i += 64) a.frames[d + i] = a.stream[s + i];
        }
        return;
    }

    const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(a.stream, a.stream_len);
    stage_span<STREAM_AUX>(rsrc, slab, st, a.stream_len, lane);
    // image byte j is output byte out_lo - phase + j
    const uint32_t my_dst = (uint32_t)(fstart - out_lo) + phase, my_src = (uint32_t)(lo - st.origin);
    if (valid)
        for (uint32_t b = 0; b < 4; b++) img[my_dst + b] = (uint8_t)(size >> (8 * (3 - b)));
    // Records up to FW_LANE bytes: every lane copies its own, all in lockstep over the longest —
    // bytes up to the destination's dword boundary, whole destination dwords four at a time
    // (their loads issued before the stores wait), the last bytes.  (A wave-wide pass per record
    // measured 0.36 ms on 1M Flat16 records: 64 passes of three dependent LDS round trips.)
    {
        const bool small = valid && size <= FW_LANE;
        const uint32_t s = my_src, d = my_dst + 4, len = small ? size : 0;
        uint32_t first = (4 - (d & 3)) & 3;
        if (first > len) first = len;
        const uint32_t nd = (len - first) >> 2, done = first + 4 * nd;
        for (uint32_t b = 0; b < 3; b++)
            if (b < first) img[d + b] = slab[s + b];
        for (uint32_t i = 0; __ballot(i < nd); i += 4) {
            uint32_t v[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; t++)
                if (i + t < nd) v[t] = lds_dword_at(slab, s + first + 4 * (i + t));
#pragma unroll
            for (uint32_t t = 0; t < 4; t++)
                if (i + t < nd) *(uint32_t *)(img + d + first + 4 * (i + t)) = v[t];
        }
        for (uint32_t b = 0; b < 3; b++)
            if (done + b < len) img[d + done + b] = slab[s + done + b];
    }
    // longer records: one after the other, wave-wide
    uint64_t longs = __ballot(valid && size > FW_LANE);
    while (longs) {
        const int k = __builtin_ctzll(longs);
        longs &= longs - 1;
        const uint32_t s = __builtin_amdgcn_readlane(my_src, k), d = __builtin_amdgcn_readlane(my_dst, k) + 4;
        const uint32_t len = __builtin_amdgcn_readlane(size, k);
        const uint32_t first = (4 - (d & 3)) & 3; // (len > FW_LANE)
        const uint32_t nd = (len - first) >> 2, done = first + 4 * nd;
        if ((uint32_t)lane < first) img[d + lane] = slab[s + lane];
        for (uint32_t i = lane; i < nd; i += 64)
            *(uint32_t *)(img + d + first + 4 * i) = lds_dword_at(slab, s + first + 4 * i);
        if ((uint32_t)lane < len - done) img[d + done + lane] = slab[s + done + lane];
    }
    __syncthreads();
    // the image's granules: whole ones as 16-byte stores, the range's two ends bytewise
    const uint32_t end = phase + (uint32_t)(out_hi - out_lo);
    uint8_t *g0 = a.frames + out_lo - phase; // 16-byte aligned (never dereferenced below out_lo)
    for (uint32_t j = 16 * lane; j < end; j += 1024) {
        if (j >= phase && j + 16 <= end) {
            *(uint4 *)(g0 + j) = *(const uint4 *)(img + j);
        } else {
            for (uint32_t t = 0; t < 16; t++)
                if (j + t >= phase && j + t < end) g0[j + t] = img[j + t];
        }
    }
}

} // namespace

int launch_frames_write(const uint8_t *stream_bytes, uint64_t stream_len, const uint64_t *ends, uint64_t n,
                        uint8_t *frames, uint64_t *frame_ends, hipStream_t stream) {
    FwArgs a = {stream_bytes, stream_len, ends, n, frames, frame_ends};
    hipLaunchKernelGGL(frames_write_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace spec

// test_build_frames.cpp — MessageBatchWriter::BuildFrames (include/spec_amd.hpp) on the GPU: the
// mpx frames [u32 BE size][message] of the oracle Writer's records (mpx/conn_writer.go:84-97),
// equal to WriteFrames(Build()), and an encoder error thrown as Build throws it.
// Built and run by tests/test_gpu_cpp_frames.py.  Exit 0 = all pass.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "spec_amd.hpp"
#include "spec_oracle.h"

namespace {

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) throw std::runtime_error(std::string(__FILE__ ":") + std::to_string(__LINE__) + ": " #cond); \
    } while (0)

const uint16_t kTags[5] = {1, 2, 5, 9, 12};
const uint8_t kKinds[5] = {SPEC_KIND_INT64, SPEC_KIND_STRING, SPEC_KIND_FLOAT64, SPEC_KIND_BOOL, SPEC_KIND_UINT32};

struct HostRecords {
    uint64_t n;
    std::vector<int64_t> i64;
    std::vector<uint32_t> str; // {off, len}
    std::vector<double> f64;
    std::vector<uint8_t> b;
    std::vector<uint32_t> u32;
    std::vector<uint8_t> heap;
    std::vector<uint8_t> frames; // [u32 BE size][record] of the oracle's records
    std::vector<uint64_t> frame_ends;
};

HostRecords test_records(uint64_t n) {
    HostRecords h;
    h.n = n;
    uint64_t x = 4242;
    for (uint64_t i = 0; i < n; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        h.i64.push_back((int64_t)x >> (x & 63));
        uint32_t len = (uint32_t)(x >> 57);
        h.str.push_back((uint32_t)h.heap.size());
        h.str.push_back(len);
        for (uint32_t k = 0; k < len; k++) h.heap.push_back((uint8_t)('a' + (x >> (k & 31)) % 26));
        h.f64.push_back((double)(int64_t)x * 1e-3);
        h.b.push_back((x >> 9) & 1);
        h.u32.push_back((uint32_t)(x >> 17));
    }
    const void *cols[5] = {h.i64.data(), h.str.data(), h.f64.data(), h.b.data(), h.u32.data()};
    const uint8_t *heaps[5] = {nullptr, h.heap.data(), nullptr, nullptr, nullptr};
    std::vector<uint8_t> stream(n * 128 + h.heap.size() + 16);
    std::vector<uint64_t> ends(n);
    if (so_encode_flat_batch(5, kTags, kKinds, cols, heaps, n, stream.data(), stream.size(), ends.data()))
        throw std::runtime_error("oracle encode");
    uint64_t start = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t size = (uint32_t)(ends[i] - start);
        for (int k = 3; k >= 0; k--) h.frames.push_back((uint8_t)(size >> (8 * k)));
        h.frames.insert(h.frames.end(), stream.begin() + start, stream.begin() + ends[i]);
        h.frame_ends.push_back(h.frames.size());
        start = ends[i];
    }
    return h;
}

void should_write_frames_like_conn_writer() {
    spec::Stream s;
    HostRecords h = test_records(7001);
    spec::Schema schema;
    for (int f = 0; f < 5; f++) schema.Field(kTags[f], (spec::Kind)kKinds[f]);
    auto c0 = spec::DeviceBuffer::From(h.i64, s), c1 = spec::DeviceBuffer::From(h.str, s),
         c2 = spec::DeviceBuffer::From(h.f64, s), c3 = spec::DeviceBuffer::From(h.b, s),
         c4 = spec::DeviceBuffer::From(h.u32, s), heap = spec::DeviceBuffer::From(h.heap, s);
    spec::MessageBatchWriter w(schema, h.n);
    w.Field(0, c0).Field(1, c1, &heap).Field(2, c2).Field(3, c3).Field(4, c4);
    spec::Frames f = w.BuildFrames(s);
    REQUIRE(f.n == h.n && f.len == h.frames.size());
    auto out = f.bytes.ToHost<uint8_t>(s);
    auto ends = f.ends.ToHost<uint64_t>(s);
    REQUIRE(std::memcmp(out.data(), h.frames.data(), f.len) == 0);
    REQUIRE(std::memcmp(ends.data(), h.frame_ends.data(), h.n * 8) == 0);
    // the two-pass send path gives the same frames
    spec::Frames two = spec::WriteFrames(w.Build(s), s);
    auto out2 = two.bytes.ToHost<uint8_t>(s);
    auto ends2 = two.ends.ToHost<uint64_t>(s);
    REQUIRE(two.len == f.len && std::memcmp(out2.data(), out.data(), f.len) == 0);
    REQUIRE(std::memcmp(ends2.data(), ends.data(), h.n * 8) == 0);
    // a span outside its heap: thrown, as Build throws it
    h.str[2 * 17] = (uint32_t)h.heap.size();
    h.str[2 * 17 + 1] = 5;
    auto bad = spec::DeviceBuffer::From(h.str, s);
    w.Field(1, bad, &heap);
    bool thrown = false;
    try {
        w.BuildFrames(s);
    } catch (const spec::Error &e) {
        thrown = e.rc == SPEC_E_INVALID_ARGUMENT;
    }
    REQUIRE(thrown);
}

} // namespace

int main() {
    try {
        should_write_frames_like_conn_writer();
    } catch (const std::exception &e) {
        std::printf("FAIL BuildFrames: %s\n1 tests, 1 failed\n", e.what());
        return 1;
    }
    std::printf("PASS BuildFrames\n1 tests, 0 failed\n");
    return 0;
}

// test_present.cpp — optional fields through the C++ host API (include/spec_amd.hpp) on the GPU:
// MessageBatchWriter::SetPresent writes only the fields of each record's mask, OpenMessageBatch /
// OpenMessageFrames with present = true give the masks back (MessageBatch::Present, the generated
// HasX() of every field), a present field its value and an absent one zero.
// Built and run by tests/test_gpu_cpp_present.py.  Exit 0 = all pass.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "spec_amd.hpp"

namespace {

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) throw std::runtime_error(std::string(__FILE__ ":") + std::to_string(__LINE__) + ": " #cond); \
    } while (0)

const uint16_t kTags[5] = {1, 2, 5, 9, 12};
const spec::Kind kKinds[5] = {spec::Kind::Int64, spec::Kind::String, spec::Kind::Float64, spec::Kind::Bool,
                              spec::Kind::Uint32};

void check(const spec::MessageBatch &m, const std::vector<uint64_t> &mask, const std::vector<int64_t> &i64,
           const std::vector<uint32_t> &u32, const std::vector<uint32_t> &str, spec::Stream &s) {
    const uint64_t n = mask.size();
    auto got = m.Present().ToHost<uint64_t>(s);
    auto st = m.Status().ToHost<uint8_t>(s);
    auto g0 = m.Get<int64_t>(0, s);
    auto g1 = m.Get<uint32_t>(1, s);
    auto g4 = m.Get<uint32_t>(4, s);
    for (uint64_t i = 0; i < n; i++) {
        REQUIRE(st[i] == 0);
        REQUIRE(got[i] == mask[i]);
        REQUIRE(g0[i] == ((mask[i] & 1) ? i64[i] : 0));
        REQUIRE(g4[i] == ((mask[i] & 16) ? u32[i] : 0u));
        REQUIRE(g1[2 * i + 1] == ((mask[i] & 2) ? str[2 * i + 1] : 0u)); // the string's length
    }
}

void should_round_trip_masks() {
    spec::Stream s;
    const uint64_t n = 130;
    std::vector<int64_t> i64;
    std::vector<uint32_t> str, u32;
    std::vector<double> f64;
    std::vector<uint8_t> b, heap;
    std::vector<uint64_t> mask;
    uint64_t x = 99;
    for (uint64_t i = 0; i < n; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        i64.push_back((int64_t)x >> (x & 63));
        const uint32_t len = (uint32_t)(x >> 58);
        str.push_back((uint32_t)heap.size());
        str.push_back(len);
        for (uint32_t k = 0; k < len; k++) heap.push_back((uint8_t)('a' + (x >> (k & 31)) % 26));
        f64.push_back((double)(int64_t)x * 1e-3);
        b.push_back((x >> 9) & 1);
        u32.push_back((uint32_t)(x >> 17));
        mask.push_back((x >> 33) & 31); // every field with p = 0.5
    }
    mask[0] = 0;   // no field written: 00 00 50
    mask[64] = 31; // every field
    spec::Schema schema;
    for (int f = 0; f < 5; f++) schema.Field(kTags[f], kKinds[f]);
    auto c0 = spec::DeviceBuffer::From(i64, s), c1 = spec::DeviceBuffer::From(str, s),
         c2 = spec::DeviceBuffer::From(f64, s), c3 = spec::DeviceBuffer::From(b, s),
         c4 = spec::DeviceBuffer::From(u32, s), hp = spec::DeviceBuffer::From(heap, s),
         pm = spec::DeviceBuffer::From(mask, s);
    spec::MessageBatchWriter w(schema, n);
    w.Field(0, c0).Field(1, c1, &hp).Field(2, c2).Field(3, c3).Field(4, c4).SetPresent(pm);
    spec::Batch batch = w.Build(s);
    REQUIRE(batch.n == n);
    auto ends = batch.ends.ToHost<uint64_t>(s);
    REQUIRE(ends[0] == 3); // record 0 is the empty message
    auto bytes = batch.stream.ToHost<uint8_t>(s);
    REQUIRE(bytes[0] == 0 && bytes[1] == 0 && bytes[2] == 80);
    check(spec::OpenMessageBatch(schema, batch, s, true), mask, i64, u32, str, s);
    REQUIRE(spec::OpenMessageBatch(schema, batch, s).Present().size() == 0);

    spec::Frames frames = w.BuildFrames(s);
    REQUIRE(frames.n == n && frames.len == batch.len + 4 * n);
    check(spec::OpenMessageFrames(schema, frames, s, true), mask, i64, u32, str, s);
}

} // namespace

int main() {
    try {
        should_round_trip_masks();
    } catch (const std::exception &e) {
        std::printf("FAIL Present: %s\n1 tests, 1 failed\n", e.what());
        return 1;
    }
    std::printf("PASS Present\n1 tests, 0 failed\n");
    return 0;
}

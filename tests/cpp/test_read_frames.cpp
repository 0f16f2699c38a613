// test_read_frames.cpp — the receive side of the C++ host API over mpx frames (include/spec_amd.hpp):
// spec::OpenMessageFrames decodes the frames of a batch where they lie to the columns that went in
// (and to OpenMessageBatch's over the unframed records, spans 4(k + 1) further on), and
// HostMessageReader::ReadFrames gives Read's chunk-major output over the unframed batch
// (mpx/conn_reader.go:179-194).  Built and run by tests/test_gpu_cpp_read_frames.py.  Exit 0 = all pass.
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
    std::vector<uint8_t> stream; // the oracle's records, and their frames [u32 BE size][record]
    std::vector<uint64_t> ends;
    std::vector<uint8_t> frames;
    std::vector<uint64_t> frame_ends;
};

HostRecords test_records(uint64_t n) {
    HostRecords h;
    h.n = n;
    uint64_t x = 777;
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
    h.stream.resize(n * 128 + h.heap.size() + 16);
    h.ends.resize(n);
    if (so_encode_flat_batch(5, kTags, kKinds, cols, heaps, n, h.stream.data(), h.stream.size(), h.ends.data()))
        throw std::runtime_error("oracle encode");
    h.stream.resize(n ? h.ends[n - 1] : 0);
    uint64_t start = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t size = (uint32_t)(h.ends[i] - start);
        for (int k = 3; k >= 0; k--) h.frames.push_back((uint8_t)(size >> (8 * k)));
        h.frames.insert(h.frames.end(), h.stream.begin() + start, h.stream.begin() + h.ends[i]);
        h.frame_ends.push_back(h.frames.size());
        start = h.ends[i];
    }
    return h;
}

spec::Schema test_schema() {
    spec::Schema schema;
    for (int f = 0; f < 5; f++) schema.Field(kTags[f], (spec::Kind)kKinds[f]);
    return schema;
}

// the string spans of the framed decode: the unframed ones 4(k + 1) further on, the same bytes
void require_spans(const std::vector<uint32_t> &got, const std::vector<uint32_t> &plain, const HostRecords &h,
                   uint64_t r0, uint64_t r1) {
    for (uint64_t k = r0; k < r1; k++) {
        const uint32_t go = got[2 * (k - r0)], gl = got[2 * (k - r0) + 1];
        const uint32_t po = plain[2 * (k - r0)], pl = plain[2 * (k - r0) + 1];
        REQUIRE(gl == pl && gl == h.str[2 * k + 1]);
        if (!gl) continue;
        REQUIRE(go == po + 4 * (k + 1));
        REQUIRE(std::memcmp(h.frames.data() + go, h.heap.data() + h.str[2 * k], gl) == 0);
    }
}

void should_open_frames_in_place() {
    spec::Stream s;
    HostRecords h = test_records(7001);
    spec::Schema schema = test_schema();
    spec::Frames f;
    f.bytes = spec::DeviceBuffer::From(h.frames, s);
    f.ends = spec::DeviceBuffer::From(h.frame_ends, s);
    f.len = h.frames.size();
    f.n = h.n;
    spec::Batch b;
    b.stream = spec::DeviceBuffer::From(h.stream, s);
    b.ends = spec::DeviceBuffer::From(h.ends, s);
    b.len = h.stream.size();
    b.n = h.n;
    spec::MessageBatch m = spec::OpenMessageFrames(schema, f, s), p = spec::OpenMessageBatch(schema, b, s);
    REQUIRE(m.Len() == h.n);
    auto st = m.Status().ToHost<uint8_t>(s);
    for (uint64_t i = 0; i < h.n; i++) REQUIRE(st[i] == 0);
    REQUIRE(std::memcmp(m.Get<int64_t>(0, s).data(), h.i64.data(), h.n * 8) == 0);
    REQUIRE(std::memcmp(m.Get<double>(2, s).data(), h.f64.data(), h.n * 8) == 0);
    REQUIRE(std::memcmp(m.Get<uint8_t>(3, s).data(), h.b.data(), h.n) == 0);
    REQUIRE(std::memcmp(m.Get<uint32_t>(4, s).data(), h.u32.data(), h.n * 4) == 0);
    require_spans(m.Get<uint32_t>(1, s), p.Get<uint32_t>(1, s), h, 0, h.n);
    // the frames a writer built on the device decode the same way
    auto c0 = spec::DeviceBuffer::From(h.i64, s), c1 = spec::DeviceBuffer::From(h.str, s),
         c2 = spec::DeviceBuffer::From(h.f64, s), c3 = spec::DeviceBuffer::From(h.b, s),
         c4 = spec::DeviceBuffer::From(h.u32, s), heap = spec::DeviceBuffer::From(h.heap, s);
    spec::MessageBatchWriter w(schema, h.n);
    w.Field(0, c0).Field(1, c1, &heap).Field(2, c2).Field(3, c3).Field(4, c4);
    spec::MessageBatch m2 = spec::OpenMessageFrames(schema, w.BuildFrames(s), s);
    REQUIRE(std::memcmp(m2.Get<int64_t>(0, s).data(), h.i64.data(), h.n * 8) == 0);
    REQUIRE(std::memcmp(m2.Get<uint32_t>(1, s).data(), m.Get<uint32_t>(1, s).data(), h.n * 8) == 0);
}

void should_read_frames_from_host_memory() {
    HostRecords h = test_records(3000);
    spec::Schema schema = test_schema();
    spec::HostMessageReader r(schema, h.n, h.frames.size(), 3);
    spec::PinnedBuffer frames(h.frames.size()), fends(h.n * 8), stream(h.stream.size()), ends(h.n * 8);
    std::memcpy(frames.data(), h.frames.data(), h.frames.size());
    std::memcpy(fends.data(), h.frame_ends.data(), h.n * 8);
    std::memcpy(stream.data(), h.stream.data(), h.stream.size());
    std::memcpy(ends.data(), h.ends.data(), h.n * 8);
    spec::PinnedBuffer out(r.OutBytes(h.n)), plain(r.OutBytes(h.n));
    r.Read(stream, h.stream.size(), ends, h.n, plain);
    r.ReadFrames(frames, h.frames.size(), fends, h.n, out);
    for (uint32_t k = 0; k < r.Chunks(); k++) {
        const auto v = r.Chunk(h.n, k);
        const uint64_t nk = v.r1 - v.r0;
        for (size_t f = 0; f < schema.Len(); f++) {
            const size_t bytes = nk * spec::Width(schema.KindOf(f));
            if (schema.KindOf(f) == spec::Kind::String) {
                std::vector<uint32_t> g(2 * nk), p(2 * nk);
                std::memcpy(g.data(), out.data() + v.col_off[f], bytes);
                std::memcpy(p.data(), plain.data() + v.col_off[f], bytes);
                require_spans(g, p, h, v.r0, v.r1);
            } else {
                REQUIRE(std::memcmp(out.data() + v.col_off[f], plain.data() + v.col_off[f], bytes) == 0);
            }
        }
        REQUIRE(std::memcmp(out.data() + v.status_off, plain.data() + v.status_off, nk) == 0);
        REQUIRE(std::memcmp(out.data() + v.col_off[0], h.i64.data() + v.r0, nk * 8) == 0);
    }
    // frame ends that pass the buffer: refused
    ((uint64_t *)fends.data())[h.n - 1] = h.frames.size() + 1;
    bool thrown = false;
    try {
        r.ReadFrames(frames, h.frames.size(), fends, h.n, out);
    } catch (const spec::Error &e) {
        thrown = e.rc == SPEC_E_INVALID_ARGUMENT;
    }
    REQUIRE(thrown);
}

} // namespace

int main() {
    struct {
        const char *name;
        void (*fn)();
    } tests[] = {{"OpenMessageFrames", should_open_frames_in_place}, {"ReadFrames", should_read_frames_from_host_memory}};
    int failed = 0;
    for (auto &t : tests) {
        try {
            t.fn();
            std::printf("PASS %s\n", t.name);
        } catch (const std::exception &e) {
            std::printf("FAIL %s: %s\n", t.name, e.what());
            failed++;
        }
    }
    std::printf("2 tests, %d failed\n", failed);
    return failed ? 1 : 0;
}

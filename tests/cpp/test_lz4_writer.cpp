// test_lz4_writer.cpp — spec::Lz4FrameWriter (include/spec_amd.hpp) on the GPU: three Writes and
// a Close give one LZ4 frame (mpx/conn_writer.go:42-56) that the oracle's reader (oracle/lz4.c)
// accepts, content checksum included, and decompresses to what was written.
// Built and run by tests/test_gpu_cpp_lz4_writer.py.  Exit 0 = all pass.
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

void append(std::vector<uint8_t> &wire, const spec::Lz4Segment &seg, spec::Stream &s) {
    const uint64_t n = seg.Size(s);
    REQUIRE(n + 1 <= seg.bytes.size());
    std::vector<uint8_t> host(n);
    if (n) seg.bytes.CopyTo(host.data(), n, s);
    s.Sync();
    wire.insert(wire.end(), host.begin(), host.end());
}

void should_write_one_frame_over_several_writes() {
    spec::Stream s;
    std::vector<uint8_t> data(700001);
    uint64_t x = 99;
    for (size_t i = 0; i < data.size(); i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        data[i] = i < 300000 ? (uint8_t)("field table trailer "[i % 20]) : i < 500000 ? (uint8_t)(x >> 56) : (uint8_t)((x >> 60) + 'a');
    }
    auto d = spec::DeviceBuffer::From(data, s);
    spec::Lz4FrameWriter w(s, 256u << 10, true);
    const size_t cuts[4] = {0, 1, 400000, data.size()};
    std::vector<uint8_t> wire;
    for (int i = 0; i < 3; i++)
        append(wire, w.Write((const uint8_t *)d.data() + cuts[i], cuts[i + 1] - cuts[i], s), s);
    append(wire, w.Close(s), s);
    REQUIRE(wire.size() < data.size()); // two thirds of it compress
    std::vector<uint8_t> back(data.size() + 16);
    size_t out_len = 0, consumed = 0;
    REQUIRE(so_lz4_frame_read(wire.data(), wire.size(), back.data(), back.size(), &out_len, &consumed) == 0);
    REQUIRE(consumed == wire.size() && out_len == data.size());
    REQUIRE(std::memcmp(back.data(), data.data(), data.size()) == 0);
    wire[wire.size() - 1] ^= 0x10; // the stored content checksum
    REQUIRE(so_lz4_frame_read(wire.data(), wire.size(), back.data(), back.size(), &out_len, &consumed) == -6);
}

} // namespace

int main() {
    try {
        should_write_one_frame_over_several_writes();
    } catch (const std::exception &e) {
        std::printf("FAIL Lz4FrameWriter: %s\n1 tests, 1 failed\n", e.what());
        return 1;
    }
    std::printf("PASS Lz4FrameWriter\n1 tests, 0 failed\n");
    return 0;
}

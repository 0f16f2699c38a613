// jit_module.cpp — hiprtc, the on-disk code-object cache and the loaded modules behind the
// schema-specialised kernels (jit.cpp: flat and nested; jit_tree.cpp: schema trees).
#include "jit_module.hpp"

#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>
#include <utime.h>
#include <unistd.h>

#include <atomic>
#include <mutex>
#include <unordered_map>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace spec {
namespace jit {
namespace {

// the device sources, embedded at build time (Makefile -> build/rtc_sources.inc), by the names
// the generated sources include them under; in this order they are hashed (source_hash)
#include "build/rtc_sources.inc"
const struct { const char *name, *src; } kHeaders[] = {
    {"spec_device.hpp", kSpecDeviceHpp},          {"decode_core.hpp", kDecodeCoreHpp},
    {"encode_core.hpp", kEncodeCoreHpp},          {"decode_nested_core.hpp", kDecodeNestedCoreHpp},
    {"encode_nested_core.hpp", kEncodeNestedCoreHpp}, {"tree_core.hpp", kTreeCoreHpp},
    {"tree_decode_core.hpp", kTreeDecodeCoreHpp}};
constexpr int NHDR = sizeof kHeaders / sizeof kHeaders[0];

// by Prog: the hiprtc program name, the SPEC_AMD_JIT_DUMP file stem
const struct { const char *name, *stem; } kProgs[] = {
    {"spec_decode_flat_jit.hip", "decode"},          {"spec_encode_jit.hip", "encode"},
    {"spec_decode_nested_jit.hip", "nested"},        {"spec_encode_nested_jit.hip", "nested_encode"},
    {"spec_tree_jit.hip", "tree"}};

// the product kernels are compiled with fixed options only: no environment variable can change
// what a kernel computes
const char *const kOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
constexpr int NOPTS = sizeof kOpts / sizeof kOpts[0];

struct Remembered { // remember_module
    int device;
    std::vector<char> desc;
    const Module *m;
};

std::mutex g_mu; // the two below
std::unordered_map<std::string, Module> g_cache;
std::vector<Remembered> g_remembered;
std::atomic<int> g_enabled{-1}; // -1: read SPEC_AMD_JIT on first use

bool debug() {
    const char *e = getenv("SPEC_AMD_DEBUG");
    return e && e[0] && e[0] != '0';
}

// SPEC_AMD_JIT_DUMP=prefix: the generated source is written to <prefix><program>.hip before the
// compile (a slow compile can be inspected while it runs), the code object to <prefix><program>.co
// after it (ISA inspection)
void dump(Prog p, const char *ext, const char *data, size_t n) {
    const char *d = getenv("SPEC_AMD_JIT_DUMP");
    if (!d) return;
    if (FILE *f = fopen((std::string(d) + kProgs[p].stem + ext).c_str(), "wb")) {
        fwrite(data, 1, n, f);
        fclose(f);
    }
}

// hiprtc compile only; returns the code object (empty on failure)
std::vector<char> compile_uncached(const std::string &src, Prog p) {
    dump(p, ".hip", src.data(), src.size());
    const char *hdr_src[NHDR], *hdr_name[NHDR];
    for (int i = 0; i < NHDR; i++) hdr_src[i] = kHeaders[i].src, hdr_name[i] = kHeaders[i].name;
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), kProgs[p].name, NHDR, hdr_src, hdr_name) != HIPRTC_SUCCESS) return {};
    hiprtcResult rc = hiprtcCompileProgram(prog, NOPTS, (const char **)kOpts);
    if (rc != HIPRTC_SUCCESS || debug()) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        if (ls > 1) {
            std::vector<char> log(ls + 1, 0);
            hiprtcGetProgramLog(prog, log.data());
            fprintf(stderr, "spec_amd jit: %s\n", log.data());
        }
    }
    if (rc != HIPRTC_SUCCESS) {
        fprintf(stderr, "spec_amd jit: hiprtc compile of %s failed; the generic kernel is used\n", kProgs[p].name);
        hiprtcDestroyProgram(&prog);
        return {};
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    std::vector<char> code(cs);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    dump(p, ".co", code.data(), code.size());
    return code;
}

// ---- on-disk code-object cache -----------------------------------------------------------
// A compile costs ~3 s per (schema, kernel set); its result depends only on the generated
// source, the embedded headers and the options, so it is cached under <libdir>/jit_cache
// (next to libspec_amd.so: build() fills it for the benchmark schemas, and it travels with the
// library) or, where that is not writable, $XDG_CACHE_HOME/spec_amd or ~/.cache/spec_amd.
uint64_t fnv1a(uint64_t h, const char *p, size_t n) {
    for (size_t i = 0; i < n; i++) h = (h ^ (uint8_t)p[i]) * 0x100000001b3ull;
    return h;
}

std::string lib_dir() {
    Dl_info info;
    if (dladdr((void *)&fnv1a, &info) && info.dli_fname) {
        std::string f = info.dli_fname;
        size_t k = f.rfind('/');
        return k == std::string::npos ? std::string(".") : f.substr(0, k);
    }
    return ".";
}

std::vector<std::string> cache_dirs() {
    std::vector<std::string> v = {lib_dir() + "/jit_cache"};
    if (const char *x = getenv("XDG_CACHE_HOME")) v.push_back(std::string(x) + "/spec_amd");
    else if (const char *h = getenv("HOME")) v.push_back(std::string(h) + "/.cache/spec_amd");
    return v;
}

bool read_file(const std::string &path, std::vector<char> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    bool ok = n > 0 && fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

void write_cache(const std::string &name, const std::vector<char> &code) {
    for (const std::string &d : cache_dirs()) {
        mkdir(d.c_str(), 0755); // best effort; a missing parent makes the open below fail
        static std::atomic<unsigned> seq{0}; // concurrent compiles (threads) of one process
        const std::string tmp = d + "/." + name + "." + std::to_string(getpid()) + "." + std::to_string(seq++);
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f) continue;
        bool ok = fwrite(code.data(), 1, code.size(), f) == code.size();
        ok = (fclose(f) == 0) && ok;
        if (ok && rename(tmp.c_str(), (d + "/" + name).c_str()) == 0) return;
        unlink(tmp.c_str());
    }
}

} // namespace

bool enabled() {
    int on = g_enabled.load(std::memory_order_relaxed);
    if (on < 0) {
        const char *e = getenv("SPEC_AMD_JIT");
        int unread = -1; // (a jit_set_enabled in between wins)
        on = (e && e[0] == '0') ? 0 : 1;
        if (!g_enabled.compare_exchange_strong(unread, on)) on = unread;
    }
    return on == 1;
}

uint64_t source_hash(const std::string &src) {
    uint64_t h = fnv1a(0xcbf29ce484222325ull, src.data(), src.size());
    for (const auto &hd : kHeaders) h = fnv1a(h, hd.src, strlen(hd.src) + 1);
    for (const char *o : kOpts) h = fnv1a(h, o, strlen(o) + 1);
    return h;
}

std::vector<char> compile_source(const std::string &src, Prog p) {
    char name[64];
    snprintf(name, sizeof name, "%016llx.co", (unsigned long long)source_hash(src));
    std::vector<char> cached;
    const bool dump = getenv("SPEC_AMD_JIT_DUMP") != nullptr; // diagnostic: always compile (and dump)
    for (const std::string &d : cache_dirs())
        if (!dump && read_file(d + "/" + name, cached)) {
            utime((d + "/" + name).c_str(), nullptr); // in use: build() prunes entries it did not touch
            return cached;
        }
    std::vector<char> code = compile_uncached(src, p);
    if (!code.empty()) write_cache(name, code);
    return code;
}

Module load_module(const std::vector<char> &code, const std::vector<Kernel> &kernels) {
    Module m;
    bool ok = !code.empty() && hipModuleLoadData(&m.mod, code.data()) == hipSuccess;
    bool some = false, all = true;
    for (size_t i = 0; ok && i < kernels.size(); i++) {
        const Kernel &k = kernels[i];
        const bool got = hipModuleGetFunction(&m.fn[k.fn], m.mod, k.name.c_str()) == hipSuccess;
        if (!got) {
            (void)hipGetLastError();
            m.fn[k.fn] = nullptr;
        }
        ok = got || k.optional;
        if (k.optional) {
            some = some || got;
            all = all && got;
        }
    }
    if (!ok || (some && !all)) {
        (void)hipGetLastError();
        m.failed = true;
        for (hipFunction_t &f : m.fn) f = nullptr;
    }
    return m;
}

const Module *find_module(const std::string &key, Prog p, const std::function<Module()> &make) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_cache.find(key);
    if (it == g_cache.end()) {
        it = g_cache.emplace(key, make()).first;
        if (it->second.failed)
            fputs(p == TREE ? "spec_amd jit: tree compile/load failed, run-time tree kernels in use\n"
                            : "spec_amd jit: compile/load failed, generic kernel in use\n", stderr);
    }
    return it->second.failed ? nullptr : &it->second;
}

bool recall_module(int device, const void *desc, size_t bytes, const Module **m) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (const Remembered &k : g_remembered)
        if (k.device == device && k.desc.size() == bytes && memcmp(k.desc.data(), desc, bytes) == 0) {
            *m = k.m;
            return true;
        }
    return false;
}

void remember_module(int device, const void *desc, size_t bytes, const Module *m) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_remembered.push_back({device, std::vector<char>((const char *)desc, (const char *)desc + bytes), m});
}

int launch_module(hipFunction_t fn, unsigned grid, unsigned block, unsigned lds_bytes, hipStream_t stream,
                  const void *args, size_t size) {
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, (void *)args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                     HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, lds_bytes, stream, nullptr, extra) == hipSuccess ? 1 : -1;
}

} // namespace jit

void jit_set_enabled(int on) { jit::g_enabled = on ? 1 : 0; }

} // namespace spec

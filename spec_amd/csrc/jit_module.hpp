// jit_module.hpp — run-time compilation for jit.cpp and jit_tree.cpp: hiprtc, the on-disk
// code-object cache, the loaded modules of this process and their launch.  Nothing here knows a
// schema or a tree: a caller brings a generated source, a cache key and the kernels to load.
#pragma once

#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

namespace spec {
namespace jit {

// The generated programs (jit_module.cpp kProgs: their hiprtc names and dump file stems)
enum Prog { DECODE = 0, ENCODE = 1, NESTED = 2, NESTED_ENC = 3, TREE = 4 };

// A loaded code object and its kernels, by the slots its program's generator defines (jit.cpp
// DecodeFn .. NestedEncFn; tree_internal.hpp TreeFn, the most: jit_tree.cpp checks they fit)
constexpr int MODULE_MAX_FN = 388;
struct Module {
    hipModule_t mod = nullptr;
    hipFunction_t fn[MODULE_MAX_FN] = {};
    bool failed = false;
};
// A kernel of a generated module: its slot in Module::fn and its name.  Optional kernels are
// generated together or not at all.
struct Kernel {
    int fn;
    std::string name;
    bool optional = false;
};

bool enabled(); // SPEC_AMD_JIT (read on first use) or the last jit_set_enabled

// FNV-1a of the source, the embedded headers and the compile options: names the source's code
// object in the disk cache (<hash>.co), and stands for the source where its text is too long a key
uint64_t source_hash(const std::string &src);
// The source's code object, from the disk cache or hiprtc (then cached); empty on failure
std::vector<char> compile_source(const std::string &src, Prog p);
// generate() compiled if `ok` (the program's predicate): the code object's size, 0 for none
template <class Generate>
long long compile_only(bool ok, Prog p, Generate generate) {
    return ok ? (long long)compile_source(generate(), p).size() : 0;
}

// The code object loaded and its kernels looked up; failed if it is empty, does not load, lacks a
// kernel that is not optional, or has only some of the optional ones
Module load_module(const std::vector<char> &code, const std::vector<Kernel> &kernels);
// The module cached under `key`; make() compiles and loads it on first use (under the cache's
// mutex: hiprtc serialises compiles within a process anyway).  A failed compile or load is
// remembered, not retried.  nullptr => use the generic kernel.
const Module *find_module(const std::string &key, Prog p, const std::function<Module()> &make);
// In front of find_module for a program whose source is costly to generate: its answer (nullptr
// included) remembered for the bytes the source is generated from, on one device
bool recall_module(int device, const void *desc, size_t bytes, const Module **m);
void remember_module(int device, const void *desc, size_t bytes, const Module *m);

// fn<<<grid, block, lds_bytes, stream>>> with args[0, size) as its raw parameter buffer: 1, or -1
// on a HIP error
int launch_module(hipFunction_t fn, unsigned grid, unsigned block, unsigned lds_bytes, hipStream_t stream,
                  const void *args, size_t size);

} // namespace jit
} // namespace spec

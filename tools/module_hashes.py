#!/usr/bin/env python3
"""Compile generated modules afresh and print what identifies their code, for comparing two builds.

    python3 tools/module_hashes.py OUT_DIR [share k]      (from the root of a built tree; no GPU)

Modules: flat decode of FLAT16, the bench's wide schemas and every schema of the shape sweep, nested
decode of NESTED, and the first two precompiled trees.  Each is compiled with SPEC_AMD_JIT_DUMP (which
bypasses the code-object cache) into OUT_DIR; per module one line with the sha256 of its .text and
.rodata sections, and one line per kernel with its register counts, scratch, LDS and wavefront size.
An embedded header's text changes a module's cache name and its __hip_cuid_ symbol, not these.
With `share k`: only modules share, share + k, ... (run k processes; hiprtc compiles one at a time).
"""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")

import spec_amd  # noqa: E402
from spec_amd import workload  # noqa: E402
from spec_amd.tree_catalog import precompiled_trees  # noqa: E402


def modules(L):
    flat = {"FLAT16": spec_amd.FLAT16, **workload.bench_wide_schemas(), **workload.shape_sweep_schemas()}
    for name, s in flat.items():
        yield f"flat_{name}_", "decode", lambda s=s: L.spec_decode_flat_jit_compile(C.byref(s.c), 1 << 28, 1 << 20)
    yield "nested_NESTED_", "nested", lambda: L.spec_decode_nested_jit_compile(C.byref(spec_amd.NESTED.c))
    for i, t in enumerate(precompiled_trees()[:2]):
        yield f"tree{i}_", "tree", lambda t=t: L.spec_tree_jit_compile(C.byref(t.c))


def section_sha(co, sec):
    tmp = co + sec + ".bin"
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={sec}", co, tmp], check=True)
    with open(tmp, "rb") as f:
        h = hashlib.sha256(f.read()).hexdigest()
    os.remove(tmp)
    return h


def kernel_meta(co):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    keys = (".name", ".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size",
            ".group_segment_fixed_size", ".wavefront_size")
    rows, cur = [], {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.\w+):\s*(\S+)\s*$", line)
        if not m or m.group(1) not in keys:
            continue
        if m.group(1) in cur:  # the next kernel's entry
            rows.append(cur)
            cur = {}
        cur[m.group(1)] = m.group(2)
    if cur:
        rows.append(cur)
    return sorted((r for r in rows if ".vgpr_count" in r), key=lambda r: r[".name"])


def main():
    out = os.path.abspath(sys.argv[1])
    share, k = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (0, 1)
    os.makedirs(out, exist_ok=True)
    L = spec_amd.lib()
    for prefix, stem, compile_ in list(modules(L))[share::k]:
        os.environ["SPEC_AMD_JIT_DUMP"] = os.path.join(out, prefix)
        if compile_() <= 0:
            raise SystemExit(f"{prefix}: compile failed")
        co = os.path.join(out, prefix + stem + ".co")
        print(f"{prefix}{stem} .text {section_sha(co, '.text')} .rodata {section_sha(co, '.rodata')}")
        for r in kernel_meta(co):
            print(f"{prefix}{stem} " + " ".join(f"{key[1:]}={r.get(key, '-')}" for key in
                                                 (".name", ".vgpr_count", ".agpr_count", ".sgpr_count",
                                                  ".private_segment_fixed_size", ".group_segment_fixed_size",
                                                  ".wavefront_size")))


if __name__ == "__main__":
    main()

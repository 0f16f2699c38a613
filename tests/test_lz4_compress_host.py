"""The compressor's shared integer code (spec_amd/csrc/lz4_compress_core.hpp) in a stand-alone host
program (tests/cpp/lz4_compress_host.cpp) built with AddressSanitizer and UBSan together with the
oracle's lz4.c and run as a plain child process."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sanitizers' runtimes are linked into the program itself: it runs in the environment it inherits
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1",
       "-static-libasan", "-static-libubsan"]


def test_core_on_the_host_under_sanitizers(tmp_path):
    obj, exe = str(tmp_path / "lz4.o"), str(tmp_path / "lz4_compress_host")
    inc = ["-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "spec_amd", "csrc")]
    subprocess.run(["gcc", "-std=c11", "-c", os.path.join(ROOT, "oracle", "lz4.c"), "-o", obj] + SAN + inc, check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "lz4_compress_host.cpp"), obj, "-o",
                    exe] + SAN + inc, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failed" in r.stdout

"""Optional fields through the C++ host API (include/spec_amd.hpp, tests/cpp/test_present.cpp):
MessageBatchWriter::SetPresent -> Build / BuildFrames -> OpenMessageBatch / OpenMessageFrames with
present = true over 130 records with a 50 % mask; built here with g++ (CPU), run on the GPU."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(out):
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_present.cpp"), "-o", out,
           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "spec_amd"), "-lspec_amd",
           "-Wl,-rpath," + os.path.join(ROOT, "spec_amd")]
    subprocess.run(cmd, check=True)


def test_cpp_present_builds(tmp_path):
    build(str(tmp_path / "test_present"))


@pytest.mark.gpu
def test_cpp_present_on_gpu(tmp_path, dev):
    exe = str(tmp_path / "test_present")
    build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout

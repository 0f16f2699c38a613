"""The send path's LZ4 frame compressor (spec_lz4_compress_frame) on the CPU: exported, declared to
ctypes, every argument check made before any HIP call, and spec_lz4_frame_bound equal to the size
of the frame the oracle writes for data no block of which compresses."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import spec_amd
from oracle import oracle as O

P = C.c_void_p(1)  # a non-NULL pointer no check may dereference
OPEN, CLOSE, CC = 1, 2, 4
BM = 64 << 10
NAMES = ("spec_lz4_frame_bound", "spec_lz4_compress_workspace_size", "spec_lz4_compress_frame")


def test_symbols_declared():
    L = spec_amd.lib()
    for name in NAMES:
        assert name in spec_amd.header_symbols()
        assert getattr(L, name).argtypes is not None
    assert L.spec_lz4_frame_bound.restype is C.c_uint64
    assert L.spec_lz4_compress_workspace_size.restype is C.c_size_t
    assert callable(spec_amd.compress_frame) and callable(spec_amd.frame_bound) and callable(spec_amd.Lz4Writer)
    assert spec_amd.lib().spec_abi_version() == 2


def test_argument_checks_without_gpu():
    L = spec_amd.lib()
    f = L.spec_lz4_compress_frame
    ws = L.spec_lz4_compress_workspace_size(100, BM)
    big = 1 << 40
    # unknown flag bits, bad block sizes
    assert f(P, 100, BM, 8, None, P, big, P, P, ws, None) == -1
    assert f(P, 100, BM, 1 << 31, None, P, big, P, P, ws, None) == -1
    for bm in (0, 1, BM - 1, BM + 1, 128 << 10, 8 << 20):
        assert f(P, 100, bm, OPEN, None, P, big, P, P, ws, None) == -1
        assert L.spec_lz4_frame_bound(100, bm, OPEN) == 0
        assert L.spec_lz4_compress_workspace_size(100, bm) == 0
    assert L.spec_lz4_frame_bound(100, BM, 8) == 0
    # NULL pointers with len > 0
    assert f(None, 100, BM, OPEN, None, P, big, P, P, ws, None) == -1
    assert f(P, 100, BM, OPEN, None, None, big, P, P, ws, None) == -1
    assert f(P, 100, BM, OPEN, None, P, big, None, P, ws, None) == -1
    assert f(P, 100, BM, OPEN, None, P, big, P, None, ws, None) == -1
    # a checksummed close needs the digest (with and without data)
    assert f(P, 100, BM, CLOSE | CC, None, P, big, P, P, ws, None) == -1
    assert f(None, 0, BM, OPEN | CLOSE | CC, None, P, big, P, None, 0, None) == -1
    # len reaches 4 GiB
    assert f(P, 1 << 32, BM, OPEN, None, P, 1 << 62, P, P, 1 << 62, None) == -3
    assert f(P, 1 << 40, 4 << 20, 0, None, P, 1 << 62, P, P, 1 << 62, None) == -3
    # out_cap one byte short of the bound, for every kind of call
    for flags in range(8):
        for n in (0, 1, BM, BM + 1):
            bound = L.spec_lz4_frame_bound(n, BM, flags)
            if bound == 0:
                continue
            w = L.spec_lz4_compress_workspace_size(n, BM)
            assert f(P if n else None, n, BM, flags, P, P, bound - 1, P, P, w, None) == -4, (flags, n)
    assert f(P, (1 << 32) - 1, BM, OPEN, None, P, (1 << 32) - 1, P, P, 1 << 62, None) == -4
    # the workspace one byte short
    assert f(P, 100, BM, OPEN, None, P, big, P, P, ws - 1, None) == -5
    w2 = L.spec_lz4_compress_workspace_size(3 * BM + 1, BM)
    assert w2 >= 4 * BM and f(P, 3 * BM + 1, BM, 0, None, P, big, P, P, w2 - 1, None) == -5


@pytest.mark.parametrize("bm", [64 << 10, 256 << 10])
def test_frame_bound_is_the_oracles_stored_frame(bm):
    rng = np.random.default_rng(bm)
    L = spec_amd.lib()
    for n in (0, 1, 12, 13, bm - 1, bm, bm + 1, 2 * bm + 13):
        data = rng.integers(0, 256, n, dtype=np.uint8)
        for cc in (False, True):
            for cl in (False, True):
                flags = (CC if cc else 0) | (CLOSE if cl else 0)
                want = O.lz4_frame_write(data, [n], bm, content_checksum=cc, close=cl).size
                assert L.spec_lz4_frame_bound(n, bm, flags | OPEN) == want, (n, cc, cl)
                assert spec_amd.frame_bound(n, bm, flags | OPEN) == want
                assert L.spec_lz4_frame_bound(n, bm, flags) == want - 7, (n, cc, cl)
    # the figures checked by hand against the format
    assert L.spec_lz4_frame_bound(0, bm, OPEN | CLOSE | CC) == 15
    assert L.spec_lz4_frame_bound(1, bm, OPEN | CLOSE | CC) == 20
    assert L.spec_lz4_frame_bound(12, bm, OPEN | CLOSE | CC) == 31
    assert L.spec_lz4_frame_bound(0, bm, 0) == 0 and L.spec_lz4_frame_bound(1 << 32, bm, OPEN) == 0

"""The send path's frame writer (spec_frames_write) on the CPU: exported, declared to ctypes, and
every argument check made before any HIP call."""
from __future__ import annotations

import ctypes as C

import spec_amd

P = C.c_void_p(1)  # a non-NULL pointer no check may dereference


def test_symbol_declared():
    L = spec_amd.lib()
    assert "spec_frames_write" in spec_amd.header_symbols()
    assert L.spec_frames_write.argtypes is not None
    assert callable(spec_amd.write_frames)


def test_frames_write_argument_checks_without_gpu():
    L = spec_amd.lib()
    # n == 0 is a no-op whatever else is passed
    assert L.spec_frames_write(None, 0, None, 0, None, 0, None, None) == 0
    assert L.spec_frames_write(P, 10, None, 0, None, 0, None, None) == 0
    # NULL pointers with n > 0 (frame_ends may be NULL: checked below by reaching the next check)
    assert L.spec_frames_write(P, 10, None, 1, P, 100, P, None) == -1
    assert L.spec_frames_write(P, 10, P, 1, None, 100, P, None) == -1
    assert L.spec_frames_write(None, 10, P, 1, P, 100, P, None) == -1
    # stream_len + 4 n reaches 4 GiB
    assert L.spec_frames_write(P, (1 << 32) - 4, P, 1, P, 1 << 33, None, None) == -3
    assert L.spec_frames_write(P, 0, P, 1 << 30, P, 1 << 33, None, None) == -3
    assert L.spec_frames_write(P, 1 << 32, P, 1, P, 1 << 33, None, None) == -3
    # frames_cap one byte short
    assert L.spec_frames_write(P, 10, P, 2, P, 17, None, None) == -4
    assert L.spec_frames_write(P, (1 << 32) - 9, P, 2, P, (1 << 32) - 2, None, None) == -4

"""The fused framed encoder (spec_encode_flat_frames) on the CPU: exported, declared to ctypes,
reachable from Python, every argument check made before any HIP call, and the generated encode
source (which now holds the framed write kernel too) still compiles for gfx950."""
from __future__ import annotations

import ctypes as C

import spec_amd
from spec_amd import Field, Kind, Schema
from spec_amd._lib import SpecSchema

P = C.c_void_p(1)  # a non-NULL pointer no check may dereference
INVALID_ARGUMENT, WORKSPACE = -1, -5  # include/spec_amd.h SPEC_E_*


def _call(schema_c, columns, heaps, heap_lens, n, frames, cap, frame_ends, ws, ws_size):
    return spec_amd.lib().spec_encode_flat_frames(schema_c, columns, heaps, heap_lens, n, frames, cap, frame_ends,
                                                  ws, ws_size, P, None)


def _ptrs(nf):
    return (C.c_void_p * max(1, nf))(*([1] * nf))


def test_symbol_declared_and_wrappers_callable():
    L = spec_amd.lib()
    assert "spec_encode_flat_frames" in spec_amd.header_symbols()
    assert L.spec_encode_flat_frames.argtypes is not None
    assert len(L.spec_encode_flat_frames.argtypes) == 12
    assert callable(spec_amd.encode_flat_frames)
    assert callable(spec_amd.Encoder.encode_frames_into)
    assert "encode_flat_frames" in spec_amd.__all__
    assert L.spec_abi_version() == 2  # a new function does not bump the ABI


def test_argument_checks_without_gpu():
    L = spec_amd.lib()
    sc = C.byref(spec_amd.FLAT16.c)
    nf = len(spec_amd.FLAT16)
    cols, heaps, lens = _ptrs(nf), _ptrs(nf), (C.c_uint64 * nf)()
    n = 100
    ws = L.spec_encode_flat_workspace_size(n)
    # an invalid schema: NULL, and a kind that does not exist
    assert _call(None, cols, heaps, lens, n, P, 1 << 20, P, P, ws) == INVALID_ARGUMENT
    bad = SpecSchema()
    bad.nfields = 1
    bad.fields[0].tag = 1
    bad.fields[0].kind = 250
    assert _call(C.byref(bad), cols, heaps, lens, n, P, 1 << 20, P, P, ws) == INVALID_ARGUMENT
    # NULL columns / workspace / frames / frame_ends with n > 0
    assert _call(sc, None, heaps, lens, n, P, 1 << 20, P, P, ws) == INVALID_ARGUMENT
    assert _call(sc, cols, heaps, lens, n, P, 1 << 20, P, None, ws) == INVALID_ARGUMENT
    assert _call(sc, cols, heaps, lens, n, None, 1 << 20, P, P, ws) == INVALID_ARGUMENT
    assert _call(sc, cols, heaps, lens, n, P, 1 << 20, None, P, ws) == INVALID_ARGUMENT
    # a workspace one byte short
    assert _call(sc, cols, heaps, lens, n, P, 1 << 20, P, P, ws - 1) == WORKSPACE
    # a string field with NULL heaps (Flat16 has string and bytes columns)
    assert any(f.kind in (Kind.STRING, Kind.BYTES) for f in spec_amd.FLAT16.fields)
    assert _call(sc, cols, None, lens, n, P, 1 << 20, P, P, ws) == INVALID_ARGUMENT
    assert _call(sc, cols, heaps, None, n, P, 1 << 20, P, P, ws) == INVALID_ARGUMENT


def test_wide_schema_argument_checks_without_gpu():
    # more than 64 fields: the wide path, whose checks also precede its field-set upload
    L = spec_amd.lib()
    schema = Schema([Field(i + 1, Kind.STRING if i == 70 else Kind.INT32) for i in range(72)])
    nf = len(schema)
    cols, heaps, lens = _ptrs(nf), _ptrs(nf), (C.c_uint64 * nf)()
    ws = L.spec_encode_flat_workspace_size(10)
    sc = C.byref(schema.c)
    assert _call(sc, cols, heaps, lens, 10, None, 1 << 20, P, P, ws) == INVALID_ARGUMENT
    assert _call(sc, cols, heaps, lens, 10, P, 1 << 20, P, P, ws - 1) == WORKSPACE
    assert _call(sc, cols, None, lens, 10, P, 1 << 20, P, P, ws) == INVALID_ARGUMENT


def test_generated_encode_source_compiles_for_gfx950():
    # hiprtc, no device: the module of the size, write, and framed write kernels
    L = spec_amd.lib()
    assert L.spec_encode_flat_jit_compile(C.byref(spec_amd.FLAT16.c)) > 0
    big_tag = Schema([Field(300, Kind.INT64), Field(2, Kind.STRING), Field(3, Kind.BOOL)])
    assert L.spec_encode_flat_jit_compile(C.byref(big_tag.c)) > 0

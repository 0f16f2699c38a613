"""The optional-field entry points (spec_decode_flat_present, spec_decode_frames_present,
spec_encode_flat_present, spec_encode_flat_present_frames) on the CPU: in the header, declared to
ctypes with their dense twins' arguments plus the mask, reachable from Python, every argument
check made before any HIP call, and the generated decode module (with the present kernels) still
compiles for gfx950."""
from __future__ import annotations

import ctypes as C
import inspect

import spec_amd
from spec_amd import FLAT16, Kind, Schema
from spec_amd._lib import SpecSchema

P = C.c_void_p(1)  # a non-NULL pointer no check may dereference
INVALID_ARGUMENT, TOO_LARGE, WORKSPACE = -1, -3, -5  # include/spec_amd.h SPEC_E_*
GIB4 = 1 << 32


def _ptrs(nf, v=1):
    return (C.c_void_p * max(1, nf))(*([v] * nf))


def _lens(nf):
    return (C.c_uint64 * max(1, nf))(*([16] * nf))


def test_symbols_declared_and_wrappers_exported():
    L = spec_amd.lib()
    syms = spec_amd.header_symbols()
    for name, twin, extra in (("spec_decode_flat_present", "spec_decode_flat_errors", 1),
                              ("spec_decode_frames_present", "spec_decode_frames_errors", 1),
                              ("spec_encode_flat_present", "spec_encode_flat", 1),
                              ("spec_encode_flat_present_frames", "spec_encode_flat_frames", 1)):
        assert name in syms, name
        assert len(getattr(L, name).argtypes) == len(getattr(L, twin).argtypes) + extra, name
    assert len(L.spec_decode_flat_present.argtypes) == 10
    assert len(L.spec_decode_frames_present.argtypes) == 12
    assert len(L.spec_encode_flat_present.argtypes) == 13
    assert L.spec_encode_flat_present_frames.argtypes == L.spec_encode_flat_present.argtypes
    for name in ("decode_flat_present", "decode_frames_present", "encode_flat_present"):
        assert callable(getattr(spec_amd, name)) and name in spec_amd.__all__, name
    for name in ("size_present", "encode_present_into", "encode_present_frames_into"):
        assert callable(getattr(spec_amd.Encoder, name)), name
    sig = inspect.signature(spec_amd.decode_flat_present)
    assert sig.parameters["errors"].default is False and sig.parameters["cuda_stream"].default is None
    sig = inspect.signature(spec_amd.encode_flat_present)
    assert list(sig.parameters)[:6] == ["schema", "cols", "heaps", "present", "n", "frames"]
    assert L.spec_abi_version() == 2  # new functions do not bump the ABI


def _bad_schemas():
    bad = SpecSchema.from_buffer_copy(FLAT16.c)
    bad.fields[0].kind = 250
    empty = SpecSchema.from_buffer_copy(FLAT16.c)
    empty.nfields = 0
    over = SpecSchema.from_buffer_copy(FLAT16.c)
    over.nfields = 1025
    return [None, C.byref(bad), C.byref(empty), C.byref(over)]


def test_decode_argument_checks_without_gpu():
    L = spec_amd.lib()
    sc = C.byref(FLAT16.c)
    cols = _ptrs(len(FLAT16))

    def flat(s=sc, stream=P, stream_len=1000, ends=P, n=100, columns=cols, errmask=None, present=P):
        return L.spec_decode_flat_present(s, stream, stream_len, ends, n, columns, P, errmask, present, None)

    def frames(s=sc, buf=P, buf_len=1000, ends=P, r0=0, r1=100, columns=cols, errmask=None, present=P):
        return L.spec_decode_frames_present(s, buf, buf_len, ends, r0, r1, 0, columns, P, errmask, present, None)

    for call in (flat, frames):
        for s in _bad_schemas():
            assert call(s=s) == INVALID_ARGUMENT
        assert call(present=None) == INVALID_ARGUMENT
        assert call(ends=None) == INVALID_ARGUMENT
        assert call(columns=None) == INVALID_ARGUMENT
        hole = _ptrs(len(FLAT16))
        hole[3] = None
        assert call(columns=hole) == INVALID_ARGUMENT
    assert flat(stream=None) == INVALID_ARGUMENT
    assert flat(stream_len=GIB4) == TOO_LARGE
    assert flat(n=0, present=None) == INVALID_ARGUMENT  # present is required even for an empty batch
    assert flat(n=0, stream=None, ends=None, columns=None) == 0
    assert frames(buf=None) == INVALID_ARGUMENT
    assert frames(buf_len=GIB4) == TOO_LARGE
    assert frames(r0=5, r1=4) == INVALID_ARGUMENT
    assert frames(r0=7, r1=7, buf=None, ends=None, columns=None) == 0  # an empty range: nothing to do
    # a schema of more than 64 fields (the chunked route): the same checks first
    wide = Schema([(i + 1, Kind.INT32) for i in range(100)])
    assert flat(s=C.byref(wide.c), columns=_ptrs(100), present=None) == INVALID_ARGUMENT
    hole = _ptrs(100)
    hole[99] = None
    assert flat(s=C.byref(wide.c), columns=hole) == INVALID_ARGUMENT


def test_encode_argument_checks_without_gpu():
    L = spec_amd.lib()
    sc = C.byref(FLAT16.c)
    nf = len(FLAT16)
    n = 100
    ws = L.spec_encode_flat_workspace_size(n)

    for fn in (L.spec_encode_flat_present, L.spec_encode_flat_present_frames):
        def call(s=sc, columns=_ptrs(nf), heaps=_ptrs(nf), lens=_lens(nf), present=P, out=P, ends=P, work=P,
                 ws_size=ws, total=P):
            return fn(s, columns, heaps, lens, present, n, out, 1 << 20, ends, work, ws_size, total, None)

        for s in _bad_schemas():
            assert call(s=s) == INVALID_ARGUMENT
        assert call(present=None) == INVALID_ARGUMENT
        assert call(columns=None) == INVALID_ARGUMENT
        assert call(work=None) == INVALID_ARGUMENT
        assert call(total=None) == INVALID_ARGUMENT
        assert call(ends=None) == INVALID_ARGUMENT  # with out: the ends are written too
        assert call(heaps=None) == INVALID_ARGUMENT  # FLAT16 has string / bytes fields
        assert call(lens=None) == INVALID_ARGUMENT
        assert call(heaps=_ptrs(nf, None)) == INVALID_ARGUMENT  # NULL heap with a length
        assert call(ws_size=ws - 1) == WORKSPACE


def test_generated_decode_sources_compile_for_gfx950():
    # hiprtc, no device: the present kernels live in the schema's decode module (the schemas
    # build() precompiles: the sparse fast path, the 40-field and the big-table class)
    from spec_amd import workload

    L = spec_amd.lib()
    for s in (FLAT16, *workload.bench_wide_schemas().values()):
        assert L.spec_decode_flat_jit_compile(C.byref(s.c), 1 << 28, 1 << 20) > 0

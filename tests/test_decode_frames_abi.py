"""The decoders over mpx frames (spec_decode_frames_errors, spec_decode_nested_frames_index,
spec_decode_nested_frames, spec_decode_nested_frames_onepass, spec_tree_decoder_index_frames,
spec_tree_decoder_run_frames, spec_host_decoder_run_frames) on the CPU: in the header, declared to
ctypes with their unframed twins' arguments, reachable from Python, every argument check made before
any HIP call, and the generated decode sources still compile for gfx950 with `head` in NestedArgs
and TreeBufs."""
from __future__ import annotations

import ctypes as C

import spec_amd
from spec_amd import FLAT16, NESTED, Kind, NestedSchema
from spec_amd._lib import SpecNestedSchema, SpecSchema

P = C.c_void_p(1)  # a non-NULL pointer no check may dereference
INVALID_ARGUMENT, TOO_LARGE, WORKSPACE = -1, -3, -5  # include/spec_amd.h SPEC_E_*
GIB4 = 1 << 32

TWINS = {  # framed entry point -> (unframed twin, argument count)
    "spec_decode_frames_errors": ("spec_decode_flat_range", 11),  # the range call's arguments + errmask
    "spec_decode_nested_frames_index": ("spec_decode_nested_index", 9),
    "spec_decode_nested_frames": ("spec_decode_nested", 14),
    "spec_decode_nested_frames_onepass": ("spec_decode_nested_onepass", 15),
    "spec_tree_decoder_index_frames": ("spec_tree_decoder_index", 7),
    "spec_tree_decoder_run_frames": ("spec_tree_decoder_run", 9),
    "spec_host_decoder_run_frames": ("spec_host_decoder_run", 6),
}


def _ptrs(nf):
    return (C.c_void_p * max(1, nf))(*([1] * nf))


def test_symbols_declared_and_wrappers_exported():
    L = spec_amd.lib()
    syms = spec_amd.header_symbols()
    for name, (twin, nargs) in TWINS.items():
        assert name in syms, name
        got = len(getattr(L, name).argtypes)
        assert got == nargs, (name, got)
        if name != "spec_decode_frames_errors":
            assert got == len(getattr(L, twin).argtypes), name
    assert len(L.spec_decode_frames_errors.argtypes) == len(L.spec_decode_flat_range.argtypes) + 1
    for name in ("decode_frames_errors", "decode_nested_frames", "decode_tree_frames"):
        assert callable(getattr(spec_amd, name)) and name in spec_amd.__all__, name
    assert callable(spec_amd.TreeDecoder.index_frames) and callable(spec_amd.TreeDecoder.run_frames)
    assert callable(spec_amd.HostDecoder.run_frames)
    import inspect

    assert inspect.signature(spec_amd.NestedDecoder.__init__).parameters["head"].default == 0
    assert L.spec_abi_version() == 2  # new functions do not bump the ABI


def _index(schema_c, frames=P, frames_len=1000, ends=P, n=100, ws=P, ws_size=None, total=P):
    L = spec_amd.lib()
    ws_size = L.spec_decode_nested_workspace_size(n) if ws_size is None else ws_size
    return L.spec_decode_nested_frames_index(schema_c, frames, frames_len, ends, n, ws, ws_size, total, None)


def _decode(fn, schema_c, schema=NESTED, frames=P, frames_len=1000, ends=P, n=100, outer="default", item_begin=P,
            items="default", item_cap=300, ws=P, ws_size=None, total=P):
    L = spec_amd.lib()
    ws_size = L.spec_decode_nested_workspace_size(n) if ws_size is None else ws_size
    oc = _ptrs(len(schema.outer)) if outer == "default" else outer
    ic = _ptrs(len(schema.item)) if items == "default" else items
    args = [schema_c, frames, frames_len, ends, n, oc, P, item_begin, ic, P, item_cap, ws, ws_size]
    if fn == "spec_decode_nested_frames_onepass":
        args.append(total)
    return getattr(L, fn)(*args, None)


def test_nested_argument_checks_without_gpu():
    sc = C.byref(NESTED.c)
    bad = SpecNestedSchema.from_buffer_copy(NESTED.c)
    bad.item.fields[0].kind = 250
    flat = SpecNestedSchema.from_buffer_copy(NESTED.c)
    for f in range(flat.outer.nfields):
        if flat.outer.fields[f].kind == int(Kind.LIST):
            flat.outer.fields[f].kind = int(Kind.INT32)
    # the index
    for s in (None, C.byref(bad), C.byref(flat)):
        assert _index(s) == INVALID_ARGUMENT
    assert _index(sc, frames=None) == INVALID_ARGUMENT
    assert _index(sc, ends=None) == INVALID_ARGUMENT
    assert _index(sc, ws=None) == INVALID_ARGUMENT
    assert _index(sc, total=None) == INVALID_ARGUMENT
    assert _index(sc, ws_size=spec_amd.lib().spec_decode_nested_workspace_size(100) - 1) == WORKSPACE
    assert _index(sc, frames_len=GIB4) == TOO_LARGE
    # the decode and the one-pass call
    lf = next(f for f, fld in enumerate(NESTED.outer.fields) if fld.kind == Kind.LIST)
    for fn in ("spec_decode_nested_frames", "spec_decode_nested_frames_onepass"):
        for s in (None, C.byref(bad), C.byref(flat)):
            assert _decode(fn, s) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, frames=None) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, ends=None) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, ws=None) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, outer=None) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, item_begin=None) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, items=None) == INVALID_ARGUMENT, fn
        hole = _ptrs(len(NESTED.outer))
        hole[(lf + 1) % len(NESTED.outer)] = None  # (the list field's own column is never read)
        assert _decode(fn, sc, outer=hole) == INVALID_ARGUMENT, fn
        hole = _ptrs(len(NESTED.item))
        hole[1] = None
        assert _decode(fn, sc, items=hole) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, ws_size=spec_amd.lib().spec_decode_nested_workspace_size(100) - 1) == WORKSPACE, fn
        assert _decode(fn, sc, frames_len=GIB4) == TOO_LARGE, fn
    assert _decode("spec_decode_nested_frames_onepass", sc, total=None) == INVALID_ARGUMENT


def test_nested_wide_half_argument_checks_without_gpu():
    # an item schema of 70 fields: the chunked decode, whose checks also come first
    schema = NestedSchema([(1, Kind.INT64), (2, Kind.LIST)], [(i + 1, Kind.INT32) for i in range(70)])
    sc = C.byref(schema.c)
    for fn in ("spec_decode_nested_frames", "spec_decode_nested_frames_onepass"):
        assert _decode(fn, sc, schema, outer=None) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, schema, ws=None) == INVALID_ARGUMENT, fn
        hole = _ptrs(70)
        hole[69] = None
        assert _decode(fn, sc, schema, items=hole) == INVALID_ARGUMENT, fn
        assert _decode(fn, sc, schema, ws_size=8) == WORKSPACE, fn
        assert _decode(fn, sc, schema, frames_len=GIB4) == TOO_LARGE, fn
    assert _decode("spec_decode_nested_frames_onepass", sc, schema, total=None) == INVALID_ARGUMENT


def test_flat_errors_argument_checks_without_gpu():
    L = spec_amd.lib()
    sc = C.byref(FLAT16.c)
    cols = _ptrs(len(FLAT16))

    def call(s=sc, frames=P, frames_len=1000, ends=P, r0=0, r1=100, columns=cols, errmask=P):
        return L.spec_decode_frames_errors(s, frames, frames_len, ends, r0, r1, 0, columns, P, errmask, None)

    assert call(s=None) == INVALID_ARGUMENT
    bad = SpecSchema.from_buffer_copy(FLAT16.c)
    bad.fields[0].kind = 250
    assert call(s=C.byref(bad)) == INVALID_ARGUMENT
    assert call(frames=None) == INVALID_ARGUMENT
    assert call(ends=None) == INVALID_ARGUMENT
    assert call(columns=None) == INVALID_ARGUMENT
    assert call(errmask=None) == INVALID_ARGUMENT
    hole = _ptrs(len(FLAT16))
    hole[3] = None
    assert call(columns=hole) == INVALID_ARGUMENT
    assert call(r0=5, r1=4) == INVALID_ARGUMENT
    assert call(frames_len=GIB4) == TOO_LARGE
    assert call(r0=7, r1=7, frames=None, ends=None, columns=None, errmask=None) == 0  # an empty range: nothing to do


def test_tree_and_host_argument_checks_without_gpu():
    # (a decoder itself needs a device: only the checks that come before it is looked at)
    L = spec_amd.lib()
    assert L.spec_tree_decoder_index_frames(None, P, 1000, P, 10, None, None) == INVALID_ARGUMENT
    assert L.spec_tree_decoder_run_frames(None, P, 1000, P, 10, _ptrs(4), None, None, None) == INVALID_ARGUMENT
    assert L.spec_host_decoder_run_frames(None, P, 1000, P, 10, P) == INVALID_ARGUMENT


def test_generated_decode_sources_compile_for_gfx950():
    # hiprtc, no device: NestedArgs and TreeBufs carry `head`; the flat kernels are untouched
    L = spec_amd.lib()
    assert L.spec_decode_nested_jit_compile(C.byref(NESTED.c)) > 0
    assert L.spec_tree_jit_compile(C.byref(spec_amd.pkg1_tree().c)) > 0
    assert L.spec_decode_flat_jit_compile(C.byref(FLAT16.c), 1 << 28, 1 << 20) > 0

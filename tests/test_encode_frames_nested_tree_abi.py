"""The framed nested and tree encoders (spec_encode_nested_frames, spec_encode_tree_frames) on the
CPU: exported, declared to ctypes, reachable from Python, every argument check made before any
HIP call, and the generated nested encode source (which now holds the framed write kernels too)
still compiles for gfx950."""
from __future__ import annotations

import ctypes as C

import spec_amd
from spec_amd import Kind, NestedSchema
from spec_amd._lib import SpecNestedSchema, SpecTree

P = C.c_void_p(1)  # a non-NULL pointer no check may dereference
INVALID_ARGUMENT, WORKSPACE = -1, -5  # include/spec_amd.h SPEC_E_*
NESTED = spec_amd.NESTED


def _ptrs(nf):
    return (C.c_void_p * max(1, nf))(*([1] * nf))


def _nested(schema_c, outer_cols, item_begin, item_cols, nitems, n, frames, frame_ends, ws, ws_size, total=P,
            outer_heaps="default", item_heaps="default"):
    no, ni = len(NESTED.outer), len(NESTED.item)
    oh = _ptrs(no) if outer_heaps == "default" else outer_heaps
    ih = _ptrs(ni) if item_heaps == "default" else item_heaps
    return spec_amd.lib().spec_encode_nested_frames(schema_c, outer_cols, oh, (C.c_uint64 * no)(), item_begin,
                                                    item_cols, ih, (C.c_uint64 * ni)(), nitems, n, frames, 1 << 20,
                                                    frame_ends, ws, ws_size, total, None)


def test_symbols_declared_and_wrappers_callable():
    L = spec_amd.lib()
    syms = spec_amd.header_symbols()
    assert "spec_encode_nested_frames" in syms and "spec_encode_tree_frames" in syms
    assert len(L.spec_encode_nested_frames.argtypes) == len(L.spec_encode_nested.argtypes) == 17
    assert len(L.spec_encode_tree_frames.argtypes) == len(L.spec_encode_tree.argtypes) == 12
    assert callable(spec_amd.encode_nested_frames) and callable(spec_amd.NestedEncoder.encode_frames)
    assert callable(spec_amd.encode_tree_frames) and callable(spec_amd.TreeEncoder.encode_frames)
    assert "encode_nested_frames" in spec_amd.__all__ and "encode_tree_frames" in spec_amd.__all__
    assert L.spec_abi_version() == 2  # new functions do not bump the ABI


def test_nested_argument_checks_without_gpu():
    L = spec_amd.lib()
    sc = C.byref(NESTED.c)
    oc, ic = _ptrs(len(NESTED.outer)), _ptrs(len(NESTED.item))
    n, nitems = 100, 300
    ws = L.spec_encode_nested_workspace_size(n)
    # an invalid schema: NULL, an item kind that does not exist, an outer schema without a list
    assert _nested(None, oc, P, ic, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    bad = SpecNestedSchema.from_buffer_copy(NESTED.c)
    bad.item.fields[0].kind = 250
    assert _nested(C.byref(bad), oc, P, ic, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    flat = SpecNestedSchema.from_buffer_copy(NESTED.c)
    for f in range(flat.outer.nfields):
        if flat.outer.fields[f].kind == int(Kind.LIST):
            flat.outer.fields[f].kind = int(Kind.INT32)
    assert _nested(C.byref(flat), oc, P, ic, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    # NULL outer columns / item_begin / item columns / total / workspace; frames without frame_ends
    assert _nested(sc, None, P, ic, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    assert _nested(sc, oc, None, ic, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    assert _nested(sc, oc, P, None, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    assert _nested(sc, oc, P, ic, nitems, n, P, P, P, ws, total=None) == INVALID_ARGUMENT
    assert _nested(sc, oc, P, ic, nitems, n, P, P, None, ws) == INVALID_ARGUMENT
    assert _nested(sc, oc, P, ic, nitems, n, P, None, P, ws) == INVALID_ARGUMENT
    # one outer column NULL (not the list field's, which is never read)
    lf = next(f for f, fld in enumerate(NESTED.outer.fields) if fld.kind == Kind.LIST)
    hole = _ptrs(len(NESTED.outer))
    hole[(lf + 1) % len(NESTED.outer)] = None
    assert _nested(sc, hole, P, ic, nitems, n, P, P, P, ws) == INVALID_ARGUMENT
    # string fields with NULL heaps
    assert any(f.kind in (Kind.STRING, Kind.BYTES) for f in NESTED.outer.fields)
    assert _nested(sc, oc, P, ic, nitems, n, P, P, P, ws, outer_heaps=None) == INVALID_ARGUMENT
    assert any(f.kind in (Kind.STRING, Kind.BYTES) for f in NESTED.item.fields)
    assert _nested(sc, oc, P, ic, nitems, n, P, P, P, ws, item_heaps=None) == INVALID_ARGUMENT
    # a workspace one byte short
    assert _nested(sc, oc, P, ic, nitems, n, P, P, P, ws - 1) == WORKSPACE


def test_nested_wide_half_argument_checks_without_gpu():
    # an item schema of 70 fields: the tree route, whose checks also come first
    L = spec_amd.lib()
    schema = NestedSchema([(1, Kind.INT64), (2, Kind.LIST)], [(i + 1, Kind.INT32) for i in range(70)])
    no, ni = 2, 70
    ws = L.spec_encode_nested_workspace_size(10)

    def call(oc, ws_ptr, ws_size, total=P):
        return L.spec_encode_nested_frames(C.byref(schema.c), oc, _ptrs(no), (C.c_uint64 * no)(), P, _ptrs(ni),
                                           _ptrs(ni), (C.c_uint64 * ni)(), 30, 10, P, 1 << 20, P, ws_ptr, ws_size,
                                           total, None)

    assert call(None, P, ws) == INVALID_ARGUMENT
    assert call(_ptrs(no), None, ws) == INVALID_ARGUMENT
    assert call(_ptrs(no), P, ws, total=None) == INVALID_ARGUMENT
    assert call(_ptrs(no), P, ws - 1) == WORKSPACE
    hole = _ptrs(no)
    hole[0] = None
    assert call(hole, P, ws) == INVALID_ARGUMENT


def test_tree_argument_checks_without_gpu():
    L = spec_amd.lib()
    tree = spec_amd.pkg1_tree()
    nt, nc = len(tree.tables), len(tree.columns)
    rows = (C.c_uint64 * nt)(*([8] * nt))
    ws = L.spec_encode_tree_workspace_size(C.byref(tree.c), rows)
    assert ws > 0
    cols, heaps, lens = _ptrs(nc), _ptrs(nc), (C.c_uint64 * nc)()

    def call(tc, cp, rp, ws_ptr, ws_size, total=P, hp=heaps):
        return L.spec_encode_tree_frames(tc, cp, hp, lens, rp, P, 1 << 20, P, ws_ptr, ws_size, total, None)

    tc = C.byref(tree.c)
    # an invalid tree: NULL, and a field whose parent follows it
    assert call(None, cols, rows, P, ws) == INVALID_ARGUMENT
    bad = SpecTree.from_buffer_copy(tree.c)
    bad.fields[0].parent = 5
    assert call(C.byref(bad), cols, rows, P, ws) == INVALID_ARGUMENT
    # NULL columns / rows / total / workspace
    assert call(tc, None, rows, P, ws) == INVALID_ARGUMENT
    assert call(tc, cols, None, P, ws) == INVALID_ARGUMENT
    assert call(tc, cols, rows, P, ws, total=None) == INVALID_ARGUMENT
    assert call(tc, cols, rows, None, ws) == INVALID_ARGUMENT
    # one input column NULL while its table has rows; a span column without its heap
    from spec_amd.tree import INPUT_ROLES

    c = next(c for c in tree.columns if c.role in INPUT_ROLES)
    hole = _ptrs(nc)
    hole[c.index] = None
    assert call(tc, hole, rows, P, ws) == INVALID_ARGUMENT
    assert call(tc, cols, rows, P, ws, hp=None) == INVALID_ARGUMENT
    # a workspace one byte short
    assert call(tc, cols, rows, P, ws - 1) == WORKSPACE


def test_tree_return_code_precedence_without_gpu():
    # spec_encode_tree's checks in their order: invalid tree, workspace, then columns and rows
    from spec_amd.tree import INPUT_ROLES, REL_ONE, Message, Tree

    L = spec_amd.lib()
    tree = Tree(Message("R", [("a", 1, Kind.INT32), ("sub", 2, Message("S", [("x", 1, Kind.INT64)]))]))
    child = next(t for t in tree.tables if t.rel == REL_ONE)
    nt, nc = len(tree.tables), len(tree.columns)
    rows = (C.c_uint64 * nt)(*([8] * nt))
    ws = L.spec_encode_tree_workspace_size(C.byref(tree.c), rows)
    assert ws > 0

    def call(tc, cp, rp, ws_size):
        return L.spec_encode_tree(tc, cp, None, None, rp, P, 1 << 20, P, P, ws_size, P, None)

    # a sub-message table has a row per owner row
    short = (C.c_uint64 * nt)(*([8] * nt))
    short[child.index] = 7
    assert short[child.index] != short[child.parent]
    assert call(C.byref(tree.c), _ptrs(nc), short, ws) == INVALID_ARGUMENT
    # a null input column and a workspace one byte short: the workspace is checked first
    hole = _ptrs(nc)
    hole[next(c for c in tree.columns if c.role in INPUT_ROLES).index] = None
    assert call(C.byref(tree.c), hole, rows, ws) == INVALID_ARGUMENT
    assert call(C.byref(tree.c), hole, rows, ws - 1) == WORKSPACE
    # an invalid tree and a workspace one byte short: the tree is checked first
    bad = SpecTree.from_buffer_copy(tree.c)
    bad.fields[0].parent = 5
    assert call(C.byref(bad), _ptrs(nc), rows, ws - 1) == INVALID_ARGUMENT


def test_generated_nested_encode_source_compiles_for_gfx950():
    # hiprtc, no device: the module of the size kernel, the write kernels (one wave per group and a
    # wave pair) and their framed instantiations
    L = spec_amd.lib()
    assert L.spec_encode_nested_jit_compile(C.byref(NESTED.c)) > 0

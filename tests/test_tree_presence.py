"""Schema trees with optional fields (SPEC_TREE_FIELD_OPTIONAL, the HASMASK column) without a GPU:
the layout, the refusal of every invalid placement of the flag before any HIP call, the generated
source, and the record walker of tests/tree_presence_helpers.py pinned against the oracle through
the plain tree and the pruned tree, the two references that need no walker."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import pytest

import spec_amd
from oracle import oracle as O
from oracle.tree_oracle import oracle_decode, oracle_encode, oracle_fields
from spec_amd import Kind, workload
from spec_amd.tree import (FIELD_OPTIONAL, INPUT_ROLES, ROLE_ERRMASK, ROLE_HASMASK, ROLE_STATUS, ListOf, Message, Opt,
                           Struct, Tree)
from spec_amd.tree_catalog import PRESENCE_TREES_JSON, precompiled_trees, presence_trees
from tests import tree_presence_helpers as H

SPEC_E_INVALID_ARGUMENT = -1
NAMES = ["presence_small", "presence_wide", "pkg1"]


# ---- layout ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_hasmask_follows_errmask_with_its_width(name):
    tree = H.tree_of(name)
    assert ROLE_HASMASK == 6 and ROLE_HASMASK in INPUT_ROLES
    seen = 0
    for t in tree.tables:
        roles = [c.role for c in t.columns]
        flagged = t.shape == 0 and any(tree.fields[i].optional for i in H.direct_fields(tree, t.index))
        assert (ROLE_HASMASK in roles) == flagged, t.path
        if not flagged:
            continue
        seen += 1
        e = roles.index(ROLE_ERRMASK)
        assert roles[e + 1] == ROLE_HASMASK and roles[e + 2] == ROLE_STATUS and roles.count(ROLE_HASMASK) == 1
        nd = len(H.direct_fields(tree, t.index))
        assert t.columns[e + 1].width == t.columns[e].width == 8 * max(1, (nd + 63) // 64)
        assert t.columns[e + 1].name == f"{t.path}#hasmask"
    assert seen >= 2


def test_layout_shapes_of_the_test_trees():
    small, wide = H.tree_of("presence_small"), H.tree_of("presence_wide")
    assert "nf#hasmask" not in small.by_name and "nf#errmask" in small.by_name  # a table with nothing flagged
    assert {"#hasmask", "sub#hasmask", "items[]#hasmask"} == {c.name for c in H.hasmask_columns(small)}
    flags = {f.path: f.optional for f in small.fields}
    assert flags["i32"] and flags["st"] and not flags["plain"] and not flags["st.name"] and not flags["any"]
    assert any(f.tag == 300 and f.optional for f in small.fields)
    assert wide.by_name["#hasmask"].width == 24 and wide.by_name["sub#hasmask"].width == 16
    d = H.direct_fields(wide, 0)
    assert len(d) == 131 and all(wide.fields[d[k]].optional for k in (63, 64, 65, 129))


@pytest.mark.parametrize("name", NAMES)
def test_unflagged_layout_is_the_oracles(name):
    """The plain tree's layout is exactly what it was: the oracle's, column for column; and the
    presence tree's layout is the plain one with the HASMASK columns put in."""
    tree = H.tree_of(name)
    plain = tree.plain()
    tables, cols = O.tree_layout(oracle_fields(plain))
    assert len(tables) == len(plain.tables) and len(cols) == len(plain.columns)
    for c, w in zip(plain.columns, cols):
        assert (c.table, c.field, c.role, c.kind, c.width) == tuple(int(w[k]) for k in ("table", "field", "role", "kind", "width"))
    for t, w in zip(plain.tables, tables):
        assert len(t.columns) == int(w["ncolumns"])
    assert [c.name for c in tree.columns if c.role != ROLE_HASMASK] == [c.name for c in plain.columns]
    assert all(c.role != ROLE_HASMASK for c in plain.columns)


def test_tree_python_surface():
    """Opt(), presence=, TreeField.optional, to_fields / from_fields with the sixth element."""
    st = Struct("S", [("a", Kind.INT32)])
    msg = Message("M", [("x", 1, Opt(Kind.INT32)), ("y", 2, Kind.INT32), ("s", 3, Opt(st)), ("z", 4, Kind.ANY),
                        ("l", 5, ListOf(Kind.INT32))])
    t = Tree(msg)
    assert [f.optional for f in t.fields] == [True, False, True, False, False, False]
    assert [len(f) for f in t.to_fields()] == [6, 5, 6, 5, 5, 5]
    t2 = Tree.from_fields(json.loads(json.dumps(t.to_fields())))
    assert [f.optional for f in t2.fields] == [f.optional for f in t.fields]
    assert [c.name for c in t2.columns] == [c.name for c in t.columns]
    p = Tree(msg, presence=True)
    assert [f.optional for f in p.fields] == [True, True, True, False, False, False]
    assert all(len(f) == 5 for f in t.plain().to_fields())
    for bad in (Opt(Kind.ANY), Opt(ListOf(Kind.INT32)), Opt(Message("N", [("a", 1, Kind.INT32)]))):
        with pytest.raises(ValueError):
            Tree(Message("M", [("x", 1, bad)]))


# ---- the flag's validation ---------------------------------------------------------------------------

def _ctree(fields):
    """fields: (tag, kind, elem, parent, reserved)"""
    t = spec_amd._lib.SpecTree()
    t.nfields = len(fields)
    for i, (tag, kind, elem, parent, res) in enumerate(fields):
        t.fields[i].tag, t.fields[i].kind, t.fields[i].elem, t.fields[i].parent, t.fields[i].reserved = \
            tag, int(kind), int(elem), parent, res
    return t


OPT = FIELD_OPTIONAL
INVALID = {
    "on_message": [(1, Kind.MESSAGE, 0, -1, OPT), (1, Kind.INT32, 0, 0, 0)],
    "on_list": [(1, Kind.LIST, Kind.INT32, -1, OPT)],
    "on_message_list": [(1, Kind.LIST, Kind.MESSAGE, -1, OPT), (1, Kind.INT32, 0, 0, 0)],
    "on_any": [(1, Kind.ANY, 0, -1, OPT)],
    "on_struct_member": [(1, Kind.STRUCT, 0, -1, 0), (0, Kind.INT32, 0, 0, OPT)],
    "on_inner_struct": [(1, Kind.STRUCT, 0, -1, 0), (0, Kind.STRUCT, 0, 0, OPT), (0, Kind.INT32, 0, 1, 0)],
    "on_struct_list_member": [(1, Kind.LIST, Kind.STRUCT, -1, 0), (0, Kind.INT32, 0, 0, OPT)],
    "bit1": [(1, Kind.INT32, 0, -1, 2)],
    "bit1_and_flag": [(1, Kind.INT32, 0, -1, 3)],
    "bit15": [(1, Kind.INT32, 0, -1, 0x8000)],
    "bit8_on_message": [(1, Kind.MESSAGE, 0, -1, 0x100), (1, Kind.INT32, 0, 0, 0)],
    "other_bit_on_struct_member": [(1, Kind.STRUCT, 0, -1, 0), (0, Kind.INT32, 0, 0, 4)],
}
VALID = {
    "record_scalar": [(1, Kind.INT32, 0, -1, OPT)],
    "record_struct": [(1, Kind.STRUCT, 0, -1, OPT), (0, Kind.INT32, 0, 0, 0)],
    "sub_message_scalar": [(1, Kind.MESSAGE, 0, -1, 0), (1, Kind.STRING, 0, 0, OPT)],
    "list_item_scalar": [(1, Kind.LIST, Kind.MESSAGE, -1, 0), (1, Kind.BIN256, 0, 0, OPT)],
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_flag_refused_by_every_entry_point(case):
    """spec_tree_layout, spec_tree_decoder_create and spec_encode_tree answer
    SPEC_E_INVALID_ARGUMENT before any HIP call (this test runs without a GPU), and so does the
    compile entry point."""
    L = spec_amd.lib()
    t = _ctree(INVALID[case])
    nt, nc = C.c_uint32(0), C.c_uint32(0)
    assert L.spec_tree_layout(C.byref(t), None, C.byref(nt), None, C.byref(nc)) == SPEC_E_INVALID_ARGUMENT
    h = C.c_void_p()
    assert L.spec_tree_decoder_create(C.byref(t), C.byref(h)) == SPEC_E_INVALID_ARGUMENT and not h.value
    cols = (C.c_void_p * 8)()
    rows = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    ws = (C.c_uint8 * 64)()
    L.spec_encode_tree.restype = C.c_int
    rc = L.spec_encode_tree(C.byref(t), cols, None, None, rows, None, C.c_uint64(0), None, ws, C.c_size_t(64),
                            C.byref(total), None)
    assert rc == SPEC_E_INVALID_ARGUMENT
    L.spec_encode_tree_workspace_size.restype = C.c_size_t
    assert L.spec_encode_tree_workspace_size(C.byref(t), rows) == 0
    L.spec_tree_jit_compile.restype = C.c_longlong
    assert L.spec_tree_jit_compile(C.byref(t)) == SPEC_E_INVALID_ARGUMENT


@pytest.mark.parametrize("case", sorted(VALID))
def test_valid_flag_placements(case):
    L = spec_amd.lib()
    t = _ctree(VALID[case])
    T = (spec_amd._lib.SpecTreeTable * spec_amd._lib.SPEC_TREE_MAX_TABLES)()
    K = (spec_amd._lib.SpecTreeColumn * spec_amd._lib.SPEC_TREE_MAX_COLUMNS)()
    nt, nc = C.c_uint32(0), C.c_uint32(0)
    assert L.spec_tree_layout(C.byref(t), T, C.byref(nt), K, C.byref(nc)) == 0
    assert sum(1 for c in range(nc.value) if K[c].role == ROLE_HASMASK) == 1


# ---- the generated source ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_presence_trees_compile_for_gfx950(name):
    L = spec_amd.lib()
    L.spec_tree_jit_compile.restype = C.c_longlong
    assert L.spec_tree_jit_compile(C.byref(H.tree_of(name).c)) > 0


def test_unflagged_source_does_not_mention_the_column(tmp_path, monkeypatch):
    """The presence test of an optional field is a compile-time fact of the generated code: the
    source generated for unflagged pkg1_tree(2) has none of it, the presence tree's has."""
    import subprocess
    import sys

    def source(expr, tag):
        env = dict(os.environ, SPEC_AMD_JIT_DUMP=str(tmp_path / tag))
        code = ("import ctypes as C, spec_amd\n"
                f"t = {expr}\n"
                "L = spec_amd.lib()\nL.spec_tree_jit_compile.restype = C.c_longlong\n"
                "assert L.spec_tree_jit_compile(C.byref(t.c)) > 0\n")
        subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=os.path.dirname(os.path.dirname(__file__)))
        return open(str(tmp_path / tag) + "tree.hip").read()

    plain = source("spec_amd.pkg1_tree(2)", "plain_")
    for word in ("has_bit", " hw", "ro.has", "uint64_t has", "tree_rows_pair<2, true>"):
        assert word not in plain, word
    pres = source("__import__('tests.tree_presence_helpers').tree_presence_helpers.presence_small()", "pres_")
    for word in (" hw", "uint64_t has"):
        assert word in pres, word


# ---- the walker against references 1 and 2 -------------------------------------------------------------

N = 50


def _small(seed=11, has=0.5):
    tree = H.tree_of("presence_small")
    cols, heaps, rows = workload.tree_batch(tree, N, seed=seed, has=has, count=(0, 3))
    return tree, cols, heaps, rows


def test_walker_all_ones_is_the_plain_tree():
    tree, cols, heaps, rows = _small(has=1.0)
    for c in H.hasmask_columns(tree):
        nd = len(H.direct_fields(tree, c.table))
        assert nd < 64 and np.all(H.mask_of(cols, tree, c.table)[:, 0] >> np.uint64(nd) == 0)
    s, e = H.walk_encode(tree, cols, heaps, N)
    ws, we = oracle_encode(tree.plain(), cols, heaps, N)
    assert np.array_equal(s, ws) and np.array_equal(e, we)


UNIFORM = {
    "none": lambda t, k, f: False,
    "odd": lambda t, k, f: k % 2 == 1,
    "no_big_no_struct": lambda t, k, f: f.tag != 300 and f.kind != Kind.STRUCT,
}


@pytest.mark.parametrize("pattern", sorted(UNIFORM))
def test_walker_uniform_mask_is_the_pruned_tree(pattern):
    tree, cols, heaps, rows = _small(has=1.0)
    keep = UNIFORM[pattern]
    mcols = H.set_masks(tree, cols, keep)
    s, e = H.walk_encode(tree, mcols, heaps, N)
    ws, we = oracle_encode(H.pruned(tree, keep), mcols, heaps, N)
    assert np.array_equal(s, ws) and np.array_equal(e, we)
    assert s.size < oracle_encode(tree.plain(), cols, heaps, N)[0].size
    # the masks the walker reads back from those bytes are the ones that went in (live rows)
    got, live = H.walk_masks(tree, s, e, rows), H.live_rows(tree, mcols, rows)
    for x, m in got.items():
        assert np.array_equal(m, H.mask_of(mcols, tree, x) * live[x][:, None].astype(np.uint64)), x


def test_walker_mixed_masks_round_trip_through_the_oracle():
    """Mixed masks: the walker's masks of its own bytes are the input masks, and the oracle's decode
    of those bytes with the plain tree gives the input columns back (absent fields zero)."""
    from tests.tree_helpers import roundtrip_mismatches

    tree, cols, heaps, rows = _small(has=0.5)
    s, e = H.walk_encode(tree, cols, heaps, N)
    for x, m in H.walk_masks(tree, s, e, rows).items():
        assert np.array_equal(m, H.mask_of(cols, tree, x)), x
    got_rows, got = oracle_decode(tree.plain(), s, e)
    assert got_rows == rows
    assert roundtrip_mismatches(tree.plain(), cols, heaps, got, s) == []
    assert not np.array_equal(s, oracle_encode(tree.plain(), cols, heaps, N)[0])


def _handcrafted(end_of_i32):
    """One presence_small record written by the Writer with i32 = 5 and plain = 9, then the table
    entry of tag 1 patched to the given end offset."""
    w = O.Writer()
    w.message()
    w.field(1, "int32", 5)
    w.field(7, "int32", 9)
    rec, err = w.end()
    assert err is None
    rec = bytearray(rec)
    # small table: [tag u8, end u16 BE] x 2, then rvarint(data), rvarint(table), type
    t0 = len(rec) - 3 - 6
    assert rec[t0] == 1 and rec[t0 + 3] == 7
    rec[t0 + 1], rec[t0 + 2] = end_of_i32 >> 8, end_of_i32 & 0xff
    return bytes(rec)


def test_handcrafted_end_zero_is_present_and_end_past_data_is_absent():
    tree = H.tree_of("presence_small")
    k = [tree.fields[i].path for i in H.direct_fields(tree, 0)].index("i32")
    for end, bit in ((0, 1), (0xffff, 0)):
        rec = _handcrafted(end)
        m = O.Message(rec)
        assert m.err is None and m.has_field(1) == bool(bit) and m.get("int32", 1) == 0 and m.get("int32", 7) == 9
        s, e = np.frombuffer(rec, np.uint8), np.array([len(rec)], np.uint64)
        masks = H.walk_masks(tree, s, e, [1] + [0 if t.rel == 2 else 1 for t in tree.tables[1:]])
        assert (int(masks[0][0, 0]) >> k) & 1 == bit
        rows, got = oracle_decode(tree.plain(), s, e)
        plain = tree.plain()
        assert not np.any(got[plain.by_name["#errmask"].index]) and not np.any(got[plain.by_name["#status"].index])
        assert not np.any(got[plain.by_name["i32"].index])


# ---- the precompile list ----------------------------------------------------------------------------

def test_precompile_presence_list_is_current():
    """tests/golden/precompile_presence_trees.json holds exactly presence_test_trees(), and with
    pkg1_tree(2, presence=True) they are the last three trees build() precompiles."""
    d = json.load(open(PRESENCE_TREES_JSON))
    want = {k: [list(f) for f in t.to_fields()] for k, t in H.presence_test_trees().items()}
    assert d == want, "run tests/golden/make_precompile_presence_trees.py"
    pt = presence_trees()
    assert len(pt) == 3 and [t.to_fields() for t in precompiled_trees()[-3:]] == [t.to_fields() for t in pt]
    assert pt[0].to_fields() == H.tree_of("pkg1").to_fields()

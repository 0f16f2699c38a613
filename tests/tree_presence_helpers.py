"""Helpers of the schema-tree presence tests (SPEC_TREE_FIELD_OPTIONAL, the HASMASK column): the
test trees, and three references built on the committed oracle, which knows no HASMASK.

  1. the plain tree: T = T'.plain() (flags cleared).  Every non-HASMASK column of a decode with T'
     equals oracle_decode(T, ...); with all-ones masks the encode with T' equals oracle_encode(T, ...).
  2. the pruned tree: when every row of every table carries the same mask, the expected bytes are
     oracle_encode of the tree with the absent fields removed (pruned()).
  3. a record walker (walk_encode / walk_masks): expected bytes from the oracle's own Writer driven
     per record from the columns, an optional field skipped when its bit is clear; expected masks
     from oracle.Message(bytes).has_field(tag), walking sub-messages and list items in table row
     order.  tests/test_tree_presence.py pins the walker against 1 and 2 on the CPU.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from spec_amd.schema import Kind
from spec_amd.tree import REL_ONE, ROLE_HASMASK, ListOf, Message, Opt, Struct, Tree, pkg1_tree

SCALAR = lambda k: 1 <= int(k) <= 15  # noqa: E731


# ---- the trees -----------------------------------------------------------------------------------

def presence_small() -> Tree:
    """Optional scalars of several kinds, an optional struct with a string member, an optional
    field with tag 300 (a row's table is big exactly when it is written), a flagged and an unflagged
    field side by side, any, a sub-message and a message list with optional scalars, a value list,
    and a sub-message with nothing flagged (no HASMASK column)."""
    st = Struct("S", [("name", Kind.STRING), ("v", Kind.INT32)])
    sub = Message("Sub", [("a", 1, Opt(Kind.INT32)), ("t", 2, Opt(Kind.STRING)), ("c", 3, Kind.INT64)])
    item = Message("Item", [("x", 1, Opt(Kind.INT32)), ("y", 2, Opt(Kind.BYTES))])
    noflag = Message("NoFlag", [("p", 1, Kind.INT32), ("q", 2, Kind.STRING)])
    return Tree(Message("PresenceSmall", [
        ("i32", 1, Opt(Kind.INT32)), ("u64", 2, Opt(Kind.UINT64)), ("f64", 3, Opt(Kind.FLOAT64)),
        ("s", 4, Opt(Kind.STRING)), ("b128", 5, Opt(Kind.BIN128)), ("st", 6, Opt(st)),
        ("big", 300, Opt(Kind.INT16)), ("plain", 7, Kind.INT32), ("any", 8, Kind.ANY),
        ("sub", 9, sub), ("items", 10, ListOf(item)), ("vals", 11, ListOf(Kind.INT64)), ("nf", 12, noflag)]))


def presence_wide() -> Tree:
    """A record of 130 optional direct fields and a sub-message of 70: HASMASK of 3 and 2 words."""
    kinds = [Kind.INT32, Kind.UINT64, Kind.BOOL, Kind.STRING, Kind.FLOAT32, Kind.INT16, Kind.BIN64]
    sub = Message("WideSub", [(f"g{i}", i + 1, Opt(kinds[i % len(kinds)])) for i in range(70)])
    return Tree(Message("PresenceWide", [(f"f{i}", i + 1, Opt(kinds[i % len(kinds)])) for i in range(130)]
                        + [("sub", 131, sub)]))


def pkg1_presence() -> Tree:
    return pkg1_tree(2, presence=True)


def presence_test_trees() -> dict:
    """The test-only presence trees build() precompiles (tests/golden/precompile_presence_trees.json)."""
    return {"presence_small": presence_small(), "presence_wide": presence_wide()}


@functools.lru_cache(maxsize=None)
def tree_of(name: str) -> Tree:
    return {"presence_small": presence_small, "presence_wide": presence_wide, "pkg1": pkg1_presence}[name]()


# ---- the tree's shape ----------------------------------------------------------------------------

def direct_fields(tree: Tree, table: int) -> list:
    """Indices of the direct fields of a message table, in write order (bit k = the k-th)."""
    f = tree.tables[table].field
    return [i for i, g in enumerate(tree.fields) if g.parent == f]


def hasmask_columns(tree: Tree) -> list:
    return [c for c in tree.columns if c.role == ROLE_HASMASK]


def without_hasmask(tree: Tree, got: list) -> list:
    """Decoded columns (T' layout order) without the HASMASK ones: the plain tree's layout order."""
    return [g for c, g in zip(tree.columns, got) if c.role != ROLE_HASMASK]


def mask_of(cols: dict, tree: Tree, table: int) -> np.ndarray:
    """uint64 [rows, W] view of a table's HASMASK column in a column dict."""
    c = next(c for c in tree.tables[table].columns if c.role == ROLE_HASMASK)
    return np.ascontiguousarray(cols[c.name]).view(np.uint64).reshape(-1, c.width // 8)


def set_masks(tree: Tree, cols: dict, fn) -> dict:
    """A copy of cols with every optional field's bit set to fn(table, k, field) (a bool, the same in
    every row); the other bits stay."""
    out = dict(cols)
    for c in hasmask_columns(tree):
        m = np.ascontiguousarray(cols[c.name]).view(np.uint64).reshape(-1, c.width // 8).copy()
        for k, i in enumerate(direct_fields(tree, c.table)):
            if tree.fields[i].optional:
                bit = np.uint64(1) << np.uint64(k % 64)
                m[:, k // 64] = (m[:, k // 64] | bit) if fn(c.table, k, tree.fields[i]) else (m[:, k // 64] & ~bit)
        out[c.name] = m.view(np.uint8).reshape(-1, c.width)
    return out


def live_rows(tree: Tree, cols: dict, rows: list) -> dict:
    """{table: bool [rows]}: the rows an encode writes (a sub-message row is dead where its owner
    row is dead or has no such field; its mask is then ignored, and a decode reports 0)."""
    live = {0: np.ones(rows[0], bool)}
    for t in tree.tables[1:]:
        if t.rel == REL_ONE:
            pres = np.ascontiguousarray(cols[f"{tree.fields[t.field].path}?"]).reshape(-1).astype(bool)
            live[t.index] = pres & live[t.parent]
        else:
            live[t.index] = np.ones(rows[t.index], bool)
    return live


def pruned(tree: Tree, keep) -> Tree:
    """The plain tree without the optional fields (and their struct members) for which
    keep(table, k, field) is false; paths, hence column names, stay."""
    drop = set()
    for t in tree.tables:
        if t.shape != 0:
            continue
        for k, i in enumerate(direct_fields(tree, t.index)):
            if tree.fields[i].optional and not keep(t.index, k, tree.fields[i]):
                drop.add(i)
    remap, out = {-1: -1}, []
    for i, f in enumerate(tree.fields):
        if i in drop or f.parent in drop:
            drop.add(i)
            continue
        remap[i] = len(out)
        out.append((f.path, f.tag, int(f.kind), int(f.elem), remap[f.parent]))
    return Tree.from_fields(out)


# ---- the record walker ---------------------------------------------------------------------------

def _declare():
    L = O.lib()
    if getattr(L, "_presence_declared", False):
        return L
    pp = C.POINTER(C.c_void_p)
    L.so_field_value.restype = C.c_char_p
    L.so_field_value.argtypes = [C.c_void_p, C.c_uint16, C.c_int, C.c_void_p, C.c_void_p]
    L.so_elem_value.restype = C.c_char_p
    L.so_elem_value.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.so_field_struct_tree.restype = C.c_char_p
    L.so_field_struct_tree.argtypes = [C.c_void_p, C.c_uint16, C.c_int, C.c_int, C.c_void_p, pp, pp, C.POINTER(C.c_int)]
    L.so_elem_struct_tree.restype = C.c_char_p
    L.so_elem_struct_tree.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, pp, pp, C.POINTER(C.c_int)]
    L.so_field_any.restype = C.c_char_p
    L.so_field_any.argtypes = [C.c_void_p, C.c_uint16, C.c_void_p, C.c_size_t]
    L.so_message_field_raw.restype = C.c_void_p
    L.so_message_field_raw.argtypes = [C.POINTER(O.CMessage), C.c_uint16, C.POINTER(C.c_size_t)]
    L._presence_declared = True
    return L


class _Walk:
    """oracle/tree.c write_message restated over the oracle's Writer calls, with the HASMASK test."""

    def __init__(self, tree: Tree, cols: dict, heaps: dict):
        self.L = _declare()
        self.tree = tree
        self.cols = {k: np.ascontiguousarray(v) for k, v in cols.items() if v is not None}
        self.heaps = {k: np.ascontiguousarray(v, dtype=np.uint8) for k, v in heaps.items() if v is not None}
        self.direct = {t.index: direct_fields(tree, t.index) for t in tree.tables if t.shape == 0}
        self.table_of = {t.field: t.index for t in tree.tables if t.index}
        self.col_of = {}  # field -> its VALUE column name
        for c in tree.columns:
            if c.role == 0:
                self.col_of[c.field] = c.name
        self.mask = {c.table: self.cols[c.name].view(np.uint64).reshape(-1, c.width // 8) for c in hasmask_columns(tree)
                     if c.name in self.cols}
        self.w = O.Writer()

    def cell(self, name, row):
        a = self.cols[name]
        return a.ctypes.data + row * a.strides[0]

    def heap(self, name):
        h = self.heaps.get(name)
        return h.ctypes.data if h is not None else None

    def struct(self, sf, row, tag, field):
        f = self.tree.fields
        kinds, vals, hps, nmem = [], [], [], []

        def members(s):
            for j in range(s + 1, len(f)):
                if f[j].parent != s:
                    continue
                kinds.append(int(f[j].kind))
                if f[j].kind == Kind.STRUCT:
                    vals.append(None)
                    hps.append(None)
                    nmem.append(sum(1 for q in f if q.parent == j))
                    members(j)
                else:
                    nmem.append(0)
                    vals.append(self.cell(self.col_of[j], row))
                    hps.append(self.heap(self.col_of[j]))

        top = sum(1 for q in f if q.parent == sf)
        members(sf)
        nm = len(kinds)
        k = (C.c_uint8 * nm)(*kinds)
        v = (C.c_void_p * nm)(*vals)
        h = (C.c_void_p * nm)(*hps)
        n = (C.c_int * nm)(*nmem)
        if field:
            self.L.so_field_struct_tree(self.w.w, tag, top, nm, k, v, h, n)
        else:
            self.L.so_elem_struct_tree(self.w.w, top, nm, k, v, h, n)

    def message(self, x, row):
        L, w, f = self.L, self.w.w, self.tree.fields
        for k, i in enumerate(self.direct[x]):
            fi = f[i]
            if fi.optional and not (int(self.mask[x][row, k // 64]) >> (k % 64)) & 1:
                continue  # the setter was skipped
            if SCALAR(fi.kind):
                name = self.col_of[i]
                L.so_field_value(w, fi.tag, int(fi.kind), self.cell(name, row), self.heap(name))
            elif fi.kind == Kind.STRUCT:
                self.struct(i, row, fi.tag, True)
            elif fi.kind == Kind.ANY:
                name = self.col_of[i]
                off, ln = (int(v) for v in self.cols[name][row].view(np.uint32))
                if ln:
                    L.so_field_any(w, fi.tag, self.heaps[name].ctypes.data + off, ln)
            elif fi.kind == Kind.MESSAGE:
                if not self.cols[f"{fi.path}?"][row, 0]:
                    continue
                L.so_field_begin_message(w, fi.tag)
                self.message(self.table_of[i], row)
                L.so_writer_end(w, None, None)
            else:
                if not self.cols[f"{fi.path}?"][row, 0]:
                    continue
                y = self.table_of[i]
                b = self.cols[f"{fi.path}#begin"].view(np.uint32).reshape(-1)
                L.so_field_begin_list(w, fi.tag)
                for j in range(int(b[row]), int(b[row + 1])):
                    if fi.elem == Kind.MESSAGE:
                        L.so_elem_begin_message(w)
                        self.message(y, j)
                        L.so_writer_end(w, None, None)
                    elif fi.elem == Kind.STRUCT:
                        self.struct(i, j, 0, False)
                    else:
                        name = self.col_of[i]
                        L.so_elem_value(w, int(fi.elem), self.cell(name, j), self.heap(name))
                L.so_writer_end(w, None, None)

    def record(self, row) -> bytes:
        L = self.L
        L.so_writer_reset(self.w.w, self.w.buf)
        L.so_writer_begin_message(self.w.w)
        self.message(0, row)
        data, err = self.w.end()
        assert err is None, err
        return data


def walk_encode(tree: Tree, cols: dict, heaps: dict, n: int):
    """Reference 3, bytes: -> (stream uint8 [total], ends uint64 [n])."""
    wk = _Walk(tree, cols, heaps)
    recs = [wk.record(r) for r in range(n)]
    wk.w.close()
    ends = np.cumsum([len(r) for r in recs], dtype=np.uint64) if n else np.zeros(0, np.uint64)
    return np.frombuffer(b"".join(recs), np.uint8).copy(), ends


def walk_masks(tree: Tree, stream: np.ndarray, ends: np.ndarray, rows: list, root_only: bool = False) -> dict:
    """Reference 3, masks: {table: uint64 [rows, W]} for every table with a HASMASK column, from
    oracle.Message(bytes).has_field(tag), sub-messages and list items in table row order; zero where
    the message does not open (or the row's owner has no such field).  root_only: the records'
    table alone (fuzzed records, whose list tables a decoder may clamp)."""
    want = {c.table: np.zeros((rows[c.table], c.width // 8), np.uint64) for c in hasmask_columns(tree)}
    direct = {t.index: direct_fields(tree, t.index) for t in tree.tables if t.shape == 0}
    table_of = {t.field: t.index for t in tree.tables if t.index}
    nxt = [0] * len(tree.tables)  # next row of each list table
    f = tree.fields

    def visit(x, row, b):
        m = O.Message(b) if b else None
        ok = m is not None and m.err is None
        for k, i in enumerate(direct[x]):
            has = ok and m.has_field(f[i].tag)
            if has and x in want:
                want[x][row, k // 64] |= np.uint64(1) << np.uint64(k % 64)
            if root_only:
                continue
            if f[i].kind == Kind.MESSAGE:
                visit(table_of[i], row, _message_bytes(m, f[i].tag) if has else None)
            elif f[i].kind == Kind.LIST:
                y = table_of[i]
                items = m.list_items(f[i].tag) if has else []
                for it in items:
                    if f[i].elem == Kind.MESSAGE:
                        visit(y, nxt[y], it)
                    nxt[y] += 1

    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    for r in range(len(ends)):
        lo, hi = int(starts[r]), int(ends[r])
        visit(0, r, bytes(stream[lo:hi]) if hi > lo else b"")
    return want


def _message_bytes(m: "O.Message", tag: int):
    """m.FieldRaw(tag) = bytes[:end] (internal/types/msg.go:466-475): the sub-message is the value
    that ENDS there, which Message(tag) opens from its end."""
    L = _declare()
    ln = C.c_size_t(0)
    p = L.so_message_field_raw(C.byref(m.m), tag, C.byref(ln))
    return C.string_at(p, ln.value) if p and ln.value else b""


# ---- constructions shared with the tree tests (restated here: this file stands on its own) ---------

def to_dev(d: dict, dev):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items() if v is not None}


def fuzz(stream, ends, seed, n):
    """Mutated bytes (one in 200) and truncated records (one in 20, by up to 4 bytes)."""
    rng = np.random.default_rng(seed)
    s = stream.copy()
    k = max(1, s.size // 200)
    idx = rng.integers(0, s.size, k)
    s[idx] = rng.integers(0, 256, k, dtype=np.uint8)
    e = ends.copy()
    cut = rng.integers(0, n, n // 20)
    starts = np.concatenate([[0], e[:-1]])
    e[cut] = np.maximum(starts[cut], e[cut] - rng.integers(0, 5, cut.size).astype(np.uint64))
    return s, e


def root_windows(ends: np.ndarray, extra: int):
    """The root group's staging per 64-record window, restated from tree_decode.hip group_shape
    and tree_decode_core.hpp tree_rows_pair: the slab (0: no staging), and per window whether its
    span fits the slab (else both waves parse it from HBM) and, for the window holding the stream's
    last partial 16-byte chunk, which wave's 1 KiB DMA chunk it is in (that wave refills it)."""
    n, total = len(ends), int(ends[-1])
    slab = (int(64.0 * total / n * 1.15 + 128 + 64) + 1023) & ~1023
    if slab + extra > 40960:  # WAVE_LDS_MAX
        return 0, []
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    out = []
    for w in range((n + 63) // 64):
        lo, hi = int(starts[w * 64]), int(ends[min(n, w * 64 + 64) - 1])
        sb, se = max(lo - 64, 0) & ~15, (hi + 31) & ~15
        fits = se - sb + 16 <= slab
        tail, chunks = total & ~15, (se - sb + 1023) >> 10
        tw = ((tail - sb) >> 10) % 2 if fits and total % 16 and sb <= tail < sb + chunks * 1024 else None
        out.append((fits, tw))
    return slab, out

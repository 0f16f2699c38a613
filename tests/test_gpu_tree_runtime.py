"""Schema trees through BOTH implementations of every pass: the kernels generated per schema
(hiprtc) and the run-time kernels a tree drops to when the generated module is switched off or
fails to build (tree.hip tree_size_kernel / tree_write_kernel / tree_pos_fill_kernel,
tree_decode.hip tree_group_kernel), when a decode omits columns, or when a group has no generated
reader.  Every comparison is bit-exact against the oracle (oracle/tree.c).

  1. encode + decode parity under `kernel` = "jit" / "runtime": pkg1 at the wave, block and tile
     boundaries, every other tree of the tree tests, fuzzed records, cross-kind readers; the
     root group staged in LDS and parsed from HBM, asserted from the stream's sizes;
  2. decode with omitted columns (None entries): the present columns are the full decode's;
  3. the encoder writes only out[0, total) and ends[0, n): canaries around both, `out` at odd
     byte phases within a 16-byte chunk;
  4. the write pass at capacity - 1, on encoder errors, on list rows no owner places, and the
     run-time writer's refusal of a table too wide for its LDS;
  5. a tree, a flat and a nested schema in turn through the one cache of generated modules.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import spec_amd
from spec_amd import Kind, SpecError, workload
from spec_amd.tree import REL_MANY, ROLE_BEGIN, ROLE_STATUS, Message, Tree, TreeDecoder, TreeEncoder
from tests import test_gpu_tree as TG
from tests.test_gpu_tree import _fuzz, _root_windows, _spec_tree, to_dev
from tests.test_tree import _test_object_columns
from tests.tree_helpers import (mismatches, nested_struct_tree, oracle_decode, oracle_encode, roundtrip_mismatches,
                                shapes_tree)
from tests.trees import cross_kind_tree, levels_tree, many_tables_tree, wide_tree

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 257, 1000]  # the wave, TB = 256 and 64-record tile boundaries
CANARY, ECANARY = 0xA5, -0x5A5A5A5A5A5A5A5B
PHASES = [0, 1, 3, 8, 15]  # out.data_ptr() % 16
WAVE_LDS_MAX = 40960  # tree_decode.hip group_shape: the root group's LDS per wave
SPEC_E_TOO_LARGE = -3  # include/spec_amd.h


@pytest.fixture(params=["jit", "runtime"])
def kernel(request):
    """Run a test with the generated tree kernels (hiprtc) and with the run-time tree kernels.
    spec_encode_tree looks its kernels up per call; a TreeDecoder once, on its first pass, so
    every case builds its decoders after this has set the mode."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """A HIP error left behind by a test ends the session: nothing more is launched after it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU error after a tree run-time test: {e}", returncode=3)


# ---- batches and their oracle results, computed once and shared (never modified) --------------

BATCHES = {
    **{f"pkg1_n{n}": (lambda n=n: (spec_amd.pkg1_tree(), n, dict(seed=100 + n))) for n in NS},
    "pkg1_depth1": lambda: (spec_amd.pkg1_tree(1), 500, dict(seed=1, present=0.9)),
    "pkg1_depth3": lambda: (spec_amd.pkg1_tree(3), 500, dict(seed=3, present=0.9)),
    "pkg1_n300": lambda: (spec_amd.pkg1_tree(), 300, dict(seed=300)),
    "pkg1_n321": lambda: (spec_amd.pkg1_tree(), 321, dict(seed=321)),
    "pkg1_long_strings": lambda: (spec_amd.pkg1_tree(), 300, dict(seed=41, str_len=(100, 160))),
    "pkg1_tiles_over_image": lambda: (spec_amd.pkg1_tree(), 200, dict(seed=700, str_len=(0, 3000))),
    "shapes_big": lambda: (shapes_tree(), 60, dict(seed=9, count=(0, 300), str_len=(0, 70))),
    # the same list lengths (up to 300 elements: IsBigList by count) with most lists absent, for the
    # tests that encode or decode a batch many times: 0.8 M rows instead of 107 M
    "shapes_lists": lambda: (shapes_tree(), 60, dict(seed=9, count=(0, 300), present=0.15, str_len=(0, 70))),
    "shapes_small": lambda: (shapes_tree(), 1000, dict(seed=10, count=(0, 3))),
    "nested_n1": lambda: (nested_struct_tree(), 1, dict(seed=301)),
    "nested_n300": lambda: (nested_struct_tree(), 300, dict(seed=600)),
    "wide_n1": lambda: (wide_tree(), 1, dict(seed=501, count=(0, 3))),
    "wide_n65": lambda: (wide_tree(), 65, dict(seed=565, count=(0, 3))),
    "wide_n300": lambda: (wide_tree(), 300, dict(seed=800, count=(0, 3))),
    "many_tables_n1": lambda: (many_tables_tree(), 1, dict(seed=701, count=(0, 3))),
    "many_tables_n300": lambda: (many_tables_tree(), 300, dict(seed=1000, count=(0, 3))),
    "levels_n257": lambda: (levels_tree(), 257, dict(seed=257)),
    "levels_no_lists": lambda: (levels_tree(), 257, dict(seed=257, count=(0, 0))),
    **{f"spec_{name}": (lambda name=name: (_spec_tree(name), 300, dict(seed=77, count=(0, 3))))
       for name in ["pkg1.Message", "pmpx.Message", "prpc.Message", "pmpx.ChannelOpen"]},
}


@functools.lru_cache(maxsize=None)
def batch(name):
    """The named batch with the oracle's encoding and the oracle's decode of it."""
    if name == "test_object":
        tree, n = spec_amd.pkg1_tree(), 1
        cols, heaps = _test_object_columns(tree)
        rows = spec_amd.tree_rows(tree, 1, cols)
    else:
        tree, n, kw = BATCHES[name]()
        cols, heaps, rows = workload.tree_batch(tree, n, **kw)
    stream, ends = oracle_encode(tree, cols, heaps, n)
    want_rows, want = oracle_decode(tree, stream, ends)
    return SimpleNamespace(tree=tree, n=n, cols=cols, heaps=heaps, rows=rows, stream=stream, ends=ends,
                           want_rows=want_rows, want=want)


def decode_fresh(tree, stream, ends, dev):
    """A new TreeDecoder's index + decode of (stream, ends): rows, columns as numpy."""
    return TG.gpu_decode(tree, stream, ends, dev)


def check_encode_decode(b, dev):
    """tests/test_gpu_tree.py check_encode_decode over a shared batch."""
    stream, ends = spec_amd.encode_tree(b.tree, to_dev(b.cols, dev), to_dev(b.heaps, dev), b.n, rows=b.rows)
    torch.cuda.synchronize()
    assert np.array_equal(ends.cpu().numpy().view(np.uint64), b.ends), "ends"
    got_stream = stream.cpu().numpy()
    if not np.array_equal(got_stream, b.stream):
        j = int(np.nonzero(got_stream != b.stream)[0][0]) if got_stream.size == b.stream.size else -1
        raise AssertionError(f"encoded bytes: {got_stream.size} bytes, oracle {b.stream.size}, first difference at {j}")
    got_rows, got = decode_fresh(b.tree, b.stream, b.ends, dev)
    assert got_rows == b.want_rows == b.rows
    assert mismatches(b.tree, got, b.want) == []
    assert roundtrip_mismatches(b.tree, b.cols, b.heaps, got, b.stream) == []


def group_tables(tree, x):
    """Tables decoded in the group of root x (tree.hip build_layout: a sub-message table joins its
    owner's group, a list table starts its own)."""
    root = {}
    for t in tree.tables:
        root[t.index] = t.index if t.index == 0 or t.rel == REL_MANY else root[t.parent]
    return [t.index for t in tree.tables if root[t.index] == x]


def root_slab(tree, ends):
    """(slab, extra) of the root group, restated from tree_decode.hip group_shape: the staging
    slab it asks for and its range slots; staged iff slab + extra <= WAVE_LDS_MAX."""
    n, total = len(ends), int(ends[-1])
    slab = (int(64.0 * total / n * 1.15 + 128 + 64) + 1023) & ~1023
    return slab, 512 * (len(group_tables(tree, 0)) - 1) + 16


def direct_fields(tree, table):
    """Direct fields of a message table (TTable.nd)."""
    f = tree.tables[table].field
    return sum(1 for g in tree.fields if g.parent == f)


# ---- 1. parity under both kernels --------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_pkg1_encode_decode(dev, kernel, n):
    """(first in the file: one record through the run-time encoder, then its decode, before
    anything wider)"""
    check_encode_decode(batch(f"pkg1_n{n}"), dev)


@pytest.mark.parametrize("name", ["pkg1_depth1", "pkg1_depth3", "test_object", "shapes_big", "shapes_small",
                                  "nested_n1", "nested_n300", "many_tables_n1", "many_tables_n300",
                                  "spec_pkg1.Message", "spec_pmpx.Message", "spec_prpc.Message",
                                  "spec_pmpx.ChannelOpen"])
def test_trees_encode_decode(dev, kernel, name):
    b = batch(name)
    if name == "shapes_big":
        assert max(b.rows) > 255  # big lists (IsBigList by count)
    if name.startswith("many_tables"):
        assert len(group_tables(b.tree, 0)) > 24  # no generated reader (jit_tree.cpp tree_group_ok) ...
        assert root_slab(b.tree, b.ends)[1] > WAVE_LDS_MAX  # ... and its range slots alone pass a wave's LDS
    check_encode_decode(b, dev)


@pytest.mark.parametrize("n", [1, 300])
def test_wide_encode_decode(dev, kernel, n):
    """wide_tree's root has more than 64 direct fields: no generated reader for its group
    (jit_tree.cpp tree_table_ok), no record-tile writer (tree_tile) — under "jit" the decode runs the
    run-time group kernel and the encode the level-fused generated writer.  Its records are too
    long for a staging slab: the run-time group kernel parses them from HBM."""
    b = batch(f"wide_n{n}")
    assert direct_fields(b.tree, 0) > 64
    slab, extra = root_slab(b.tree, b.ends)
    assert slab + extra > WAVE_LDS_MAX  # unstaged: GlobalSrc
    check_encode_decode(b, dev)


def test_empty_batch(dev, kernel):
    tree = spec_amd.pkg1_tree()
    rows, _ = decode_fresh(tree, np.zeros(0, np.uint8), np.zeros(0, np.uint64), dev)
    assert rows == [0] * len(tree.tables)
    # encode: BEGIN columns hold their closing entry, nothing else has rows
    cols = {c.name: torch.zeros((1, 4), dtype=torch.uint8, device=dev) for c in tree.columns if c.role == ROLE_BEGIN}
    enc = TreeEncoder(tree, [0] * len(tree.tables), dev)
    enc.total.fill_(-7)
    assert int(enc.encode(cols, {}, None, None).item()) == 0
    buf = torch.full((128,), CANARY, dtype=torch.uint8, device=dev)
    ebuf = torch.full((16,), ECANARY, dtype=torch.int64, device=dev)
    enc.total.fill_(-7)
    assert int(enc.encode(cols, {}, buf[64:64], ebuf[8:8]).item()) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all() and (ebuf.cpu().numpy() == ECANARY).all()


def test_one_decoder_over_full_empty_and_listless_batches(dev, kernel):
    """One TreeDecoder through batches in turn: 257 records of levels_tree (a 256-thread block and
    one row; two tables at one height and at one depth), no records, the same records with every
    list empty, the first batch again.  Each pass is the oracle's: no row count or column carries
    over from the pass before.  (An encode of no records: test_empty_batch.)"""
    full, bare = batch("levels_n257"), batch("levels_no_lists")
    tree, n = full.tree, full.n
    lists = [t.index for t in tree.tables if t.rel == REL_MANY]
    assert len(tree.tables) == 4 and len(lists) == 2 and min(full.rows) > 0
    assert [bare.rows[x] for x in lists] == [0, 0]
    check_encode_decode(full, dev)

    def put(b):
        s = torch.from_numpy(b.stream if b.stream.size else np.zeros(1, np.uint8)).to(dev)[: b.stream.size]
        return s, torch.from_numpy(b.ends.view(np.int64)).to(dev)

    d = TreeDecoder(tree)
    s_full, e_full = put(full)
    d.index(s_full, e_full)
    cols = d.alloc(dev)

    def run(s, e, want_rows, want):
        for c in cols:
            c.fill_(CANARY)
        rows_out = d.run(s, e, cols)
        torch.cuda.synchronize()
        assert rows_out.cpu().tolist() == want_rows
        got = [c[: tree.column_rows(tc, want_rows)].cpu().numpy() for c, tc in zip(cols, tree.columns)]
        assert want is None or mismatches(tree, got, want) == []
        return [c.cpu().numpy() for c in cols]

    first = run(s_full, e_full, full.want_rows, full.want)
    # no records: no scan runs, the device row counts are reset (run()'s memset of rowsd): every
    # count 0, no column written
    after = run(s_full[:0], e_full[:0], [0] * len(tree.tables), None)
    assert all((a == CANARY).all() for a in after)
    # every list empty: every group has capacity from the index above, so the zeros come from the
    # scans; the list tables (and the sub-message table under the items) have no rows
    assert bare.want_rows == [n, 0, 0, 0]
    run(*put(bare), bare.want_rows, bare.want)
    again = run(s_full, e_full, full.want_rows, full.want)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_pkg1_root_staged_and_unstaged(dev, kernel):
    """The root group from LDS and from HBM, known from the streams' sizes: pkg1 at 1,000 records
    is staged with every 64-record window inside the slab (under "runtime": tree_group_kernel
    over TreeLds), the same tree with long strings is not (GlobalSrc)."""
    staged, unstaged = batch("pkg1_n1000"), batch("pkg1_long_strings")
    slab, extra = root_slab(staged.tree, staged.ends)
    assert slab + extra <= WAVE_LDS_MAX
    got_slab, windows = _root_windows(staged.ends, extra)
    assert got_slab == slab and all(fits for fits, _ in windows)
    slab, extra = root_slab(unstaged.tree, unstaged.ends)
    assert slab + extra > WAVE_LDS_MAX
    for b in (staged, unstaged):
        check_encode_decode(b, dev)


FUZZ_TREES = {"pkg1": spec_amd.pkg1_tree, "shapes": shapes_tree, "nested_struct": nested_struct_tree}


@functools.lru_cache(maxsize=None)
def fuzzed(which, seed):
    tree, n = FUZZ_TREES[which](), 1000
    cols, heaps, _ = workload.tree_batch(tree, n, 900 + seed, count=(0, 4))
    s, e = _fuzz(*oracle_encode(tree, cols, heaps, n), 20 + seed, n)
    return tree, s, e, oracle_decode(tree, s, e)


@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("which", list(FUZZ_TREES))
def test_fuzzed_records(dev, kernel, which, seed):
    """Mutated, truncated and garbage records: every status class, panics and nil elements
    through the run-time reader — rows and every column the oracle's."""
    tree, s, e, (want_rows, want) = fuzzed(which, seed)
    assert any(np.any(w) for c, w in zip(tree.columns, want) if c.role == ROLE_STATUS)
    got_rows, got = decode_fresh(tree, s, e, dev)
    assert got_rows == want_rows
    assert mismatches(tree, got, want) == []


@functools.lru_cache(maxsize=None)
def cross_kind(shift):
    b = batch("pkg1_n300")
    reader = cross_kind_tree(shift)
    streams = [(b.stream, b.ends), _fuzz(b.stream, b.ends, shift, b.n)]
    return reader, [(s, e, oracle_decode(reader, s, e)) for s, e in streams]


@pytest.mark.parametrize("shift", [1, 4, 9])
def test_errmask_cross_kind(dev, kernel, shift):
    """test_gpu_tree.py test_errmask_cross_kind's readers: pkg1's records read with every scalar
    getter shifted to another kind, clean and fuzzed — ERRMASK and every column the oracle's."""
    reader, streams = cross_kind(shift)
    for s, e, (want_rows, want) in streams:
        got_rows, got = decode_fresh(reader, s, e, dev)
        assert got_rows == want_rows
        assert mismatches(reader, got, want) == []
    assert any(np.any(w) for c, w in zip(reader.columns, want) if c.name.endswith("#errmask"))


# ---- 2. decode with omitted columns --------------------------------------------------------------

def keep_third(tree):
    return [c.role in (ROLE_BEGIN, ROLE_STATUS) or c.index % 3 != 2 for c in tree.columns]


def keep_begin_status(tree):
    return [c.role in (ROLE_BEGIN, ROLE_STATUS) for c in tree.columns]


@pytest.mark.parametrize("name", ["pkg1_n257", "shapes_lists"])
def test_decode_with_omitted_columns(dev, kernel, name):
    """None entries in decode() / run(): the columns that are present equal the full decode's byte
    for byte (and the oracle's), the rows are the indexed rows.  Under "jit" a decoder that holds
    generated kernels switches to the run-time group kernel for such a call."""
    b = batch(name)
    tree = b.tree
    s = torch.from_numpy(b.stream).to(dev)
    e = torch.from_numpy(b.ends.view(np.int64)).to(dev)
    d = TreeDecoder(tree)
    assert d.index(s, e) == b.want_rows
    full = [c.cpu().numpy() for c in d.decode().cols]
    assert mismatches(tree, full, b.want) == []
    for keep in (keep_third(tree), keep_begin_status(tree)):
        assert not all(keep) and any(keep)
        # decode(): a decoder of its own, columns pre-filled so an unwritten one shows
        d1 = TreeDecoder(tree)
        assert d1.index(s, e) == b.want_rows
        cols = [c.fill_(CANARY) if k else None for c, k in zip(d1.alloc(dev), keep)]
        out = d1.decode(cols)
        torch.cuda.synchronize()
        assert out.rows == b.want_rows
        for c, k, g, w in zip(tree.columns, keep, out.cols, full):
            assert (g is None) == (not k), c.name
            if k:
                assert np.array_equal(g.cpu().numpy(), w), c.name
        # run(): through column_capacity (a None entry does not limit its table)
        d2 = TreeDecoder(tree)
        d2.index(s, e)
        cols = [c.fill_(CANARY) if k else None for c, k in zip(d2.alloc(dev), keep)]
        assert d2.column_capacity(cols) == [max(r, 1) for r in b.want_rows]  # what the present columns hold
        rows_out = d2.run(s, e, cols).cpu().numpy()
        assert list(rows_out) == b.want_rows
        for c, k, g, w in zip(tree.columns, keep, cols, full):
            if k:
                assert np.array_equal(g[: tree.column_rows(c, b.want_rows)].cpu().numpy(), w), c.name


# ---- 3. the encoder writes only out[0, total) and ends[0, n) -----------------------------------

class Canaried:
    """An output buffer at byte phase `phase` of a 16-byte chunk and an ends tensor, both inside
    canary-filled allocations (at least 64 bytes / 8 words on each side)."""

    def __init__(self, dev, nbytes, n, phase):
        self.buf = torch.full((64 + 16 + nbytes + 64,), CANARY, dtype=torch.uint8, device=dev)
        self.off = 64 + (phase - (self.buf.data_ptr() + 64)) % 16
        self.nbytes, self.n = nbytes, n
        self.out = self.buf[self.off: self.off + nbytes]
        assert self.out.data_ptr() % 16 == phase
        self.ebuf = torch.full((n + 16,), ECANARY, dtype=torch.int64, device=dev)
        self.ends = self.ebuf[8: 8 + n]

    def assert_outside_intact(self, label):
        whole, ewhole = self.buf.cpu().numpy(), self.ebuf.cpu().numpy()
        assert (whole[: self.off] == CANARY).all(), f"{label}: bytes before out[0] written"
        assert (whole[self.off + self.nbytes:] == CANARY).all(), f"{label}: bytes past out[total) written"
        assert (ewhole[:8] == ECANARY).all() and (ewhole[8 + self.n:] == ECANARY).all(), f"{label}: ends overrun"

    def assert_untouched(self, label):
        assert (self.buf.cpu().numpy() == CANARY).all(), f"{label}: output written"
        assert (self.ebuf.cpu().numpy() == ECANARY).all(), f"{label}: ends written"


def assert_written(c, b, label):
    """The canaried output holds the oracle's bytes and ends, and nothing else was written."""
    assert np.array_equal(c.ends.cpu().numpy().view(np.uint64), b.ends), f"{label}: ends"
    got = c.out.cpu().numpy()
    if not np.array_equal(got, b.stream):
        j = int(np.nonzero(got != b.stream)[0][0])
        i = int(np.searchsorted(b.ends, j, side="right"))
        raise AssertionError(f"{label}: byte {j} (record {i}) gpu={got[j]:#x} want={b.stream[j]:#x}")
    c.assert_outside_intact(label)


@pytest.mark.parametrize("name", ["pkg1_n1", "pkg1_n65", "pkg1_n321", "pkg1_tiles_over_image", "shapes_lists",
                                  "wide_n65"])
def test_encoder_writes_only_its_output(dev, kernel, name):
    """spec_encode_tree's size call (out = null) and write call into canaried buffers, `out` at
    five byte phases of a 16-byte chunk: the oracle's bytes and ends, *total right, every canary
    intact.  pkg1: the record-tile writer (an LDS image stored with 16-byte stores; five tiles
    with a ragged last one at 321 records; tiles over the image with 3,000-byte strings);
    wide_tree: the level-fused writer (BEmit16 / BEmit); "runtime": tree_write_kernel's BEmit."""
    b = batch(name)
    if name == "pkg1_tiles_over_image":
        starts = np.concatenate([[0], b.ends[:-1]]).astype(np.int64)
        assert max(int(b.ends[min(b.n, t + 64) - 1]) - int(starts[t]) for t in range(0, b.n, 64)) > 72 * 1024
    if name == "wide_n65":
        assert direct_fields(b.tree, 0) > 64  # tree_tile() false
    if name == "shapes_lists":
        begin = b.cols["items[].leaves#begin"].reshape(-1).view(np.uint32).astype(np.int64)
        assert np.diff(begin).max() > 255 and max(b.rows) > 255  # big lists by count
    d_cols, d_heaps = to_dev(b.cols, dev), to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    enc.total.fill_(-7)
    assert int(enc.encode(d_cols, d_heaps, None, None).item()) == b.stream.size, "size pass"
    for phase in PHASES:
        label = f"{name} {kernel} phase {phase}"
        c = Canaried(dev, b.stream.size, b.n, phase)
        enc.total.fill_(-7)
        enc.encode(d_cols, d_heaps, c.out, c.ends)
        torch.cuda.synchronize()
        assert int(enc.total.item()) == b.stream.size, f"{label}: *total"
        assert_written(c, b, label)


# ---- 4. capacity and errors on the write pass -----------------------------------------------------

@pytest.mark.parametrize("name", ["pkg1_n300", "shapes_lists"])
def test_encode_capacity_one_short(dev, kernel, name):
    """out_cap = total - 1: *total still reports the size, no byte of the buffer and no word of
    ends changes."""
    b = batch(name)
    d_cols, d_heaps = to_dev(b.cols, dev), to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    for phase in (0, 3):
        c = Canaried(dev, b.stream.size - 1, b.n, phase)
        enc.total.fill_(-7)
        enc.encode(d_cols, d_heaps, c.out, c.ends)
        torch.cuda.synchronize()
        assert int(enc.total.item()) == b.stream.size
        c.assert_untouched(f"{name} {kernel} phase {phase}")


BAD_SPAN_COLUMNS = {"pkg1_n300": ["string", "strings[]", "submessages[].value"],
                    "shapes_lists": ["big.any", "items[].name", "cs[].string"]}


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("name", ["pkg1_n300", "shapes_lists"])
def test_encode_span_outside_heap(dev, kernel, name, which):
    """One row's string / bytes / any span starting one past its heap's end, in a column of a
    one-row-per-record table and in list-item columns: the write call leaves *total all-ones and
    writes nothing; the same TreeEncoder then writes the oracle's bytes from the good columns."""
    b = batch(name)
    col = BAD_SPAN_COLUMNS[name][which]
    tc = b.tree.column(col)
    assert tc.kind in (Kind.STRING, Kind.BYTES, Kind.ANY)
    assert (b.tree.tables[tc.table].rel == REL_MANY) == (which > 0)
    sp = b.cols[col].copy().view(np.uint32).reshape(-1, 2)
    row = int(np.argmax(sp[:, 1] > 0))  # a row with bytes (row 0 if none has)
    sp[row, 0] = b.heaps[col].size + 1
    bad = dict(b.cols)
    bad[col] = sp.view(np.uint8).reshape(-1, 8)
    d_heaps = to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    c = Canaried(dev, b.stream.size, b.n, 1)
    enc.total.fill_(-7)
    enc.encode(to_dev(bad, dev), d_heaps, c.out, c.ends)
    torch.cuda.synchronize()
    assert int(enc.total.item()) == -1
    c.assert_untouched(f"{name} {kernel} {col}")
    enc.total.fill_(-7)
    enc.encode(to_dev(b.cols, dev), d_heaps, c.out, c.ends)
    torch.cuda.synchronize()
    assert int(enc.total.item()) == b.stream.size
    assert_written(c, b, f"{name} {kernel} after the error")


@pytest.mark.parametrize("which", ["pkg1_3", "shapes"])
def test_encode_list_rows_outside_owner_ranges(dev, kernel, which):
    """test_gpu_tree.py's test of child rows no owner places, under both kernels: on the
    run-time path tree_pos_fill_kernel marks every child row unplaced and tree_write_kernel
    skips the rows still marked."""
    TG.test_encode_list_rows_outside_owner_ranges(dev, which)


@functools.lru_cache(maxsize=None)
def very_wide():
    """A record of 641 scalar fields: one more than tree_write_kernel's LDS field ends hold
    (256 B per field per wave, 160 KiB).  Only ever run with the generated kernels off."""
    tree = Tree(Message("VeryWide", [(f"f{i}", i + 1, Kind.INT32) for i in range(641)]))
    cols, heaps, rows = workload.tree_batch(tree, 3, 5)
    stream, ends = oracle_encode(tree, cols, heaps, 3)
    return SimpleNamespace(tree=tree, n=3, cols=cols, heaps=heaps, rows=rows, stream=stream, ends=ends)


def test_runtime_writer_refuses_a_table_too_wide(dev):
    """With the generated kernels off, a record table of more than 640 direct fields sizes
    (out = null) without error, and its write call returns SPEC_E_TOO_LARGE before anything is
    issued: *total and out are unchanged after a device synchronise."""
    b = very_wide()
    assert direct_fields(b.tree, 0) == 641
    spec_amd.set_jit(False)
    try:
        d_cols, d_heaps = to_dev(b.cols, dev), to_dev(b.heaps, dev)
        enc = TreeEncoder(b.tree, b.rows, dev)
        assert int(enc.encode(d_cols, d_heaps, None, None).item()) == b.stream.size
        c = Canaried(dev, b.stream.size, b.n, 0)
        enc.total.fill_(0x1234)
        with pytest.raises(SpecError) as err:
            enc.encode(d_cols, d_heaps, c.out, c.ends)
        assert err.value.rc == SPEC_E_TOO_LARGE
        torch.cuda.synchronize()
        assert int(enc.total.item()) == 0x1234
        c.assert_untouched("641 fields")
    finally:
        spec_amd.set_jit(True)


# ---- 5. several programs through the one module cache (jit_module.cpp) -------------------------

def test_programs_share_one_module_cache(dev, capfd):
    """A precompiled tree, FLAT16, NESTED and the same tree again, decode and encode each, in one
    process with the generated kernels on: all five programs' modules go through the one cache
    (jit_module.cpp find_module) and each keeps its own kernels.  65 records: a full 64-record
    group and a one-record tail.  Every step against the oracle; the tree's second run equals its
    first array for array.  The specialised kernels are the ones that ran: every module compiles
    (or is read from the code-object cache), the flat launches answer for themselves
    (require_specialised), and no module printed the cache's "compile/load failed" line."""
    import ctypes as C

    from oracle import oracle as O
    from spec_amd.tree_catalog import precompiled_trees
    from tests import gpu_helpers as G
    from tests.test_gpu_nested import check_nested, nested_device_inputs

    n = 65
    spec_amd.set_jit(True)
    L = spec_amd.lib()
    tree = precompiled_trees()[1]
    cols, heaps, rows = workload.tree_batch(tree, n, seed=165)
    want_stream, want_ends = oracle_encode(tree, cols, heaps, n)
    want_rows, want = oracle_decode(tree, want_stream, want_ends)

    def run_tree():
        assert L.spec_tree_jit_compile(C.byref(tree.c)) > 0
        stream, ends = spec_amd.encode_tree(tree, to_dev(cols, dev), to_dev(heaps, dev), n, rows=rows)
        torch.cuda.synchronize()
        stream, ends = stream.cpu().numpy(), ends.cpu().numpy().view(np.uint64)
        assert np.array_equal(ends, want_ends) and np.array_equal(stream, want_stream)
        got_rows, got = decode_fresh(tree, want_stream, want_ends, dev)
        assert got_rows == want_rows == rows
        assert mismatches(tree, got, want) == []
        return [stream, ends, np.array(got_rows)] + [g for g in got if g is not None]

    first = run_tree()

    flat = spec_amd.FLAT16
    fcols, fheaps = workload.flat16(n, seed=65)
    fstream, fends = G.oracle_encode(flat, fcols, fheaps, n)
    G.require_specialised(flat, "FLAT16", decode=(fstream.size, n), encode=True)
    G.check_decode(dev, flat, fstream, fends, "FLAT16 between trees")
    G.check_encode(dev, flat, fcols, fheaps, n, "FLAT16 between trees")

    w = workload.nested(n, seed=65, count=(1, 4))
    counts = np.diff(w["item_begin"]).astype(np.int64)
    counts[3], counts[10] = 0, 70  # an empty list, and one of more than a wave's 64 items
    rng = np.random.default_rng(65)
    m = int(counts.sum())
    ib = np.zeros(n + 1, np.uint32)
    np.cumsum(counts, out=ib[1:])
    lens = rng.integers(0, 12, m).astype(np.uint32)
    label = np.zeros((m, 2), np.uint32)
    label[1:, 0] = np.cumsum(lens[:-1])
    label[:, 1] = lens
    w.update(item_begin=ib, key=rng.integers(-2**31, 2**31, m).astype(np.int32), value=rng.standard_normal(m),
             label=label, label_heap=rng.integers(32, 127, int(lens.sum()), dtype=np.uint8))
    assert L.spec_decode_nested_jit_compile(C.byref(spec_amd.NESTED.c)) > 0
    assert L.spec_encode_nested_jit_compile(C.byref(spec_amd.NESTED.c)) > 0
    nstream, nends = O.encode_nested_batch(w)
    oc, oh, ibd, ic, ih = nested_device_inputs(w, dev)
    out, ends = spec_amd.encode_nested(spec_amd.NESTED, oc, oh, ibd, ic, ih, n)
    torch.cuda.synchronize()
    assert np.array_equal(ends.cpu().numpy().view(np.uint64), nends) and np.array_equal(out.cpu().numpy(), nstream)
    check_nested(dev, nstream, nends, "NESTED between trees", modes=("twopass-xcd", "onepass"))

    again = run_tree()
    assert len(first) == len(again) and all(np.array_equal(a, b) for a, b in zip(first, again))
    assert "spec_amd jit:" not in capfd.readouterr().err

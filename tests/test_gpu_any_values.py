"""Typed values of `any` fields on the GPU: the catalog of tests/any_values.py (every type of
DecodeTypeSize's switch, well-formed and malformed, alone in its slot and behind junk; checked
against the oracle on the CPU by tests/test_any_values.py) through every kernel that opens or
reads such a value.

  1. spec_decode_values (tree_decode.hip values_kernel): every reader kind over every entry ==
     the oracle bit for bit; every (reader, scalar entry) pair == the reference's rules stated
     apart from the oracle (any_values.expect_read); spans at and past the stream's end, empty
     spans, streams at odd addresses; one call of more rows than a pass of the grid.
  2. `any` fields of four trees through the tree encoder and decoder, under the generated and the
     run-time kernels (tree_core.hpp type_size_inl; the K_ANY case of tree_decode_core.hpp
     tree_message_row_inl and of jit_tree.cpp's generated readers), as a stream and as mpx frames.
  3. spec_tree_decoder_index_spans (Value.Message()) over messages, other values, malformed
     values, empty spans and spans past the stream, under both kernels.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import Kind, workload
from spec_amd.tree import ROLE_ERRMASK, ROLE_STATUS, TreeDecoder
from tests import any_values as A
from tests.test_gpu_decode_tree_frames import framed, want_over_spans
from tests.test_gpu_tree import to_dev
from tests.test_gpu_tree_runtime import WAVE_LDS_MAX, check_encode_decode, decode_fresh, root_slab
from tests.tree_helpers import mismatches, oracle_decode, oracle_encode, oracle_fields, shapes_tree, span_bytes
from tests.trees import any_first_tree, message1_tree, wide_tree

pytestmark = pytest.mark.gpu

ST_PANIC = 6
KINDS = [Kind(k) for k in range(1, 16)]


@pytest.fixture(params=["jit", "runtime"])
def kernel(request):
    """The generated tree kernels (hiprtc) and the run-time tree kernels; a TreeDecoder looks its
    kernels up on its first pass, so every case builds its decoders after this has set the mode."""
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
        pytest.exit(f"GPU error after an any-value test: {e}", returncode=3)


def to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def gpu_values(kind, d_stream, spans, dev):
    v, e = spec_amd.decode_values(kind, d_stream, to(spans, dev))
    torch.cuda.synchronize()
    return v.cpu().numpy(), e.cpu().numpy()


# ---- 1. spec_decode_values ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def value_spans():
    """All placements' slots back to back, and one span per placement: the value where the slot
    opens as one (OpenValue's span), the whole slot where it does not (what a caller holding the raw
    field would read)."""
    pls = A.placements()
    heap, spans = A.heap_and_spans(pls)
    for j, p in enumerate(pls):
        if p.cls == "ok":
            spans[j] = (spans[j, 0] + p.off, p.size)
    return heap, spans


@functools.lru_cache(maxsize=None)
def matrix():
    """The catalog three times over, shuffled: more than a block of rows, not a multiple of one."""
    heap, spans = value_spans()
    rows = np.random.default_rng(7).permutation(np.tile(np.arange(len(spans)), 3))
    assert len(rows) > 256 and len(rows) % 256 and len(rows) < 4000
    return heap, np.ascontiguousarray(spans[rows])


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_values_matrix(dev, kind):
    """Value.<Kind>Err() of every catalog entry and placement, for every reader kind: values and
    errs are the oracle's bit for bit."""
    heap, spans = matrix()
    want_v, want_e = O.decode_values(kind, heap, spans)
    got_v, got_e = gpu_values(kind, to(heap, dev), spans, dev)
    assert want_e.any() and not want_e.all() or kind == Kind.BOOL  # both outcomes occur (Bool() never errs)
    assert np.array_equal(got_e, want_e)
    assert np.array_equal(got_v, want_v)


def test_values_by_the_reference_rules(dev):
    """Every ok scalar entry, alone and behind junk, through every reader: err and value as the
    reference's decoders define them for that pair, stated without the oracle (the entry's Python
    value; floats by bit pattern; string / bytes as absolute stream spans over the payload)."""
    cache = {}

    def read(kind, heap, spans):
        if "s" not in cache:
            cache["s"] = to(heap, dev)
        return gpu_values(kind, cache["s"], spans, dev)

    assert A.check_reads(read) > 14 * len(A.scalars())


def test_values_span_edges(dev):
    """Spans at the stream's edges: ending exactly at stream_len (read), one byte past it and
    (0xFFFFFFFF, 0xFFFFFFFF) (err 2: off + len does not wrap in 32 bits), empty spans (a nil value:
    zero, no error) — and the same stream as a view 1 and 15 bytes into its allocation."""
    cat = {e.name: e.data for e in A.catalog()}
    names = ["int64_m1", "string_127", "float64_max", "bytes_128", "bin256", "uint16_65535", "string_1"]
    stream = np.frombuffer(b"".join(cat[k] for k in names), np.uint8).copy()
    ends = np.cumsum([len(cat[k]) for k in names])
    n_last, total = len(cat[names[-1]]), len(stream)
    spans = np.array([(e - len(cat[k]), len(cat[k])) for k, e in zip(names, ends)]
                     + [(total - n_last, n_last),            # ends exactly at stream_len
                        (total - n_last + 1, n_last),        # ends at stream_len + 1
                        (total, 1), (total + 1, 0),          # starts at / past the end
                        (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF), (0xFFFFFFFF, 1),
                        (5, 0), (0, 0), (total, 0)], np.uint32)
    past = np.array([0] * (len(names) + 1) + [2, 2, 2, 2, 2, 2, 0, 0, 0], np.uint8)
    streams = {0: to(stream, dev)}
    for off in (1, 15):
        alloc = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        alloc[off: off + total] = streams[0]
        streams[off] = alloc[off: off + total]
        assert (streams[off].data_ptr() - alloc.data_ptr()) == off
    for kind in KINDS:
        want_v, want_e = O.decode_values(kind, stream, spans)
        assert np.array_equal(want_e == 2, past == 2)
        assert not want_e[-3:].any() and not want_v[-3:].any()  # a nil value reads as zero, no error
        for off, s in streams.items():
            got_v, got_e = gpu_values(kind, s, spans, dev)
            assert np.array_equal(got_e, want_e), (kind, off)
            assert np.array_equal(got_v, want_v), (kind, off)
    # the last value, read where it ends at stream_len: its own value
    v, e = gpu_values(Kind.STRING, streams[15], spans, dev)
    off, ln = v[len(names)].view(np.uint32)
    assert e[len(names)] == 0 and bytes(stream[off: off + ln]) == A.scalars()["string_1"][1]


@pytest.mark.parametrize("n", [1, 255, 256, 257, "grid"])
def test_values_grid_stride(dev, n):
    """Row counts around one block, and one call of more rows than a pass of the largest grid
    (tree.hip row_grid: 16 blocks of 256 per compute unit): the grid-stride loop reads every row."""
    heap, spans = value_spans()
    if n == "grid":
        n = torch.cuda.get_device_properties(dev).multi_processor_count * 16 * 256 + 257
    tiled = np.ascontiguousarray(np.resize(spans, (n, 2)))
    want_v, want_e = O.decode_values(Kind.INT64, heap, tiled)
    got_v, got_e = gpu_values(Kind.INT64, to(heap, dev), tiled, dev)
    assert np.array_equal(got_e, want_e)
    assert np.array_equal(got_v, want_v)
    assert n < len(spans) or (want_e == 0).any() and (want_e == 1).any()


# ---- 2. any fields through the tree encoder and decoders -----------------------------------------------

# tree, the any column, the field's path of tags from the record.  In a message a field's slot runs from
# the message's first data byte to the field's end, so in pkg1, Big and wide_tree — where other fields
# are written before the any field — their bytes are junk before the value too, and a malformed tail
# can find there what its slot lacked; in any_first_tree the slot is the catalog's slot.
TREES = {"first": (any_first_tree, "any", (1,)), "pkg1": (spec_amd.pkg1_tree, "any", (80,)),
         "shapes": (shapes_tree, "big.any", (3, 1000)), "wide": (wide_tree, "any", (203,))}
SMALL = 300  # "small": slots of at most this many bytes, so that pkg1's root group stays staged in LDS


def part_placements(part):
    cat = A.catalog()
    if part == "ok":  # what an encoder is given: well-formed values filling their slots
        return [p for p in A.placements() if p.junk == 0 and cat[p.entry].cls == "ok"]
    if part == "small":
        return [p for p in A.placements() if len(p.slot) <= SMALL]
    return list(A.placements())


@functools.lru_cache(maxsize=None)
def any_batch(which, part):
    """A batch of the tree with its `any` column replaced by spans into a heap of the catalog's
    slots (and `any#type` by each slot's last byte), the oracle's encoding of it and the oracle's
    decode of that.  Row r of the any field's table holds placement place[r] (-1: no value);
    slot[r] is the field's slot in the encoded record and expect[r] = (class, value bytes) what
    OpenValue makes of it (any_values.open_value: the oracle's DecodeTypeSize, not its tree reader)."""
    make, col, path = TREES[which]
    tree, cat = make(), A.catalog()
    tc = tree.column(col)
    assert tc.kind == Kind.ANY and tree.fields[tc.field].tag == path[-1]
    pls = part_placements(part)
    n = {"ok": 321, "small": 900, "all": 900}[part] + (100 if which == "shapes" else 0)
    cols, heaps, rows = workload.tree_batch(tree, n, 40 + len(pls), count=(0, 2))
    owner = tree.fields[tree.tables[tc.table].field].path + "?" if tc.table else None
    live = np.nonzero(cols[owner].reshape(-1))[0] if owner else np.arange(n)
    assert len(live) >= len(pls) and 256 < n < 2000 and n % 64
    heap, slots = A.heap_and_spans(pls)
    place = np.full(n, -1)
    place[live] = np.arange(len(live)) % len(pls)
    sp = np.zeros((n, 2), np.uint32)
    sp[live] = slots[place[live]]
    cols[col] = sp.view(np.uint8).reshape(n, 8)
    heaps[col] = heap
    cols[col + "#type"] = np.array([pls[j].slot[-1] if j >= 0 else 0 for j in place], np.uint8).reshape(n, 1)
    stream, ends = oracle_encode(tree, cols, heaps, n)
    want_rows, want = oracle_decode(tree, stream, ends)
    slot, expect = [], []
    for r, j in enumerate(place):
        rec = bytes(stream[(int(ends[r - 1]) if r else 0): int(ends[r])])
        s = A.field_slot(rec, path)
        cls, off, size = A.open_value(s)
        slot.append(s)
        expect.append((cls, s[off: off + size]))
        if j < 0:
            assert s == b""
            continue
        p, e = pls[j], cat[pls[j].entry]
        assert s.endswith(p.slot) and (which != "first" or s == p.slot and cls == p.cls)
        if e.cls == "ok":  # a well-formed value reads nothing before its own bytes
            assert expect[r] == ("ok", e.data)
    return SimpleNamespace(tree=tree, n=n, cols=cols, heaps=heaps, rows=rows, stream=stream, ends=ends,
                           want_rows=want_rows, want=want, col=col, pls=pls, place=place, slot=slot, expect=expect)


def any_field_bit(tree, tc):
    """(ERRMASK column, word, bit) of the any field among its table's direct fields."""
    owner = tree.tables[tc.table].field
    direct = [i for i, f in enumerate(tree.fields) if f.parent == owner]
    k = direct.index(tc.field)
    em = next(c for c in tree.columns if c.table == tc.table and c.role == ROLE_ERRMASK)
    return em, k >> 6, k & 63


def check_any_columns(b, got, buf):
    """The decoded any field of batch b against b.expect, apart from the oracle's tree reader: a
    value's span holds exactly its bytes (whatever precedes it in the slot excluded) and TYPE its
    last byte; err, nil and panic rows have span (0, 0) and TYPE 0; the field's ERRMASK bit is set
    exactly on err rows; the table's STATUS is ST_PANIC exactly on panic rows.  Returns the classes
    seen."""
    tree = b.tree
    tc = tree.column(b.col)
    g = {c.name: v for c, v in zip(tree.columns, got)}
    spans = np.ascontiguousarray(g[b.col]).view(np.uint32).reshape(-1, 2)
    types = g[b.col + "#type"].reshape(-1)
    em, word, bit = any_field_bit(tree, tc)
    errbit = (np.ascontiguousarray(g[em.name]).view(np.uint64).reshape(b.n, -1)[:, word] >> np.uint64(bit)) & np.uint64(1)
    status = g[next(c.name for c in tree.columns if c.table == tc.table and c.role == ROLE_STATUS)].reshape(-1)
    seen = set()
    for r, (cls, value) in enumerate(b.expect):
        seen.add(cls if b.place[r] >= 0 else "absent")
        off, ln = (int(x) for x in spans[r])
        assert int(errbit[r]) == (cls == "err"), (r, cls)
        assert int(status[r]) == (ST_PANIC if cls == "panic" else 0), (r, cls)
        if cls != "ok":
            assert (off, ln, int(types[r])) == (0, 0, 0), (r, cls)
            continue
        assert ln == len(value) and bytes(buf[off: off + ln]) == value, (r, b.place[r])
        assert int(types[r]) == value[-1], (r, b.place[r])
    return seen


@pytest.mark.parametrize("which", list(TREES))
def test_any_ok_values_encode_decode(dev, kernel, which):
    """Every well-formed catalog value as the tree's any field: the device encoder's bytes and ends
    are the oracle's, the decode is the oracle's, TYPE is each value's last byte, the spans hold the
    values' bytes, STATUS and ERRMASK are zero."""
    b = any_batch(which, "ok")
    assert {p.entry for p in b.pls} == {i for i, e in enumerate(A.catalog()) if e.cls == "ok"}
    assert set(range(len(b.pls))) <= set(b.place.tolist())
    check_encode_decode(b, dev)
    types = b.want[b.tree.column(b.col + "#type").index].reshape(-1)
    assert set(A.SWITCH_TYPES) <= set(types.tolist())
    assert check_any_columns(b, b.want, b.stream) <= {"ok", "absent"}


@pytest.mark.parametrize("part", ["all", "small"])
@pytest.mark.parametrize("which", list(TREES))
def test_any_all_entries_decode(dev, kernel, which, part):
    """Every catalog entry in every placement, malformed included.  The encoder copies an any span
    verbatim, so the batch encodes (bytes and ends the oracle's); the decode equals the oracle's on
    every column, and the any field's span, TYPE, ERRMASK bit and STATUS are what OpenValue makes of
    each row's slot.  "all" holds every placement (pkg1: records too long on average for the root
    group's LDS slab, parsed from HBM); "small" the slots of up to 300 bytes (pkg1: staged in LDS).
    Every class occurs where the any field is written first; ok, err and panic in the other trees,
    where the struct type byte that is nil alone in its slot reads the fields before it."""
    b = any_batch(which, part)
    assert set(range(len(b.pls))) <= set(b.place.tolist())
    if part == "all":
        assert len(b.pls) == len(A.catalog()) * len(A.JUNK_LENS)
    if which in ("pkg1", "wide"):
        slab, extra = root_slab(b.tree, b.ends)
        assert (slab + extra <= WAVE_LDS_MAX) == (which == "pkg1" and part == "small")
    stream, ends = spec_amd.encode_tree(b.tree, to_dev(b.cols, dev), to_dev(b.heaps, dev), b.n, rows=b.rows)
    torch.cuda.synchronize()
    assert np.array_equal(ends.cpu().numpy().view(np.uint64), b.ends)
    assert np.array_equal(stream.cpu().numpy(), b.stream)
    got_rows, got = decode_fresh(b.tree, b.stream, b.ends, dev)
    assert got_rows == b.want_rows == b.rows
    assert mismatches(b.tree, got, b.want) == []
    seen = check_any_columns(b, got, b.stream)
    assert ({"ok", "err", "nil", "panic"} if which == "first" else {"ok", "err", "panic"}) <= seen
    short = [r for r, (cls, value) in enumerate(b.expect) if cls == "ok" and len(value) < len(b.slot[r])]
    assert len(short) > 256  # values that do not fill their slot: the span starts at e - n, not at the slot


@pytest.mark.parametrize("which", list(TREES))
def test_any_all_entries_frames(dev, kernel, which):
    """The all-entries batch as mpx frames through spec_tree_decoder_run_frames: the oracle's decode
    over the frames' spans, which is the stream's decode with every span moved by its record's
    heads (4 bytes a record up to and including its own)."""
    b = any_batch(which, "all")
    tree = b.tree
    frames, fends = framed(b.stream, b.ends)
    rows, want = want_over_spans(tree, frames, fends)
    assert rows == b.want_rows
    d = TreeDecoder(tree)
    d.reserve(rows)
    out = [torch.zeros((max(tree.column_rows(c, rows), 1), c.width), dtype=torch.uint8, device=dev) for c in tree.columns]
    got_rows = d.run_frames(to(frames, dev), to(fends, dev), out).cpu().numpy()
    torch.cuda.synchronize()
    assert list(got_rows) == rows
    got = [c[: tree.column_rows(tc, rows)].cpu().numpy() for c, tc in zip(out, tree.columns)]
    assert mismatches(tree, got, want) == []
    # against the stream's decode: spans by their bytes, every other column equal
    spanned = {c.index for c in tree.span_columns()}
    for c, g, w in zip(tree.columns, got, b.want):
        if c.index in spanned:
            assert span_bytes(g, frames) == span_bytes(w, b.stream), c.name
        else:
            assert np.array_equal(g, w), c.name
    # the any column's table has a row per record: its spans moved by 4 * (record + 1) exactly
    tc = tree.column(b.col)
    gs = np.ascontiguousarray(got[tc.index]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    ws = np.ascontiguousarray(b.want[tc.index]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    has = ws[:, 1] > 0
    assert has.sum() > 256 and np.array_equal(gs[:, 1], ws[:, 1])
    assert np.array_equal(gs[has, 0], ws[has, 0] + 4 * (np.nonzero(has)[0] + 1)) and not gs[~has].any()
    assert {"ok", "err", "panic"} <= check_any_columns(b, got, frames)


# ---- 3. index_spans: Value.Message() ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def message_spans():
    """A stream of values and a pool of spans over it: messages written under the reader's own
    schema, the catalog's messages, values that are no messages, malformed values, empty spans; the
    stream's last value is a message, so its span ends exactly at stream_len."""
    sub = message1_tree()
    scols, sheaps, _ = workload.tree_batch(sub, 12, 31, count=(0, 3))
    s, e = oracle_encode(sub, scols, sheaps, 12)
    own = [bytes(s[(int(e[i - 1]) if i else 0): int(e[i])]) for i in range(12)]
    cat = {x.name: x for x in A.catalog()}
    messages = ["message_small", "message_big_tag", "message_list_message", "message_empty"]
    others = ["int64_m1", "string_127", "list_three_scalars", "list_300_elements", "struct_127", "bytes_0"]
    bad = ["bad_type_99", "bad_message_table_over_slot", "bad_list_data_size_varint", "bad_struct_past_slot",
           "panic_struct_size_varint", "bad_int64_eleven_byte_varint"]
    assert all(cat[k].cls == "ok" for k in messages + others) and all(cat[k].cls != "ok" for k in bad)
    items = own + [cat[k].data for k in messages + others + bad] + [own[0]]
    stream = np.frombuffer(b"".join(items), np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum([len(x) for x in items])[:-1]])
    pool = [(int(o), len(x)) for o, x in zip(offs, items)] + [(0, 0), (7, 0), (len(stream), 0)]
    assert pool[len(items) - 1][0] + pool[len(items) - 1][1] == len(stream)
    first_other = len(own) + len(messages)
    return sub, stream, np.array(pool, np.uint32), len(items) - 1, range(first_other, first_other + len(others))


@functools.lru_cache(maxsize=None)
def message_batch(n):
    sub, stream, pool, last, others = message_spans()
    pick = np.random.default_rng(n).permutation(np.resize(np.arange(len(pool)), n))
    pick[0] = last  # (n = 1: the span that ends exactly at stream_len)
    spans = pool[pick].copy()
    spans[96::97] = (len(stream) - 3, 9)  # past the stream: Go panics slicing it
    want_rows, want = O.decode_tree_spans(oracle_fields(sub), stream, spans)
    return sub, stream, spans, pick, want_rows, want


@pytest.mark.parametrize("n", [1, 65, 257, 1000])
def test_index_spans_over_values(dev, kernel, n):
    """m.Field(tag).Message() + the generated getters over spans of every sort: rows and every
    column are the oracle's.  ST_PANIC rows (a span past the stream), rows with an error status
    from a value that is no message, and clean rows all occur."""
    sub, stream, spans, pick, want_rows, want = message_batch(n)
    d = TreeDecoder(sub)
    got_rows = d.index_spans(to(stream, dev), to(spans, dev))
    got = [c.cpu().numpy() for c in d.decode().cols]
    torch.cuda.synchronize()
    assert got_rows == want_rows
    assert mismatches(sub, got, want) == []
    status = got[sub.column("#status").index].reshape(-1)
    _, _, _, last, others = message_spans()
    assert int(spans[0, 0]) + int(spans[0, 1]) == len(stream) and status[0] == 0
    if n >= 257:
        past = np.zeros(n, bool)
        past[96::97] = True
        assert np.array_equal(status == ST_PANIC, past) and past.any()
        no_message = np.isin(pick, list(others)) & ~past
        assert no_message.any() and (status[no_message] != 0).all() and (status[no_message] != ST_PANIC).all()
        assert (status == 0).sum() > n // 4
        assert want_rows[1] > 0  # list rows under the clean messages

"""GPU parity of spec_decode_flat_present / spec_decode_frames_present: per record the HasField
mask of the oracle Message (m.HasField(tag), internal/types/msg.go:106-111) beside the columns,
status and *Err bits of the oracle's flat decode — on the oracle Writer's sparse records (a
Write() that skips setters) in every mask pattern, hand-built tables, every trailer error class,
mutated records, two mask words, a repeated tag, a group parsed from HBM and mpx frames in place.
Outputs are prefilled with 0xA5 and the masks sit between canary rows.  The four schemas with
schema-specialised (hiprtc) kernels run under both kernels, everything else under the generic one."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, NESTED, Kind, Schema, workload
from tests.gpu_helpers import concat_records, require_specialised, to_dev
from tests.present_helpers import (PATTERNS, check_present, decode_present_abi, oracle_present, pack_mask, patterns,
                                   random_columns, write_sparse)
from tests.test_gpu_flat import write_record

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 130, 300]
COMPACT = NESTED.item  # {1 int32, 2 float64, 3 string}: trailer and table in one 16-byte window
WIDE40, BIG16 = (workload.bench_wide_schemas()[k] for k in ("wide40", "big16"))
JIT_SCHEMAS = {"flat16": FLAT16, "compact": COMPACT, "wide40": WIDE40, "big16": BIG16}


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    """Run a test with the schema-specialised kernels (hiprtc) and with the generic kernel."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


@pytest.fixture
def generic():
    spec_amd.set_jit(False)
    yield
    spec_amd.set_jit(True)


def sparse(schema, n, pattern, seed=1):
    cols, heaps = random_columns(schema, n, seed)
    bits = patterns(len(schema), n)[pattern]
    return write_sparse(schema, cols, heaps, bits, n), bits


# ---- 1. the mask patterns ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["flat16", "compact"])
def test_patterns(dev, kernel, name, n):
    schema = JIT_SCHEMAS[name]
    for p in PATTERNS:
        recs, bits = sparse(schema, n, p, seed=n)
        if kernel == "jit":
            require_specialised(schema, name, decode=(sum(len(r) for r in recs), n))
        want = check_present(dev, schema, recs, f"{name} {p} n={n} {kernel}", errors=p.startswith("half"))
        # a Writer's record has exactly the fields it wrote
        assert np.array_equal(want, pack_mask(bits))
        if p == "none":
            assert all(r == bytes([0, 0, 80]) for r in recs)
        if p == "all":  # the dense batch: all ones below nfields, the columns of spec_decode_flat
            assert (want[0] == (1 << len(schema)) - 1).all()
            stream, ends = concat_records(recs)
            dense = spec_amd.decode_flat(schema, to_dev(stream, dev), to_dev(ends.view(np.int64), dev))
            cols, _, _, _ = decode_present_abi(dev, schema, stream, ends)
            for f in range(len(schema)):
                assert np.array_equal(dense.cols[f].cpu().numpy(), cols[f]), f


@pytest.mark.parametrize("n", [65, 300])
@pytest.mark.parametrize("name", ["wide40", "big16"])
def test_patterns_wide_and_big_tables(dev, kernel, name, n):
    """The schemas on the batched fast path (40 fields; a tag > 255, every table big): full tables on
    the fast path, subset tables through the generic one — the same masks either way."""
    schema = JIT_SCHEMAS[name]
    for p in ("all", "none", "half0", "one_field", "alternating"):
        recs, _ = sparse(schema, n, p, seed=n + 3)
        check_present(dev, schema, recs, f"{name} {p} n={n} {kernel}", errors=True)


def test_wrapper_shapes(dev, kernel):
    n = 130
    recs, _ = sparse(FLAT16, n, "half1")
    stream, ends = concat_records(recs)
    got, pm, em = spec_amd.decode_flat_present(FLAT16, to_dev(stream, dev), to_dev(ends.view(np.int64), dev),
                                               errors=True)
    torch.cuda.synchronize()
    assert pm.dtype == torch.int64 and pm.shape == (n,) and em.shape == (n,)
    assert np.array_equal(pm.cpu().numpy().view(np.uint64), oracle_present(FLAT16, recs)[0])
    assert not em.cpu().numpy().any()
    assert len(spec_amd.decode_flat_present(FLAT16, to_dev(stream, dev), to_dev(ends.view(np.int64), dev))) == 2


# ---- 2. hand-built tables and broken records among Writer records -------------------------------------

def _table_record(vals, fields, data_size=None):
    data = b"".join(vals)
    trailer, _, err = O.encode_message_table(len(data) if data_size is None else data_size, fields)
    assert err is None, err
    return data + trailer


def edge_records(big_tag=300):
    """Records no Writer emits, or that leave the fast path, over Flat16's tags."""
    i32, i64, u16 = O.encode("int32", -77)[0], O.encode("int64", 1 << 40)[0], O.encode("uint16", 300)[0]
    e1, e2, e3 = len(i32), len(i32) + len(i64), len(i32) + len(i64) + len(u16)
    vals = [i32, i64, u16]
    recs = {
        "end0_only": O.encode_message_table(0, [(3, 0)])[0],                    # present, value zero
        "end0_first": _table_record(vals, [(3, 0), (4, e1), (5, e2), (6, e3)]),   # end 0 before real fields
        "end_past_data": _table_record(vals, [(4, e1), (5, e2 + 1000), (6, e3)]),  # absent
        "end_eq_data": _table_record(vals, [(4, e1), (5, e2), (6, e3)]),
        "foreign_after": _table_record(vals, [(4, e1), (5, e2), (200, e3)]),
        "foreign_zero": _table_record(vals, [(0, e1), (5, e2), (6, e3)]),
        "foreign_between": _table_record(vals, [(4, e1), (big_tag - 1, e2), (big_tag, e3)]),
        "unsorted": _table_record(vals, [(6, e3), (4, e1), (5, e2)]),
        "duplicate": _table_record(vals, [(4, e1), (4, e2), (6, e3)]),
        "duplicate_all": _table_record(vals, [(5, e1), (5, e2), (5, e3)]),
        "big_table_small_tags": _table_record(vals, [(4, e1), (5, e2), (big_tag, e3)]),
        "cross_kind": write_record([(3, Kind.INT16, 5), (5, Kind.INT32, 7), (10, Kind.FLOAT32, 1.5)]),
        "too_many_entries": _table_record(vals * 6, [(t + 1, e1) for t in range(17)] + [(40, e2)]),
        # every trailer error class (internal/decode/msg_test.go) and a zero-length record
        "invalid_table_size": bytes([0xFF, 80]),
        "invalid_data_size": bytes([0xFF]) + O.put_reverse_uint32(1000) + bytes([80]),
        "invalid_table": bytes([0, 0, 80, 0]) + O.put_reverse_uint32(1000) + bytes([80]),
        "invalid_data": bytes([0, 0, 80]) + O.put_reverse_uint32(1000) + bytes([0, 80]),
        "invalid_type": b"".join(vals) + bytes([70]),
        "table_size_mod3": bytes([3, 0, 80]),
        "empty": b"",
    }
    return recs


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("name", ["flat16", "big16"])
def test_edges_among_writer_records(dev, kernel, name, lane):
    """Each edge record at lane `lane` of a group (groups 0..3, so also beyond the first group) of a
    batch of sparse Writer records."""
    schema = JIT_SCHEMAS[name]
    edges = edge_records(big_tag=256 + 37 if name == "big16" else 300)
    if name == "big16":  # the same tables over this schema's tags: a subset table in a big-table schema
        t = schema.tags
        i64 = O.encode("int64", -9)[0]
        edges["subset_big"] = _table_record([i64], [(t[4], len(i64))])
        edges["subset_big_end0"] = _table_record([i64], [(t[0], 0), (t[4], len(i64))])
    names = sorted(edges)
    n = 300
    base, _ = sparse(schema, n, "half2", seed=lane)
    for b0 in range(0, len(names), 4):
        recs = list(base)
        for g, e in enumerate(names[b0:b0 + 4]):
            recs[64 * g + lane] = edges[e]
        want = check_present(dev, schema, recs, f"{name} edges {names[b0:b0 + 4]} lane {lane} {kernel}", errors=True)
        if name == "flat16":
            for g, e in enumerate(names[b0:b0 + 4]):
                m = int(want[0, 64 * g + lane])
                if e == "end0_only":
                    assert m == 1 << 2
                if e == "end0_first":
                    assert m == 0b111100
                if e == "end_past_data":
                    assert m == 0b101000
                if e.startswith("invalid") or e in ("empty", "table_size_mod3"):
                    assert m == 0


def test_record_made_big_by_a_long_field(dev, kernel):
    """A small-tag record with a 70,000-byte bytes field: IsBigMessage, a six-byte table."""
    n = 65
    cols, heaps = random_columns(FLAT16, n, 5)
    bits = patterns(16, n)["half0"]
    recs = write_sparse(FLAT16, cols, heaps, bits, n)
    blob = bytes(np.random.default_rng(1).integers(0, 256, 70000, dtype=np.uint8))
    for i in (0, 63, 64):
        recs[i] = write_record([(4, Kind.INT32, i), (15, Kind.BYTES, blob), (16, Kind.INT64, -i)])
        assert recs[i][-1] == 81  # TypeBigMessage
    want = check_present(dev, FLAT16, recs, f"big by size {kernel}")
    assert int(want[0, 63]) == (1 << 3) | (1 << 14) | (1 << 15)


@pytest.mark.parametrize("seed", range(2))
def test_fuzz_mutated_sparse_records(dev, kernel, seed):
    """Sparse Flat16 records with random byte mutations, truncations and garbage records (the
    recipe of tests/test_gpu_flat.py test_fuzz_mutated_records)."""
    rng = np.random.default_rng(2000 + seed)
    n = 300
    recs, _ = sparse(FLAT16, n, f"half{seed}", seed=seed)
    out = []
    for r in recs:
        x = rng.integers(0, 6)
        b = bytearray(r)
        if x == 0 and len(b):
            for _ in range(rng.integers(1, 4)):
                b[rng.integers(0, len(b))] = rng.integers(0, 256)
        elif x == 1 and len(b):  # mutate the trailer / table region
            for _ in range(rng.integers(1, 3)):
                b[len(b) - 1 - rng.integers(0, min(len(b), 60))] = rng.integers(0, 256)
        elif x == 2:
            b = b[rng.integers(0, len(b)):]
        elif x == 3:
            b = b[:rng.integers(0, len(b))]
        elif x == 4:
            b = bytearray(rng.integers(0, 256, rng.integers(0, 300), dtype=np.uint8).tobytes())
            if len(b) and rng.integers(0, 2):
                b[-1] = 80
        out.append(bytes(b))
    check_present(dev, FLAT16, out, f"fuzz {seed} {kernel}", errors=True)


def test_fuzz_compact_tables(dev, kernel):
    """The compact schema with its tail window mutated: subset tables, wrong sizes, foreign tags."""
    rng = np.random.default_rng(31)
    n = 300
    recs, _ = sparse(COMPACT, n, "half0", seed=9)
    out = []
    for r in recs:
        b = bytearray(r)
        if rng.integers(0, 3) == 0:
            b[len(b) - 1 - rng.integers(0, min(len(b), 16))] = rng.integers(0, 256)
        out.append(bytes(b))
    check_present(dev, COMPACT, out, f"compact fuzz {kernel}", errors=True)


# ---- 3. run-time schemas only: two mask words, a repeated tag, a foreign tag between schema tags ----------

@pytest.mark.parametrize("n", [1, 65, 300])
def test_two_mask_words(dev, generic, n):
    """100 fields: two words per record, word-major; bits at or above nfields are zero."""
    kinds = [Kind.INT32, Kind.BOOL, Kind.UINT64, Kind.STRING, Kind.FLOAT32]
    schema = Schema([(t + 1, kinds[t % 5]) for t in range(100)])
    for p in ("all", "half0", "one_field"):
        recs, _ = sparse(schema, n, p, seed=n)
        want = check_present(dev, schema, recs, f"100 fields {p} n={n}", errors=True)
        assert want.shape == (2, n) and not (want[1] >> np.uint64(36)).any()
        if p == "all":
            assert (want[0] == np.uint64(2**64 - 1)).all() and (want[1] == np.uint64(2**36 - 1)).all()


def test_repeated_tag(dev, generic):
    """Schema tags [5, 5, 7]: both fields of tag 5 look up the same entry; the oracle's bits."""
    schema = Schema([(5, Kind.INT32), (5, Kind.INT64), (7, Kind.BOOL)])
    recs = [write_record([(5, Kind.INT32, 3), (7, Kind.BOOL, True)]), write_record([(7, Kind.BOOL, False)]),
            write_record([(5, Kind.INT32, 1), (5, Kind.INT64, 2)]), write_record([])] * 40
    want = check_present(dev, schema, recs, "repeated tag", errors=True)
    assert [int(x) for x in want[0, :4]] == [0b111, 0b100, 0b011, 0]


def test_foreign_tag_between_schema_tags(dev, generic):
    schema = Schema([(2, Kind.INT32), (6, Kind.INT64), (10, Kind.UINT16)])
    i32, i64 = O.encode("int32", 5)[0], O.encode("int64", -5)[0]
    rec = _table_record([i32, i64], [(2, len(i32)), (4, len(i32)), (6, len(i32) + len(i64))])
    want = check_present(dev, schema, [rec] * 70, "foreign between")
    assert (want[0] == 0b011).all()


# ---- 4. a group parsed from HBM ------------------------------------------------------------------------

def test_group_over_its_slab(dev, kernel):
    """Group 1 of a 300-record batch holds 1,500-byte strings: its span exceeds the slab sized from
    the batch's mean record, so it is parsed from HBM; the other groups from LDS."""
    n = 300
    cols, heaps = random_columns(FLAT16, n, 12)
    bits = patterns(16, n)["half1"]
    recs = write_sparse(FLAT16, cols, heaps, bits, n)
    for i in range(64, 128):
        fields = [(14, Kind.STRING, "s" * 1500), (16, Kind.INT64, i)]
        recs[i] = write_record(fields if i % 2 else fields[:1])
    stream, _ = concat_records(recs)
    assert 64 * 1500 > 1.04 * 64 * stream.size / n + 2048  # the group cannot fit the slab
    want = check_present(dev, FLAT16, recs, f"over slab {kernel}", errors=True)
    assert int(want[0, 65]) == (1 << 13) | (1 << 15) and int(want[0, 64]) == 1 << 13


# ---- 5. mpx frames in place ------------------------------------------------------------------------------

def check_frames(dev, recs):
    """recs as mpx frames through spec_decode_frames_present, ranges [0, n), [1, n - 1) and [64, 65)
    (those that are ranges of the batch): masks, status and columns of the unframed decode, spans
    4(k + 1) further on, records outside the range untouched."""
    n = len(recs)
    stream, ends = concat_records(recs)
    want_cols, want_status = O.decode_flat_batch(FLAT16.tags, FLAT16.kinds, stream, ends, FLAT16.widths)
    want_pm = oracle_present(FLAT16, recs)
    want_em = O.decode_flat_errors(FLAT16.tags, FLAT16.kinds, stream, ends)
    fr = spec_amd.make_frames(stream, ends)
    fends = ends + 4 * (np.arange(n, dtype=np.uint64) + 1)
    shift = 4 * (np.arange(n, dtype=np.uint32) + 1)
    for r0, r1 in ((0, n), (1, n - 1), (64, 65)):
        if not (r0 < r1 <= n):
            continue
        cols, status, pm, em = decode_present_abi(dev, FLAT16, fr, fends, errors=True, frames=(r0, r1))
        inside = np.zeros(n, bool)
        inside[r0:r1] = True
        assert np.array_equal(status[inside], want_status[inside]) and (status[~inside] == 0xA5).all()
        assert np.array_equal(pm[0, r0:r1], want_pm[0, r0:r1]) and (pm[0, :r0] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
        assert np.array_equal(em[0, r0:r1], want_em[r0:r1])
        for f, fld in enumerate(FLAT16.fields):
            w = want_cols[f].copy()
            if fld.kind in (Kind.STRING, Kind.BYTES):
                wv = w.view(np.uint32)
                wv[:, 0] = np.where(wv[:, 1] > 0, wv[:, 0] + shift, 0)
            assert np.array_equal(cols[f][inside], w[inside]), (fld, r0, r1)
            assert (cols[f][~inside] == 0xA5).all()
    return want_status


@pytest.mark.parametrize("n", NS)
def test_frames_in_place(dev, kernel, n):
    recs, _ = sparse(FLAT16, n, "half0", seed=n)
    check_frames(dev, recs)


@pytest.mark.parametrize("cut", [1, 2, 3, 4])
def test_frames_cut_records(dev, kernel, cut):
    """Records 1, 64 and 129 of 130 lose their first `cut` bytes: their tables claim more data than
    the record holds.  A decoder that let a record start at its frame head would open them."""
    n = 130
    cols, heaps = random_columns(FLAT16, n, cut)
    bits = patterns(16, n)["half0"]
    bits[[1, 64, 129]] = True
    recs = write_sparse(FLAT16, cols, heaps, bits, n)
    for i in (1, 64, 129):
        recs[i] = recs[i][cut:]
    st = check_frames(dev, recs)
    assert all(st[i] != 0 for i in (1, 64, 129)) and not st[[0, 2, 63, 65, 128]].any()


def test_frames_wrapper_and_two_words(dev, generic):
    kinds = [Kind.INT32, Kind.BOOL, Kind.UINT64]
    schema = Schema([(t + 1, kinds[t % 3]) for t in range(100)])
    n = 130
    recs, _ = sparse(schema, n, "half1", seed=4)
    stream, ends = concat_records(recs)
    fr = spec_amd.make_frames(stream, ends)
    fends = (ends + 4 * (np.arange(n, dtype=np.uint64) + 1)).view(np.int64)
    want = oracle_present(schema, recs)
    got, pm = spec_amd.decode_frames_present(schema, to_dev(fr, dev), to_dev(fends, dev), 1, n - 1)
    torch.cuda.synchronize()
    g = pm.cpu().numpy().view(np.uint64)
    assert g.shape == (2, n - 1)  # word c of record r at present[c * r1 + r]
    assert np.array_equal(g[:, 1:], want[:, 1:n - 1]) and not g[:, 0].any()

"""GPU parity at the edges of the LDS staging every decode kernel shares (decode_core.hpp
stage_span) and of the column stores: record counts around a group, group spans of k KiB - 1 /
k KiB / k KiB + 1 bytes, the stream's last partial 16-byte granule, a group over the slab between
groups that fit, empty records at a group's first and last lane, streams that are views at odd
byte offsets of an aligned allocation, the frames path (head = 4), and columns allocated between
canary rows (also with the bin128 / bin256 columns as views at +8 bytes: the ABI promises no more
than a uint64 array's alignment).  Specialised, generic and *Err kernels, against the oracle; one
small nested and one small tree batch go through the same primitive."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, Kind, _lib, batch, workload
from tests.gpu_helpers import concat_records, oracle_encode

pytestmark = pytest.mark.gpu

SCHEMAS = {"flat16": FLAT16, "wide40": workload.bench_wide_schemas()["wide40"]}
PAD = 16       # canary rows before and after every column (16 rows keep a column's alignment)
CANARY = 0xA5
WIDE_BINS = (Kind.BIN128, Kind.BIN256)


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


# ---- batches (built once, with their oracle decode) ---------------------------------------------

def _freeze(stream, ends):
    stream.setflags(write=False)
    ends.setflags(write=False)
    return stream, ends


@functools.lru_cache(maxsize=None)
def counted(name, n):
    sc = SCHEMAS[name]
    cols, heaps = workload.gen_columns(sc, n, seed=1000 + n, str_len=(30, 62) if name == "flat16" else (0, 24))
    return _freeze(*oracle_encode(sc, cols, heaps, n))


def _string_lens(schema, cols):
    f = next(i for i, fld in enumerate(schema.fields) if fld.kind == Kind.STRING)
    return cols[f].view(np.uint32)[:, 1]


def _shrink(lens, rows, d):
    """Take d bytes off the strings of `rows` (each keeps at least one byte, so a record shrinks
    by exactly what its string does)."""
    for r in rows:
        take = min(d, int(lens[r]) - 1)
        lens[r] -= take
        d -= take
    assert d == 0


@functools.lru_cache(maxsize=None)
def shaped(tail):
    """Five Flat16 groups: the spans of groups 1, 2, 3 are k KiB - 1, k KiB, k KiB + 1 bytes and
    stream_len % 16 == tail (the last group holds the stream's last granule)."""
    n = 5 * 64
    cols, heaps = workload.gen_columns(FLAT16, n, seed=77)
    cols = [c.copy() for c in cols]
    lens = _string_lens(FLAT16, cols)
    _, ends = oracle_encode(FLAT16, cols, heaps, n)
    sizes = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
    for g, delta in ((1, -1), (2, 0), (3, 1)):
        rows = range(64 * g, 64 * g + 64)
        s = int(sizes[rows.start:rows.stop].sum())
        _shrink(lens, rows, s - (((s - 2) // 1024) * 1024 + delta))
    _, ends = oracle_encode(FLAT16, cols, heaps, n)
    _shrink(lens, range(256, 320), (int(ends[-1]) - tail) % 16)  # group 4 only: moves the stream's end
    stream, ends = oracle_encode(FLAT16, cols, heaps, n)
    e = np.concatenate([[0], ends.astype(np.int64)])
    assert [int(e[64 * g + 64] - e[64 * g]) % 1024 for g in (1, 2, 3)] == [1023, 0, 1]
    assert int(ends[-1]) % 16 == tail
    return _freeze(stream, ends)


@functools.lru_cache(maxsize=None)
def over_slab():
    """Eight Flat16 groups of short records with group 3 of long ones: its span exceeds the slab
    sized from the batch's mean record (decode_slab_bytes), its neighbours fit."""
    small, heaps_s = workload.gen_columns(FLAT16, 8 * 64, seed=5, str_len=(0, 24))
    big, heaps_b = workload.gen_columns(FLAT16, 64, seed=6, str_len=(100, 120))
    s1, e1 = oracle_encode(FLAT16, small, heaps_s, 8 * 64)
    s2, e2 = oracle_encode(FLAT16, big, heaps_b, 64)
    e1, e2 = e1.astype(np.int64), e2.astype(np.int64)
    recs = [bytes(s1[(e1[i - 1] if i else 0):e1[i]]) for i in range(8 * 64)]
    recs[192:256] = [bytes(s2[(e2[i - 1] if i else 0):e2[i]]) for i in range(64)]
    stream, ends = concat_records(recs)
    e = np.concatenate([[0], ends.astype(np.int64)])
    slab = 48 + (int(int(e[-1]) / len(recs) * 64 * 1.04 / 1024) + 1) * 1024 + 32
    spans = [int(e[64 * g + 64] - e[64 * g]) for g in range(8)]
    # a span fits when its 1 KiB chunks from a 16-byte aligned origin, the guard and 16 bytes do
    assert spans[3] > slab and all(48 + ((s + 15 + 1023) & ~1023) + 16 <= slab
                                   for g, s in enumerate(spans) if g != 3), (slab, spans)
    return _freeze(stream, ends)


@functools.lru_cache(maxsize=None)
def with_empties():
    """Three Flat16 groups; records 64 and 127 (group 1's first and last lane), 0 and 191 are empty."""
    stream, ends = counted("flat16", 192)
    e = np.concatenate([[0], ends.astype(np.int64)])
    recs = [b"" if i in (0, 64, 127, 191) else bytes(stream[e[i]:e[i + 1]]) for i in range(192)]
    return _freeze(*concat_records(recs))


@functools.lru_cache(maxsize=None)
def wanted(name, key):
    """Oracle columns, status and *Err mask of a batch (key: the builder call that made it)."""
    sc = SCHEMAS[name]
    stream, ends = BATCHES[key[0]](*key[1:])
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    cols, status = O.decode_flat_batch(sc.tags, sc.kinds, stream, ends, sc.widths, nthreads=4)
    mask = O.decode_flat_errors(sc.tags, sc.kinds, stream, ends)
    return cols, status, mask


BATCHES = {"counted": counted, "shaped": lambda tail: shaped(tail), "over_slab": lambda: over_slab(),
           "with_empties": lambda: with_empties()}


# ---- one decode between canaries ---------------------------------------------------------------

def _canary_buffer(n, w, shift, dev):
    raw = torch.full(((n + 2 * PAD) * w + 16,), CANARY, dtype=torch.uint8, device=dev)
    lo = shift + PAD * w
    return raw, raw[lo:lo + n * w].view(n, w), lo


def run_case(dev, name, key, variant, offset=0, col_shift=0):
    """Decode the batch `key` with the plain, *Err or frames entry point, the stream a view
    `offset` bytes into an aligned allocation, every column and the status between canary rows
    (bin128 / bin256 columns `col_shift` bytes further), and compare with the oracle."""
    sc = SCHEMAS[name]
    stream, ends = BATCHES[key[0]](*key[1:])
    want_cols, want_status, want_mask = wanted(name, key)
    n = len(ends)
    e64 = np.ascontiguousarray(ends, dtype=np.uint64).view(np.int64)
    if variant == "frames":
        stream = spec_amd.make_frames(stream, e64)
        e64 = e64 + 4 * (np.arange(n, dtype=np.int64) + 1)
    room = torch.zeros(offset + max(stream.size, 1), dtype=torch.uint8)
    room[offset:offset + stream.size] = torch.from_numpy(np.array(stream))
    d_stream = room.to(dev)[offset:offset + stream.size]
    assert (d_stream.data_ptr() - offset) % 128 == 0
    d_ends = torch.from_numpy(e64).to(dev)
    held = [_canary_buffer(n, w, col_shift if fld.kind in WIDE_BINS else 0, dev)
            for fld, w in zip(sc.fields, sc.widths)]
    held.append(_canary_buffer(n, 1, 0, dev))
    cols = [c for _, c, _ in held[:-1]]
    status = held[-1][1].view(n)
    mask = None
    if variant == "plain":
        spec_amd.decode_flat(sc, d_stream, d_ends, cols=cols, status=status)
    elif variant == "frames":
        spec_amd.decode_frames(sc, d_stream, d_ends, cols=cols, status=status)
    else:
        held.append(_canary_buffer(n, 8, 0, dev))
        mask = held[-1][1]
        ptrs = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
        rc = _lib.lib().spec_decode_flat_errors(C.byref(sc.c), batch._ptr(d_stream), d_stream.numel(),
                                                batch._ptr(d_ends), n, ptrs, batch._ptr(status), batch._ptr(mask),
                                                batch._stream_handle())
        _lib.check(rc, "spec_decode_flat_errors")
    torch.cuda.synchronize()
    label = f"{name} {key} {variant} +{offset} cols+{col_shift}"
    assert np.array_equal(status.cpu().numpy(), want_status), label + ": status"
    shift = 4 * (np.arange(n, dtype=np.uint32) + 1)
    for f, fld in enumerate(sc.fields):
        w = want_cols[f]
        if variant == "frames" and fld.kind in (Kind.STRING, Kind.BYTES):  # spans point into the framed buffer
            w = w.copy()
            wv = w.view(np.uint32)
            wv[:, 0] = np.where(wv[:, 1] > 0, wv[:, 0] + shift, 0)
        g = cols[f].cpu().numpy()
        if not np.array_equal(g, w):
            i = int(np.nonzero((g != w).any(axis=1))[0][0])
            raise AssertionError(f"{label}: field {f} ({fld.kind.name}) record {i}: gpu={g[i].tobytes().hex()} "
                                 f"oracle={w[i].tobytes().hex()}")
    if mask is not None:
        assert np.array_equal(mask.cpu().numpy().view(np.uint64).ravel(), want_mask.ravel()), label + ": errmask"
    for (raw, col, lo), what in zip(held, [f"field {f}" for f in range(len(sc))] + ["status", "errmask"]):
        r = raw.cpu().numpy()
        hi = lo + col.numel()
        assert (r[:lo] == CANARY).all() and (r[hi:] == CANARY).all(), f"{label}: {what} written outside its rows"


# ---- the cases ----------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "err"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129, 513])
@pytest.mark.parametrize("name", ["flat16", "wide40"])
def test_record_counts(dev, kernel, name, n, variant):
    run_case(dev, name, ("counted", name, n), variant)


@pytest.mark.parametrize("variant", ["plain", "err", "frames"])
@pytest.mark.parametrize("tail", [0, 1, 15])
def test_group_spans_and_stream_tail(dev, kernel, tail, variant):
    run_case(dev, "flat16", ("shaped", tail), variant)


@pytest.mark.parametrize("variant", ["plain", "err", "frames"])
def test_group_over_slab_between_groups_that_fit(dev, kernel, variant):
    run_case(dev, "flat16", ("over_slab",), variant)


@pytest.mark.parametrize("variant", ["plain", "err", "frames"])
def test_empty_records_at_group_edges(dev, kernel, variant):
    run_case(dev, "flat16", ("with_empties",), variant)


@pytest.mark.parametrize("variant", ["plain", "err", "frames"])
@pytest.mark.parametrize("offset", [0, 1, 15, 16, 112, 127])
def test_stream_views(dev, kernel, offset, variant):
    """spec_decode_flat takes a stream at any byte address (it checks no alignment): every offset
    into a 128-byte aligned allocation decodes the same."""
    run_case(dev, "flat16", ("shaped", 1), variant, offset=offset)
    run_case(dev, "wide40", ("counted", "wide40", 129), variant, offset=offset)


@pytest.mark.parametrize("variant", ["plain", "err"])
@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("name", ["flat16", "wide40"])
def test_wide_bin_columns_at_plus_8(dev, kernel, name, n, variant):
    """bin128 / bin256 columns only 8-byte aligned (what the ABI promises)."""
    run_case(dev, name, ("counted", name, n), variant, col_shift=8)


@pytest.mark.parametrize("offset", [0, 112])
def test_nested_small(dev, kernel, offset):
    from tests.test_gpu_nested import _check_nested_mode

    n = 193
    stream, ends = O.encode_nested_batch(workload.nested(n, seed=3))
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    want = O.decode_nested_batch(stream, ends)
    room = torch.zeros(offset + stream.size, dtype=torch.uint8)
    room[offset:] = torch.from_numpy(np.array(stream))
    d_stream = room.to(dev)[offset:]
    d_ends = torch.from_numpy(ends.view(np.int64)).to(dev)
    for onepass in (False, True):
        _check_nested_mode(dev, d_stream, d_ends, want, n, f"nested +{offset} onepass={onepass}", onepass, None)


@pytest.mark.parametrize("offset", [0, 112])
def test_tree_small(dev, offset):
    from tests.tree_helpers import mismatches, oracle_decode
    from tests.tree_helpers import oracle_encode as tree_encode

    n = 129
    tree = spec_amd.pkg1_tree()
    cols, heaps, _ = workload.tree_batch(tree, n, 900)
    stream, ends = tree_encode(tree, cols, heaps, n)
    want_rows, want = oracle_decode(tree, stream, ends)
    room = torch.zeros(offset + stream.size, dtype=torch.uint8)
    room[offset:] = torch.from_numpy(np.array(stream))
    out = spec_amd.decode_tree(tree, room.to(dev)[offset:],
                               torch.from_numpy(np.ascontiguousarray(ends).view(np.int64)).to(dev))
    torch.cuda.synchronize()
    assert out.rows == want_rows
    assert mismatches(tree, [c.cpu().numpy() for c in out.cols], want) == []

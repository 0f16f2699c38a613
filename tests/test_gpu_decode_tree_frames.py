"""GPU parity of the schema-tree decoder over mpx frames (spec_tree_decoder_index_frames,
spec_tree_decoder_run_frames): the frames of a batch decode, in place, to what the oracle's generated
readers give over the spans (ends[k-1] + 4, size_k) of the same buffer — every column equal, span
offsets included — and to what index_spans + decode give on the device; under the generated
(hiprtc) and the run-time kernels; run_frames without a host synchronisation and clamped by its
columns; the root wave pair over its slab and at the buffer's end; `head` per call, not per decoder;
records cut short (the head is not record data) and frame ends that are garbage."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import workload
from spec_amd.tree import REL_ONE, TreeDecoder
from tests.gpu_helpers import concat_records
from tests.test_gpu_tree import _spec_tree
from tests.tree_helpers import mismatches, oracle_decode, oracle_encode, oracle_fields

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 4096


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
        pytest.exit(f"GPU error after a framed tree decode test: {e}", returncode=3)


def to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def spans_of(fends):
    """The message of every frame as a span of the framed buffer: (ends[k-1] + 4, size_k); a frame
    whose ends are not 4 apart is a nil span (an empty message)."""
    fends = np.asarray(fends, np.int64)
    off = np.concatenate([[0], fends[:-1]]) + 4
    ln = np.maximum(fends - off, 0)
    return np.stack([np.where(ln > 0, off, 0), ln], 1).astype(np.uint32)


def framed(stream, ends):
    """(frames, frame ends int64, the oracle's rows and columns over the frames' spans)."""
    ends = np.ascontiguousarray(ends, dtype=np.uint64).view(np.int64)
    frames = spec_amd.make_frames(np.ascontiguousarray(stream, dtype=np.uint8), ends)
    fends = ends + 4 * (np.arange(len(ends), dtype=np.int64) + 1)
    return frames, fends


def want_over_spans(tree, frames, fends):
    return O.decode_tree_spans(oracle_fields(tree), frames, spans_of(fends))


@functools.lru_cache(maxsize=None)
def batch(name, n, seed):
    tree = spec_amd.pkg1_tree() if name == "pkg1" else _spec_tree(name)
    cols, heaps, _ = workload.tree_batch(tree, n, seed, count=(0, 3))
    stream, ends = oracle_encode(tree, cols, heaps, n)
    frames, fends = framed(stream, ends)
    rows, want = want_over_spans(tree, frames, fends)
    return tree, stream, ends, frames, fends, rows, want


def decode_frames(tree, frames, fends, dev, d=None):
    d = d or TreeDecoder(tree)
    rows = d.index_frames(to(frames, dev), to(fends, dev))
    got = [c.cpu().numpy() for c in d.decode().cols]
    torch.cuda.synchronize()
    return rows, got


def check(tree, frames, fends, dev, label, want=None):
    rows, cols = want or want_over_spans(tree, frames, fends)
    got_rows, got = decode_frames(tree, frames, fends, dev)
    assert got_rows == rows, label
    assert mismatches(tree, got, cols) == [], label
    return got_rows, got


# ---- 1. parity ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("pkg1", 1), ("pkg1", 65), ("pkg1", 300), ("pmpx.Message", 65),
                                    ("prpc.Message", 65)])
def test_tree_frames_parity(dev, kernel, name, n):
    tree, stream, ends, frames, fends, rows, want = batch(name, n, 200 + n)
    got_rows, got = check(tree, frames, fends, dev, f"{name} {kernel} n={n}", (rows, want))
    # the rows are the unframed decode's; and index_spans + decode over the same buffer agree
    assert got_rows == oracle_decode(tree, stream, ends)[0]
    d = TreeDecoder(tree)
    assert d.index_spans(to(frames, dev), to(spans_of(fends), dev)) == rows
    via_spans = [c.cpu().numpy() for c in d.decode().cols]
    torch.cuda.synchronize()
    assert mismatches(tree, got, via_spans) == []


# ---- 2. run_frames ------------------------------------------------------------------------------------

def guarded_columns(tree, rows, dev):
    bufs, out = [], []
    for c in tree.columns:
        nbytes = max(tree.column_rows(c, rows), 1) * c.width
        b = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
        bufs.append((b, nbytes))
        out.append(b[GUARD: GUARD + nbytes].view(-1, c.width))
    return bufs, out


def assert_guards(tree, bufs):
    for (b, nbytes), c in zip(bufs, tree.columns):
        h = b.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + nbytes:] == CANARY).all(), c.name


def test_tree_run_frames(dev, kernel):
    """run_frames: one asynchronous pass; rows_out as run's on the unframed batch; a list table
    clamped by its columns reports ~0 (and every table below it), nothing written past a column."""
    tree = spec_amd.pkg1_tree()
    ca, ha, _ = workload.tree_batch(tree, 400, 81, count=(3, 4))
    s1, e1 = oracle_encode(tree, ca, ha, 400)
    cb, hb, _ = workload.tree_batch(tree, 400, 82, count=(4, 4))
    s2, e2 = oracle_encode(tree, cb, hb, 400)
    f1, fe1 = framed(s1, e1)
    f2, fe2 = framed(s2, e2)
    want_rows, want = want_over_spans(tree, f2, fe2)
    d = TreeDecoder(tree)
    rows_a = d.index_frames(to(f1, dev), to(fe1, dev))
    lists = [t.index for t in tree.tables if t.rel == 2]
    over = {t for t in lists if want_rows[t] > rows_a[t]}
    assert over

    def under(t):  # t is, or hangs under, a list that did not fit
        while t > 0:
            if t in over:
                return True
            t = tree.tables[t].parent
        return False

    bufs, out = guarded_columns(tree, rows_a, dev)
    got_rows = d.run_frames(to(f2, dev), to(fe2, dev), out)  # (no synchronisation up to here)
    got_rows = got_rows.cpu().numpy()
    assert_guards(tree, bufs)
    for t in range(len(tree.tables)):
        assert got_rows[t] == (-1 if under(t) else want_rows[t]), t
    for i, c in enumerate(tree.columns):
        if not under(c.table):
            assert np.array_equal(out[i][: tree.column_rows(c, want_rows)].cpu().numpy(), want[i]), c.name
    # with room for everything: the oracle's columns, and run's row counts on the unframed batch
    d.reserve(want_rows)
    bufs, out = guarded_columns(tree, want_rows, dev)
    got_rows = d.run_frames(to(f2, dev), to(fe2, dev), out).cpu().numpy()
    assert_guards(tree, bufs)
    assert list(got_rows) == want_rows
    assert mismatches(tree, [c.cpu().numpy() for c in out], want) == []
    plain = [torch.empty_like(c) for c in out]
    assert list(d.run(to(s2, dev), to(e2.view(np.int64), dev), plain).cpu().numpy()) == want_rows


# ---- 3. the root pair over its slab and at the buffer's end ---------------------------------------------------

def _root_windows_framed(fends, extra):
    """tests/test_gpu_tree.py _root_windows for frames: the slab is sized from frames_len / n and a
    window's span starts 4 bytes after the previous frame's end."""
    n, total = len(fends), int(fends[-1])
    slab = (int(64.0 * total / n * 1.15 + 128 + 64) + 1023) & ~1023
    if slab + extra > 40960:  # WAVE_LDS_MAX
        return 0, []
    starts = np.concatenate([[0], fends[:-1]]).astype(np.int64) + 4
    out = []
    for w in range((n + 63) // 64):
        lo, hi = int(starts[w * 64]), int(fends[min(n, w * 64 + 64) - 1])
        sb, se = max(lo - 64, 0) & ~15, (hi + 31) & ~15
        fits = se - sb + 16 <= slab
        tail, chunks = total & ~15, (se - sb + 1023) >> 10
        tw = ((tail - sb) >> 10) % 2 if fits and total % 16 and sb <= tail < sb + chunks * 1024 else None
        out.append((fits, tw))
    return slab, out


@pytest.mark.parametrize("case", ["tail_wave0", "tail_wave1", "last_over_slab"])
def test_tree_frames_root_pair_over_slab_and_buffer_end(dev, case):
    """The three shapes of test_pkg1_root_pair_over_slab_and_stream_end, framed: a 64-record window
    over the slab among staged ones with the buffer's last partial 16-byte chunk refilled by wave 0 or
    by wave 1, and the last window itself over the slab."""
    tree = spec_amd.pkg1_tree()
    cols, heaps, _ = workload.tree_batch(tree, 1500, 77)
    s, e = oracle_encode(tree, cols, heaps, 1500)
    e = e.astype(np.int64)
    st = np.concatenate([[0], e[:-1]])
    sz = e - st
    big = int(np.argmax(sz))
    gn = 1 + sum(1 for t in tree.tables if t.index and t.rel == REL_ONE and tree.tables[t.parent].rel != 2)
    extra = 512 * (gn - 1) + 16
    pick = None
    for m in range(600, 1500):
        order = list(range(64)) + [big] * 64 + list(range(128, m))
        if case == "last_over_slab":
            order = list(range(m - 64)) + [big] * 64
        fe = np.cumsum(sz[order] + 4)
        slab, w = _root_windows_framed(fe, extra)
        if not slab:
            continue
        if case == "last_over_slab":
            ok = not w[-1][0] and all(f for f, _ in w[:-1]) and int(fe[-1]) % 16
        else:
            ok = not w[1][0] and all(f for f, _ in w[:1] + w[2:]) and w[-1][1] == int(case[-1])
        if ok:
            pick = order
            break
    assert pick is not None, "no record count puts the windows where the case needs them"
    stream = np.concatenate([s[st[i]: e[i]] for i in pick])
    ends = np.cumsum(sz[pick]).astype(np.uint64)
    frames, fends = framed(stream, ends)
    check(tree, frames, fends, dev, case)


# ---- 4. head is per call ------------------------------------------------------------------------------------------

def test_tree_head_is_per_call(dev, kernel):
    """One decoder: framed, unframed, framed again (index + decode, then the one-pass run): each
    result is its own oracle's — the head neither sticks nor gets lost."""
    tree, stream, ends, frames, fends, rows, want = batch("pkg1", 300, 500)
    urows, uwant = oracle_decode(tree, stream, ends)
    d = TreeDecoder(tree)
    d_s, d_e = to(stream, dev), to(np.asarray(ends).view(np.int64), dev)
    d_f, d_fe = to(frames, dev), to(fends, dev)
    for step in ("framed", "unframed", "framed"):
        if step == "framed":
            assert d.index_frames(d_f, d_fe) == rows
            assert mismatches(tree, [c.cpu().numpy() for c in d.decode().cols], want) == [], step
        else:
            assert d.index(d_s, d_e) == urows
            assert mismatches(tree, [c.cpu().numpy() for c in d.decode().cols], uwant) == [], step
    out = [torch.zeros((max(tree.column_rows(c, rows), 1), c.width), dtype=torch.uint8, device=dev)
           for c in tree.columns]
    for step in ("framed", "unframed", "framed"):
        if step == "framed":
            got_rows = d.run_frames(d_f, d_fe, out).cpu().numpy()
            w = want
        else:
            got_rows = d.run(d_s, d_e, out).cpu().numpy()
            w = uwant
        assert list(got_rows) == rows
        assert mismatches(tree, [c[: tree.column_rows(tc, rows)].cpu().numpy()
                                 for c, tc in zip(out, tree.columns)], w) == [], step


# ---- 5. cut records --------------------------------------------------------------------------------------------------

def _submessage_first_record(rng):
    """A pkg1 record written with its message1 sub-message first: the sub-message's data starts at
    the record's first byte."""
    wr = O.Writer()
    wr.message()
    wr.field_message(52)
    for tag in (1, 2, 3):
        wr.field(tag, "int32", int(rng.integers(-1000, 1000)))
    assert wr.end()[1] is None
    wr.field(1, "bool", 1)
    wr.field(11, "int32", int(rng.integers(-99, 99)))
    wr.field(50, "string", "abcdef")
    b, err = wr.end()
    assert err is None, err
    wr.close()
    return b


@pytest.mark.parametrize("what", ["root", "submessage"])
@pytest.mark.parametrize("cut", range(1, 9))
def test_tree_frames_cut_records(dev, kernel, what, cut):
    """Records 1, 64 and 129 of 130 lose their first `cut` bytes, so their message tables claim
    more data than the record holds ("submessage": records written sub-message first, whose own
    table then overruns too).  A decoder whose row bounds began at the frame head would open
    cuts 1..4."""
    tree, stream, ends, _, _, _, _ = batch("pkg1", 130, 600)
    recs = [bytes(stream[(int(ends[i - 1]) if i else 0):int(ends[i])]) for i in range(130)]
    rng = np.random.default_rng(cut)
    for i in (1, 64, 129):
        r = _submessage_first_record(rng) if what == "submessage" else recs[i]
        recs[i] = r[cut:]
    s2, e2 = concat_records(recs)
    frames, fends = framed(s2, e2)
    rows, want = want_over_spans(tree, frames, fends)
    status = want[tree.column("#status").index].reshape(-1)
    assert all(status[i] != 0 for i in (1, 64, 129)) and not status[[0, 2, 63, 65, 128]].any()
    check(tree, frames, fends, dev, f"cut {what} {cut} {kernel}", (rows, want))


# ---- 6. garbage ends ----------------------------------------------------------------------------------------------------

def test_tree_frames_garbage_ends(dev, kernel):
    """ends[k] < ends[k-1] + 4 for one k: that record is an empty message, its neighbours decode as
    they did (a record is parsed from its end), nothing is written outside the columns."""
    tree, stream, ends, frames, fends, rows0, want0 = batch("pkg1", 130, 600)
    k = 64
    bad = fends.copy()
    bad[k] = bad[k - 1] + 2
    rows, want = want_over_spans(tree, frames, bad)
    d = TreeDecoder(tree)
    d.reserve(rows0)
    bufs, out = guarded_columns(tree, rows, dev)
    got_rows = d.run_frames(to(frames, dev), to(bad, dev), out).cpu().numpy()
    assert_guards(tree, bufs)
    assert list(got_rows) == rows
    got = [c.cpu().numpy() for c in out]
    assert mismatches(tree, got, want) == []
    # record k: an empty message (status ok, nothing present); records k - 1 and k + 1: as before
    for c, g, w0 in zip(tree.columns, got, want0):
        if c.table == 0 and c.role != 1:  # (BEGIN columns shift with k's missing elements)
            assert not g[k].any(), c.name
            assert np.array_equal(g[k - 1], w0[k - 1]) and np.array_equal(g[k + 1], w0[k + 1]), c.name

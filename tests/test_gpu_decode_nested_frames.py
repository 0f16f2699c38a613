"""GPU parity of the nested decoders over mpx frames (spec_decode_nested_frames_index,
spec_decode_nested_frames, spec_decode_nested_frames_onepass): the frames of a batch decode, in place,
to what the oracle decodes from the unframed records — every non-span column, status, item_begin and
item_status equal, every non-empty span the same bytes at the unframed offset + 4(k + 1) (k: the
record, for an item its owner) — under the schema-specialised (hiprtc) and the generic kernels, every
spec_set_nested_mode, every byte phase of the buffer, empty frames, records cut short (the head is
not record data), at the slab's edge, with big lists and at item capacity, a wide half, and end to
end through the send path and LZ4."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import NESTED, Kind, workload
from tests.gpu_helpers import concat_records, to_dev
from tests.test_gpu_nested import _wide_inputs, _wide_nested, nested_device_inputs

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 256  # canary bytes on both sides of every column
SLAB_GUARD, SLAB_MAX_CHUNKS, NESTED_SLAB_MAX = 48, 40, 163840 // 4 - 1024  # decode_core.hpp
ALL_MODES = ("index+decode", "onepass")


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    """Schema-specialised decode kernel (hiprtc) and the precompiled generic kernels."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


def framed(stream, ends):
    """(frames, frame ends int64) of the records."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    fends = ends.view(np.int64) + 4 * (np.arange(len(ends), dtype=np.int64) + 1)
    return spec_amd.make_frames(stream, ends.view(np.int64)), fends


def on_device(frames, dev, phase=0):
    """The frames in a device buffer that starts at byte `phase` of its allocation."""
    buf = torch.zeros(phase + max(frames.size, 1) + 64, dtype=torch.uint8, device=dev)
    buf[phase:phase + frames.size] = to_dev(frames, dev) if frames.size else buf[:0]
    d = buf[phase:phase + frames.size]
    assert d.data_ptr() % 4 == phase % 4
    return d


def assert_spans(got, want, owner, frames, stream, label):
    """got: spans into `frames`, want: the oracle's into `stream`, owner[i]: the span's record."""
    got = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 2).astype(np.int64)
    want = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 2).astype(np.int64)
    assert got.shape == want.shape, label
    assert np.array_equal(got[:, 1], want[:, 1]), label + ": span lengths"
    some = want[:, 1] > 0
    shift = 4 * (np.asarray(owner, np.int64) + 1)
    assert np.array_equal(got[some, 0], want[some, 0] + shift[some]), label + ": span offsets"
    for (go, ln), (wo, _) in zip(got[some][:50], want[some][:50]):
        assert bytes(frames[go:go + ln]) == bytes(stream[wo:wo + ln]), label + ": span bytes"


def compare(got, want, n, frames, stream, label):
    """A NestedColumns over `frames` against the oracle's decode of the unframed records."""
    assert np.array_equal(got.status.cpu().numpy(), want["status"]), label + ": status"
    assert np.array_equal(got.item_begin.cpu().numpy().view(np.uint32), want["item_begin"]), label + ": item_begin"
    m = int(want["item_begin"][-1]) if n else 0
    assert got.total_items == m, label + ": total_items"
    assert np.array_equal(got.outer[0].cpu().numpy(), want["id"]), label + ": id"
    assert np.array_equal(got.outer[1].cpu().numpy().view(np.int64).ravel(), want["seq"]), label + ": seq"
    assert_spans(got.outer[2].cpu().numpy(), want["name"], np.arange(n), frames, stream, label + ": name")
    if m:
        assert np.array_equal(got.item_status.cpu().numpy()[:m], want["item_status"]), label + ": item_status"
        assert np.array_equal(got.items[0][:m].cpu().numpy().view(np.int32).ravel(), want["key"]), label + ": key"
        assert np.array_equal(got.items[1][:m].cpu().numpy().view(np.uint64).ravel(),
                              want["value"].view(np.uint64)), label + ": value"
        owner = np.searchsorted(want["item_begin"], np.arange(m), side="right") - 1
        assert_spans(got.items[2][:m].cpu().numpy(), want["label"], owner, frames, stream, label + ": label")


def check_frames(dev, stream, ends, label, modes=ALL_MODES, phase=0, nested_modes=(5,), fends=None):
    """decode_nested_frames over the records' frames against the oracle on the records.  fends:
    frame ends to hand the decoder in place of the true ones (the oracle gets `ends` either way)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    n = len(ends)
    want = O.decode_nested_batch(stream, ends)
    frames, true_fends = framed(stream, ends)
    d_frames = on_device(frames, dev, phase)
    d_fends = to_dev(true_fends if fends is None else fends, dev)
    L = spec_amd.lib()
    for nm in nested_modes:
        L.spec_set_nested_mode(nm)
        try:
            for mode in modes:
                got = spec_amd.decode_nested_frames(NESTED, d_frames, d_fends, onepass=mode == "onepass")
                torch.cuda.synchronize()
                compare(got, want, n, frames, stream, f"{label} [{mode}, nested mode {nm}]")
        finally:
            L.spec_set_nested_mode(5)
    return want


# ---- 1. parity -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
def test_nested_frames_decode_parity(dev, kernel, n):
    stream, ends = O.encode_nested_batch(workload.nested(n, seed=n + 17))
    # n = 129: the count kernel, the tail-count kernel, ranges and halves are different code
    check_frames(dev, stream, ends, f"parity {kernel} n={n}", nested_modes=(1, 2, 3, 4, 5) if n == 129 else (5,))


# ---- 2. byte phase of the buffer -------------------------------------------------------------------

@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_nested_frames_decode_byte_phase(dev, kernel, phase):
    stream, ends = O.encode_nested_batch(workload.nested(200, seed=50 + phase))
    check_frames(dev, stream, ends, f"phase {kernel} {phase}", phase=phase)


# ---- 3. empty frames ---------------------------------------------------------------------------------

def test_nested_frames_decode_empty_frames(dev, kernel):
    """Records 0, 63, 64 and the last are size-0 frames (a head and nothing else); the other
    records have empty lists."""
    n = 150
    stream, ends = O.encode_nested_batch(workload.nested(n, seed=8, count=(0, 0)))
    recs = [bytes(stream[(int(ends[i - 1]) if i else 0):int(ends[i])]) for i in range(n)]
    for i in (0, 63, 64, n - 1):
        recs[i] = b""
    s2, e2 = concat_records(recs)
    want = check_frames(dev, s2, e2, f"empty frames {kernel}")
    assert int(want["item_begin"][-1]) == 0


# ---- 4. the head is not record data --------------------------------------------------------------------

def _list_first_record(rng):
    """A NESTED record written list first: the list's data starts at the record's first byte."""
    wr = O.Writer()
    wr.message()
    wr.field_list(4)
    for _ in range(3):
        wr.elem_message()
        wr.field(1, "int32", int(rng.integers(-1000, 1000)))
        wr.field(2, "float64", float(rng.standard_normal()))
        wr.field(3, "string", "lab" * int(rng.integers(0, 4)))
        assert wr.end()[1] is None
    assert wr.end()[1] is None
    wr.field(1, "bin128", bytes(range(16)))
    wr.field(2, "int64", int(rng.integers(-99, 99)))
    wr.field(3, "string", "name")
    b, err = wr.end()
    assert err is None, err
    wr.close()
    return b


@pytest.mark.parametrize("what", ["outer", "item"])
@pytest.mark.parametrize("cut", range(1, 9))
def test_nested_frames_decode_cut_records(dev, kernel, what, cut):
    """Records 1, 64 and 129 of 130 lose their first `cut` bytes: their message tables (and, for
    "item", whose records are written list first, their list tables) claim more data than the record
    holds.  A decoder that let a record's bounds start at the frame head would open cuts 1..4."""
    n = 130
    stream, ends = O.encode_nested_batch(workload.nested(n, seed=70))
    recs = [bytes(stream[(int(ends[i - 1]) if i else 0):int(ends[i])]) for i in range(n)]
    rng = np.random.default_rng(cut)
    for i in (1, 64, 129):
        r = _list_first_record(rng) if what == "item" else recs[i]
        recs[i] = r[cut:]
    s2, e2 = concat_records(recs)
    want = check_frames(dev, s2, e2, f"cut {what} {cut} {kernel}")
    assert all(want["status"][i] != 0 for i in (1, 64, 129))  # the oracle refuses them
    assert not want["status"][[0, 2, 63, 65, 128]].any()


# ---- 5. the slab's edge -----------------------------------------------------------------------------------

def _slab(total, n):
    """decode_core.hpp nested_slab_bytes(total / n): LDS bytes per wave (0: no staging)."""
    chunks = int(total / n * 64 * 1.16 / 1024.0) + 1
    if chunks > SLAB_MAX_CHUNKS:
        return 0
    s = SLAB_GUARD + chunks * 1024 + 32
    return s if s <= NESTED_SLAB_MAX else 0


def _fits(lo, hi, slab):
    """decode_core.hpp make_group: the span [lo, hi) staged from its 16-byte granule in whole 1 KiB chunks."""
    origin = lo & ~15
    granules = (hi - origin + 15) >> 4
    return slab > 0 and SLAB_GUARD + ((granules + 63) >> 6) * 1024 + 16 <= slab


def slab_edge_batch(far_over=False):
    """192 records whose middle group (records 64..127) has name lengths set so that its unframed
    span is staged, within 256 bytes under what the slab takes, and its framed span (256 bytes of
    heads more) is not; far_over: the group far over the slab both ways."""
    n = 192
    w = workload.nested(n, seed=33, count=(2, 4))
    pool = w["name_heap"].size
    w["name_heap"] = np.concatenate([w["name_heap"], np.full(4096, ord("x"), np.uint8)])

    def build(lens):
        name = w["name"].copy()
        name[64:128, 0] = pool
        name[64:128, 1] = lens
        w["name"] = name
        return O.encode_nested_batch(w, cap=1 << 20)

    if far_over:
        stream, ends = build(np.concatenate([np.full(32, 1500, np.uint32), np.full(32, 500, np.uint32)]))
        for total, head in ((int(ends[-1]), 0), (int(ends[-1]) + 4 * n, 4)):
            slab = _slab(total, n)
            pos = lambda k: (int(ends[k - 1]) if k else 0) + head * k  # noqa: E731  (record k's frame start)
            assert _fits(pos(0) + head, pos(64), slab) and _fits(pos(128) + head, pos(192), slab)  # the neighbours staged
            assert not _fits(pos(64) + head, pos(96), slab)  # not even its first half: parsed from memory
        return stream, ends
    for chunks in range(2, SLAB_MAX_CHUNKS):
        target = chunks * 1024 - 40  # the group's span, unframed
        lens = np.zeros(64, np.uint32)
        _, ends = build(lens)
        base = int(ends[127]) - int(ends[63])
        if base > target or (target - base) // 64 > 4000:
            continue
        lens[:] = (target - base) // 64
        _, ends = build(lens)
        lens[63] += target - (int(ends[127]) - int(ends[63]))
        stream, ends = build(lens)
        if int(ends[127]) - int(ends[63]) != target:
            continue  # (a length crossed a size class of the string header)
        lo, hi, total = int(ends[63]), int(ends[127]), int(ends[-1])
        slab_u, slab_f = _slab(total, n), _slab(total + 4 * n, n)
        if _fits(lo, hi, slab_u) and not _fits(lo + 4 * 64 + 4, hi + 4 * 128, slab_f) and \
                _fits(4, int(ends[63]) + 4 * 64, slab_f):
            assert hi - lo + 256 > slab_f - SLAB_GUARD - 32 - 16 >= hi - lo  # within 256 bytes under the bound
            return stream, ends
    raise AssertionError("no chunk count puts the middle group at the slab's edge")


@pytest.mark.parametrize("far_over", [False, True])
def test_nested_frames_decode_slab_edge(dev, kernel, far_over):
    stream, ends = slab_edge_batch(far_over)
    check_frames(dev, stream, ends, f"slab edge {kernel} far_over={far_over}")


# ---- 6. big lists and capacity ---------------------------------------------------------------------------------

def _guarded(dev, rows, width):
    buf = torch.full((GUARD + max(rows, 1) * width + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + max(rows, 1) * width].view(max(rows, 1), width)


def test_nested_frames_decode_big_list_and_capacity(dev, kernel):
    """One record with 300 items (a big list table) among short ones; the one-pass call with
    item_cap below the total writes items [0, item_cap) only — canaries behind every column — and
    the right *total_items; with room for all it equals the oracle."""
    n = 100
    w = workload.nested(n, seed=9, count=(0, 3))
    counts = np.diff(w["item_begin"]).astype(np.int64)
    counts[37] = 300
    from tests.test_gpu_encode_nested_frames import with_counts

    stream, ends = O.encode_nested_batch(with_counts(w, counts, 2))
    want = check_frames(dev, stream, ends, f"big list {kernel}")
    m = int(want["item_begin"][-1])
    assert m >= 300
    frames, fends = framed(stream, ends)
    d_frames, d_fends = on_device(frames, dev), to_dev(fends, dev)
    cap = 200
    d = spec_amd.NestedDecoder(NESTED, d_frames, d_fends, head=4)
    bufs = []
    outer = []
    for f, c in zip(NESTED.outer.fields, d.outer):
        if c is None:
            outer.append(None)
            continue
        b, v = _guarded(dev, n, f.width)
        bufs.append((b, n * f.width, f"outer {f.tag}"))
        outer.append(v)
    d.outer = outer
    b, v = _guarded(dev, n, 1)
    bufs.append((b, n, "status"))
    d.status = v.view(-1)
    b, v = _guarded(dev, n + 1, 4)
    bufs.append((b, 4 * (n + 1), "item_begin"))
    d.item_begin = v.view(torch.int32).view(-1)
    d.items = []
    for f in NESTED.item.fields:
        b, v = _guarded(dev, cap, f.width)
        bufs.append((b, cap * f.width, f"item {f.tag}"))
        d.items.append(v)
    b, v = _guarded(dev, cap, 1)
    bufs.append((b, cap, "item_status"))
    d.item_status = v.view(-1)
    d.item_cap = cap
    assert int(d.decode_onepass().item()) == m
    torch.cuda.synchronize()
    for b, nbytes, name in bufs:
        h = b.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + nbytes:] == CANARY).all(), name
    assert np.array_equal(d.item_begin.cpu().numpy().view(np.uint32), want["item_begin"])
    assert np.array_equal(d.status.cpu().numpy(), want["status"])
    assert np.array_equal(d.items[0].cpu().numpy().view(np.int32).ravel(), want["key"][:cap])
    assert np.array_equal(d.item_status.cpu().numpy(), want["item_status"][:cap])


# ---- 7. a wide half --------------------------------------------------------------------------------------------

def test_nested_frames_decode_wide_half(dev, kernel):
    """The 70-field item schema (decoded in chunks of 64 fields), n = 65: every non-span column
    equal to the unframed decode's, spans the same bytes 4(k + 1) further on."""
    from tests.tree_helpers import oracle_decode

    schema, tree, list_at = _wide_nested(no=10, ni=70, list_at=3)
    n = 65
    cols, heaps, rows, ws, we, outer, oh, items, ih, ib = _wide_inputs(tree, schema, list_at, n, 961, dev)
    wrows, want = oracle_decode(tree, ws, we)
    wcol = {c.name: x for c, x in zip(tree.columns, want)}
    frames, fends = framed(ws, we)
    d_frames, d_fends = on_device(frames, dev), to_dev(fends, dev)
    wib = wcol[f"o{list_at}#begin"].view(np.uint32).reshape(-1)
    owner = np.searchsorted(wib, np.arange(wrows[1]), side="right") - 1
    for onepass in (False, True):
        got = spec_amd.decode_nested_frames(schema, d_frames, d_fends, onepass=onepass)
        torch.cuda.synchronize()
        assert got.total_items == wrows[1]
        assert np.array_equal(got.item_begin.cpu().numpy().view(np.uint32), wib)
        assert not got.status.cpu().numpy().any()
        assert not got.item_status.cpu().numpy()[: wrows[1]].any()
        for i, k in enumerate(f.kind for f in schema.outer.fields):
            if k == Kind.LIST:
                continue
            g, x = got.outer[i].cpu().numpy(), wcol[f"o{i}"]
            if k in (Kind.STRING, Kind.BYTES):
                assert_spans(g, x, np.arange(n), frames, ws, f"wide outer {i}")
            else:
                assert np.array_equal(g, x.reshape(g.shape)), (onepass, i)
        for j, k in enumerate(f.kind for f in schema.item.fields):
            g, x = got.items[j].cpu().numpy()[: wrows[1]], wcol[f"o{list_at}[].w{j}"]
            if k in (Kind.STRING, Kind.BYTES):
                assert_spans(g, x, owner, frames, ws, f"wide item {j}")
            else:
                assert np.array_equal(g, x.reshape(g.shape)), (onepass, j)


# ---- 8. end to end ------------------------------------------------------------------------------------------------

def test_nested_frames_end_to_end(dev, kernel):
    """encode_nested_frames -> compress_frame -> LZ4 decompress + pack -> frames_index_device ->
    decode_nested_frames: the columns that went in."""
    from spec_amd.lz4 import compress_frame, decompress, frame_blocks

    n = 1000
    w = workload.nested(n, seed=91)
    oc, oh, ib, ic, ih = nested_device_inputs(w, dev)
    frames, _ = spec_amd.encode_nested_frames(NESTED, oc, oh, ib, ic, ih, n)
    comp = compress_frame(frames, 64 << 10, open=True, close=True).cpu().numpy()
    blocks, used, bmax, rc = frame_blocks(comp)
    assert rc == 0 and used == comp.size
    plain, _, status = decompress(to_dev(comp, dev), blocks, bmax)
    assert not status.cpu().numpy().any() and plain.numel() == frames.numel()
    fends, consumed, st = spec_amd.frames_index_device(plain, n)
    assert st == 0 and consumed == plain.numel() and fends.numel() == n
    m = len(w["key"])
    fr = plain.cpu().numpy()
    for onepass in (False, True):
        got = spec_amd.decode_nested_frames(NESTED, plain, fends, onepass=onepass)
        torch.cuda.synchronize()
        assert got.total_items == m and not got.status.cpu().numpy().any()
        assert np.array_equal(got.item_begin.cpu().numpy().view(np.uint32), w["item_begin"])
        assert np.array_equal(got.outer[0].cpu().numpy(), w["id"])
        assert np.array_equal(got.outer[1].cpu().numpy().view(np.int64).ravel(), w["seq"])
        assert np.array_equal(got.items[0][:m].cpu().numpy().view(np.int32).ravel(), w["key"])
        assert np.array_equal(got.items[1][:m].cpu().numpy().view(np.uint64).ravel(), w["value"].view(np.uint64))
        assert not got.item_status[:m].cpu().numpy().any()
        for g, x, heap in ((got.outer[2].cpu().numpy(), w["name"], w["name_heap"]),
                           (got.items[2][:m].cpu().numpy(), w["label"], w["label_heap"])):
            g = g.view(np.uint32).reshape(-1, 2)
            x = np.asarray(x).view(np.uint32).reshape(-1, 2)
            assert np.array_equal(g[:, 1], x[:, 1])
            for (go, ln), (xo, _) in list(zip(g, x))[::7]:
                assert bytes(fr[go:go + ln]) == bytes(heap[xo:xo + ln])

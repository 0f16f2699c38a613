"""GPU parity of the framed nested encoder (spec_encode_nested_frames): for the same columns its
bytes are spec_amd.make_frames over the oracle Writer's records, its ends the oracle's ends plus
4(k + 1), and both equal spec_frames_write over spec_encode_nested on the device — through the
schema-specialised (hiprtc) kernels and the generic kernels, each with the plain workspace (the
one-wave write pass) and with the `_items` workspace (the size pass's prefix cache: under "jit" the
wave-pair write pass); at the wave and block boundaries, at every output byte phase, with empty
lists, over the item cap, with big lists, around the write pass's LDS slab size, at capacity and on
encoder errors; a wide half through the tree encoder; and the receive side takes what it wrote."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import NESTED, Kind, workload
from tests.gpu_helpers import to_dev
from tests.test_gpu_nested import (GEN_ITEM, GEN_OUTER, _spans, _wide_inputs, _wide_nested, _writer_encode_generic,
                                   nested_device_inputs)

pytestmark = pytest.mark.gpu

NENC_SLAB, NENC_ITEM_CAP = 17920, 512  # encode_nested_core.hpp: a wave's LDS staging; items per wave, item-parallel
CANARY, ECANARY = 0xA5, -0x5A5A5A5A5A5A5A5B
FRONT = 16  # canary bytes before the output (keeps `offset` the output's phase in a 16-byte granule)
WORKSPACES = ["plain", "items"]


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    """Run a test with the schema-specialised kernels (hiprtc) and with the generic kernels."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


def expected(stream, ends):
    n = len(ends)
    frames = spec_amd.make_frames(stream, ends)
    fends = np.asarray(ends).view(np.int64) + 4 * (np.arange(n, dtype=np.int64) + 1)
    return frames, fends


class Call:
    """spec_encode_nested_frames (or the unframed call) over fixed device inputs with a workspace
    of exactly the plain or the `_items` size."""

    def __init__(self, dev, schema, inputs, n, workspace):
        self.schema, self.n, self.inputs = schema, n, inputs
        oc, oh, ib, ic, ih = inputs
        self.m = int(ic[0].shape[0]) if ic else 0
        L = spec_amd.lib()
        self.ws = (L.spec_encode_nested_workspace_size(n) if workspace == "plain"
                   else L.spec_encode_nested_workspace_size_items(n, self.m))
        if workspace == "items" and self.m:
            assert self.ws > L.spec_encode_nested_workspace_size(n)
        self.workspace = torch.empty((self.ws + 7) // 8, dtype=torch.int64, device=dev)
        self.total = torch.full((1,), -7, dtype=torch.int64, device=dev)

    def __call__(self, out, ends, inputs=None, fn="spec_encode_nested_frames"):
        oc, oh, ib, ic, ih = inputs or self.inputs
        E = spec_amd.NestedEncoder
        self.total.fill_(-7)
        rc = getattr(spec_amd.lib(), fn)(
            C.byref(self.schema.c), E._ptrs(oc), *E._heaps(self.schema.outer.fields, oh), C.c_void_p(ib.data_ptr()),
            E._ptrs(ic), *E._heaps(self.schema.item.fields, ih), self.m, self.n,
            C.c_void_p(out.data_ptr() if out is not None else 0), out.numel() if out is not None else 0,
            C.c_void_p(ends.data_ptr() if ends is not None else 0), C.c_void_p(self.workspace.data_ptr()), self.ws,
            C.c_void_p(self.total.data_ptr()), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return int(self.total.item())


def check_frames(dev, schema, inputs, n, want_stream, want_ends, label, workspace, offset=0):
    """The framed call into a canary-filled buffer at byte phase `offset`, frame ends into a
    canary-padded tensor; against the oracle and against encode_nested + write_frames."""
    want, wends = expected(want_stream, want_ends)
    call = Call(dev, schema, inputs, n, workspace)
    total = want.size
    assert call(None, None) == total, f"{label}: size only"
    buf = torch.full((FRONT + offset + total + 64,), CANARY, dtype=torch.uint8, device=dev)
    ebuf = torch.full((n + 16,), ECANARY, dtype=torch.int64, device=dev)
    out = buf[FRONT + offset: FRONT + offset + total]
    assert out.data_ptr() % 16 == offset
    fends = ebuf[8: 8 + n]
    assert call(out, fends) == total, f"{label}: *total"
    ge = fends.cpu().numpy()
    if not np.array_equal(ge, wends):
        i = int(np.nonzero(ge != wends)[0][0])
        raise AssertionError(f"{label}: frame_ends[{i}] gpu={ge[i]} want={wends[i]}")
    go = out.cpu().numpy()
    if not np.array_equal(go, want):
        j = int(np.nonzero(go != want)[0][0])
        i = int(np.searchsorted(wends, j, side="right"))
        s = int(wends[i - 1]) if i else 0
        e = min(int(wends[i]), s + 400)
        raise AssertionError(f"{label}: byte {j} (frame {i}, +{j - s}) gpu={go[j]:#x} want={want[j]:#x}\n"
                             f"gpu ={go[s:e].tobytes().hex()}\nwant={want[s:e].tobytes().hex()}")
    whole, ewhole = buf.cpu().numpy(), ebuf.cpu().numpy()
    assert (whole[:FRONT + offset] == CANARY).all(), f"{label}: bytes before frames[0] written"
    assert (whole[FRONT + offset + total:] == CANARY).all(), f"{label}: bytes past frames[total] written"
    assert (ewhole[:8] == ECANARY).all() and (ewhole[8 + n:] == ECANARY).all(), f"{label}: frame_ends overrun"
    # the two-pass send path on the device writes the same bytes and ends (and the unframed
    # encoder, through the same workspace, still writes the oracle's stream)
    plain = torch.empty(max(want_stream.size, 1), dtype=torch.uint8, device=dev)
    pends = torch.empty(n, dtype=torch.int64, device=dev)
    assert call(plain, pends, fn="spec_encode_nested") == want_stream.size, f"{label}: unframed *total"
    assert np.array_equal(plain[:want_stream.size].cpu().numpy(), want_stream), f"{label}: unframed bytes"
    two, two_ends = spec_amd.write_frames(plain[:want_stream.size], pends)
    torch.cuda.synchronize()
    assert torch.equal(out, two), f"{label}: differs from write_frames(encode_nested)"
    assert torch.equal(fends, two_ends), f"{label}: ends differ from write_frames(encode_nested)"
    return out.clone(), fends.clone()


def check_workload(dev, w, label, workspace, offset=0):
    n = len(w["seq"])
    stream, ends = O.encode_nested_batch(w)
    return check_frames(dev, NESTED, nested_device_inputs(w, dev), n, stream, ends, label, workspace, offset), (stream, ends)


def with_counts(w, counts, seed, lens=None):
    """w with its item lists replaced: `counts` items per record, fresh item columns."""
    counts = np.asarray(counts, np.int64)
    rng = np.random.default_rng(seed)
    m = int(counts.sum())
    ib = np.zeros(len(counts) + 1, np.uint32)
    np.cumsum(counts, out=ib[1:])
    if lens is None:
        lens = rng.integers(0, 12, m).astype(np.uint32)
    label = np.zeros((m, 2), np.uint32)
    if m:
        label[1:, 0] = np.cumsum(lens[:-1])
    label[:, 1] = lens
    w = dict(w)
    w.update(item_begin=ib, key=rng.integers(-2**31, 2**31, m).astype(np.int32), value=rng.standard_normal(m),
             label=label, label_heap=rng.integers(32, 127, int(np.sum(lens)), dtype=np.uint8))
    return w


# ---- 1. wave and block boundaries ------------------------------------------------------------

@pytest.mark.parametrize("workspace", WORKSPACES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_nested_frames_parity(dev, kernel, workspace, n):
    check_workload(dev, workload.nested(n, seed=n + 5), f"nested {kernel} {workspace} n={n}", workspace)


# ---- 2. output byte phase ------------------------------------------------------------------------

@pytest.mark.parametrize("workspace", WORKSPACES)
@pytest.mark.parametrize("offset", [0, 1, 3, 8, 15])
def test_nested_frames_byte_phase(dev, kernel, workspace, offset):
    check_workload(dev, workload.nested(321, seed=offset + 40), f"nested {kernel} {workspace} offset={offset}",
                   workspace, offset=offset)


@pytest.mark.parametrize("workspace", WORKSPACES)
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_list_first_field_frames(dev, kernel, workspace, offset):
    """A schema whose list is the FIRST outer field: the head lies directly below the first item,
    whose 4-byte head store may cover up to 3 of its bytes; item tags > 255, a repeated item tag;
    a wave over the item cap, a big list by count, a wave that does not fit the slab."""
    schema = spec_amd.NestedSchema(GEN_OUTER, GEN_ITEM)
    rng = np.random.default_rng(77 + offset)
    n = 200
    counts = rng.integers(0, 7, n)
    counts[64:128] = 10          # a wave over the item cap (per-lane path)
    counts[3] = 300              # a big list by count
    slen = rng.integers(0, 30, n).astype(np.uint32)
    slen[150] = 20000            # a wave whose output does not fit the LDS slab
    ib = np.zeros(n + 1, np.uint32)
    np.cumsum(counts, out=ib[1:])
    m = int(ib[-1])
    c = {"item_begin": ib, "byte": rng.integers(0, 256, n, dtype=np.uint8),
         "u32": rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 32, n).astype(np.uint32),
         "bool": rng.integers(0, 2, m, dtype=np.uint8), "u16": rng.integers(0, 2**16, m).astype(np.uint16),
         "bin": rng.integers(0, 256, (m, 8), dtype=np.uint8), "i16": rng.integers(-2**15, 2**15, m).astype(np.int16)}
    c["str"], c["str_heap"] = _spans(rng, slen)
    c["bytes"], c["bytes_heap"] = _spans(rng, rng.integers(0, 9, m).astype(np.uint32))
    want, want_ends = _writer_encode_generic(c)
    outer = [None, to_dev(c["byte"], dev), to_dev(c["str"], dev), to_dev(c["u32"], dev)]
    items = [to_dev(c["bool"], dev), to_dev(c["u16"], dev), to_dev(c["bin"], dev), to_dev(c["bytes"], dev),
             to_dev(c["i16"], dev)]
    inputs = (outer, {2: to_dev(c["str_heap"], dev)}, to_dev(ib.view(np.int32), dev), items,
              {3: to_dev(c["bytes_heap"], dev)})
    check_frames(dev, schema, inputs, n, want, want_ends, f"list first {kernel} {workspace} offset={offset}", workspace,
                 offset=offset)


# ---- 3. empty lists, the item cap, big lists ---------------------------------------------------------

@pytest.mark.parametrize("workspace", WORKSPACES)
def test_nested_frames_empty_lists(dev, kernel, workspace):
    w = workload.nested(300, seed=8, count=(0, 0))
    assert int(w["item_begin"][-1]) == 0
    check_workload(dev, w, f"empty lists {kernel} {workspace}", workspace, offset=1)


@pytest.mark.parametrize("workspace", WORKSPACES)
@pytest.mark.parametrize("shape", ["one_record", "one_wave"])
def test_nested_frames_item_cap(dev, kernel, workspace, shape):
    """One record with 513 items, and a wave whose 64 records own 513 items together: one more
    than NENC_ITEM_CAP, so those waves take the per-lane path among item-parallel neighbours."""
    n = 200
    w = workload.nested(n, seed=21, count=(0, 6))
    counts = np.diff(w["item_begin"]).astype(np.int64)
    if shape == "one_record":
        counts[70] = NENC_ITEM_CAP + 1
    else:
        counts[64:128] = 8
        counts[100] = 9
        assert counts[64:128].sum() == NENC_ITEM_CAP + 1
    check_workload(dev, with_counts(w, counts, 5), f"item cap {shape} {kernel} {workspace}", workspace, offset=3)


@pytest.mark.parametrize("workspace", WORKSPACES)
def test_nested_frames_big_lists(dev, kernel, workspace):
    """A list of 300 items (IsBigList by count) and one of more than 65,535 data bytes (by offset;
    its one long item has a big table too)."""
    n = 200
    w = workload.nested(n, seed=9, count=(0, 3))
    counts = np.diff(w["item_begin"]).astype(np.int64)
    counts[5], counts[7], counts[11] = 300, 0, 2
    m = int(counts.sum())
    lens = np.random.default_rng(1).integers(0, 12, m).astype(np.uint32)
    lens[int(counts[:11].sum())] = 70000
    w = with_counts(w, counts, 2, lens=lens)
    (_, _), (stream, ends) = check_workload(dev, w, f"big lists {kernel} {workspace}", workspace, offset=8)
    assert int(ends[11]) - int(ends[10]) > 65535


# ---- 4. the slab fit ---------------------------------------------------------------------------------

def slab_fit_batch():
    """192 records; the middle wave's (records 64..127) name lengths are set so that its unframed
    span U fits the slab at any 16-byte phase (15 + U + 16 <= NENC_SLAB) and its framed span
    U + 256 at none (U + 256 + 16 > NENC_SLAB)."""
    n = 192
    w = workload.nested(n, seed=33, count=(2, 4))
    assert int(w["item_begin"][128] - w["item_begin"][64]) <= NENC_ITEM_CAP  # item-parallel: the slab decides
    pool = w["name_heap"].size
    w["name_heap"] = np.concatenate([w["name_heap"], np.full(2048, ord("x"), np.uint8)])
    target = NENC_SLAB - 31 - 100

    def group_span(lens):
        name = w["name"].copy()
        name[64:128, 0] = pool
        name[64:128, 1] = lens
        w["name"] = name
        _, ends = O.encode_nested_batch(w)
        return int(ends[127]) - int(ends[63])

    lens = np.zeros(64, np.uint32)
    lens[:] = (target - group_span(lens)) // 64
    lens[63] += target - group_span(lens)
    u = group_span(lens)
    assert u + 31 <= NENC_SLAB < u + 256 + 16, u
    return w


@pytest.mark.parametrize("workspace", WORKSPACES)
@pytest.mark.parametrize("offset", [0, 15])
def test_nested_frames_slab_fit(dev, kernel, workspace, offset):
    """A 64-record group that is staged unframed and takes the straight-to-memory path framed:
    the same bytes."""
    check_workload(dev, slab_fit_batch(), f"slab fit {kernel} {workspace} offset={offset}", workspace, offset=offset)


# ---- 5. capacity and encoder errors -------------------------------------------------------------------

@pytest.mark.parametrize("workspace", WORKSPACES)
def test_nested_frames_capacity_and_errors(dev, kernel, workspace):
    n = 300
    w = workload.nested(n, seed=4)
    stream, ends = O.encode_nested_batch(w)
    want, wends = expected(stream, ends)
    total = want.size
    inputs = nested_device_inputs(w, dev)
    oc, oh, ib, ic, ih = inputs
    call = Call(dev, NESTED, inputs, n, workspace)
    buf = torch.full((total + 64,), CANARY, dtype=torch.uint8, device=dev)
    ebuf = torch.full((n + 16,), ECANARY, dtype=torch.int64, device=dev)

    def untouched():
        return bool((buf == CANARY).all()) and bool((ebuf == ECANARY).all())

    # one byte short: nothing written, *total the framed size
    assert call(buf[:total - 1], ebuf[8:8 + n]) == total
    assert untouched()
    # an item string outside its heap: *total all-ones, nothing written
    bad = w["label"].copy()
    bad[len(bad) // 2, 0] = w["label_heap"].size + 1
    assert call(buf[:total], ebuf[8:8 + n], inputs=(oc, oh, ib, [ic[0], ic[1], to_dev(bad, dev)], ih)) == -1
    assert untouched()
    # an outer string outside its heap
    badn = w["name"].copy()
    badn[n - 3, 1] = 1 << 20
    oc2 = list(oc)
    oc2[2] = to_dev(badn.view(np.uint8).reshape(n, 8), dev)
    assert call(buf[:total], ebuf[8:8 + n], inputs=(oc2, oh, ib, ic, ih)) == -1
    assert untouched()
    # item_begin not monotonic
    ib2 = w["item_begin"].copy()
    ib2[100] = ib2[102] + 1
    assert call(buf[:total], ebuf[8:8 + n], inputs=(oc, oh, to_dev(ib2.view(np.int32), dev), ic, ih)) == -1
    assert untouched()
    # exactly enough: written (the paths above left the workspace reusable)
    assert call(buf[:total], ebuf[8:8 + n]) == total
    assert np.array_equal(buf[:total].cpu().numpy(), want)
    assert np.array_equal(ebuf[8:8 + n].cpu().numpy(), wends)
    assert bool((buf[total:] == CANARY).all())


# ---- 6. a wide half: the tree route -----------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 3])
def test_nested_frames_wide_half(dev, kernel, offset):
    """A 70-field item schema goes through the tree encoder; its framed form through the framed
    tree encoder: the tree oracle's records behind their heads."""
    schema, tree, list_at = _wide_nested(no=10, ni=70, list_at=3)
    n = 130
    cols, heaps, rows, ws, we, outer, oh, items, ih, ib = _wide_inputs(tree, schema, list_at, n, 960, dev)
    check_frames(dev, schema, (outer, oh, ib, items, ih), n, ws, we, f"wide half {kernel} offset={offset}", "plain",
                 offset=offset)


# ---- 7. the receive side and the wrappers ---------------------------------------------------------------------

@pytest.mark.parametrize("workspace", WORKSPACES)
def test_receive_side_accepts_nested_frames(dev, kernel, workspace):
    n = 1000
    (frames, fends), _ = check_workload(dev, workload.nested(n, seed=77), f"receive {kernel} {workspace}", workspace)
    ends, consumed, status = spec_amd.frames_index_device(frames)
    assert status == 0 and ends.numel() == n and consumed == frames.numel()
    assert torch.equal(ends, fends)
    st, _ = spec_amd.parse_messages(frames, fends, head=4)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0


def test_encode_nested_frames_wrapper(dev, kernel):
    n = 500
    w = workload.nested(n, seed=12)
    want, wends = expected(*O.encode_nested_batch(w))
    oc, oh, ib, ic, ih = nested_device_inputs(w, dev)
    frames, fends = spec_amd.encode_nested_frames(NESTED, oc, oh, ib, ic, ih, n)
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), want)
    assert np.array_equal(fends.cpu().numpy(), wends)
    bad = w["label"].copy()
    bad[len(bad) // 2, 1] = 1 << 20
    with pytest.raises(spec_amd.SpecError):
        spec_amd.encode_nested_frames(NESTED, oc, oh, ib, [ic[0], ic[1], to_dev(bad, dev)], ih, n)
    # n == 0: *total = 0 and nothing else
    w0 = workload.nested(0, seed=1)
    enc = spec_amd.NestedEncoder(NESTED, 0, dev)
    enc.total.fill_(-7)
    buf = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    ib0 = to_dev(w0["item_begin"].view(np.int32), dev)
    assert int(enc.encode_frames([buf, buf, buf, None], {2: buf}, ib0, [None] * 3, {2: buf}, 0, buf[32:32],
                                 None).item()) == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())

"""GPU parity of the fused framed encoder (spec_encode_flat_frames): for the same columns its
bytes are spec_amd.make_frames over the oracle Writer's records, its ends the oracle's ends plus
4(k + 1), and both equal spec_frames_write over spec_encode_flat on the device — through the
schema-specialised (hiprtc) kernels, the generic kernels and the wide kernels; at every output
alignment, around the write pass's LDS slab size, at capacity and on encoder errors; and the
receive side (frames_index_device, decode_frames, parse_messages(head=4)) takes what it wrote."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import spec_amd
from spec_amd import Kind, Schema, workload
from tests.gpu_helpers import oracle_encode, to_dev

pytestmark = pytest.mark.gpu

FLAT16 = spec_amd.FLAT16
ALL_KINDS = [Kind(k) for k in range(1, 16)]
ENC_SLAB = 20 * 1024 - 128  # encode_core.hpp: a wave's LDS staging; a span over it goes straight to HBM
CANARY, ECANARY = 0xA5, -0x5A5A5A5A5A5A5A5B
FRONT = 16  # canary bytes before the output (keeps `offset` the output's phase in a 16-byte granule)


def wide_schema(nf, tag0=1, step=1, perm_seed=None):
    """nf fields cycling through every kind, write order permuted (as tests/test_gpu_wide.py)."""
    tags = [tag0 + step * i for i in range(nf)]
    if perm_seed is not None:
        tags = list(np.random.default_rng(perm_seed).permutation(tags))
    return Schema([(int(t), ALL_KINDS[i % len(ALL_KINDS)]) for i, t in enumerate(tags)])


SCHEMAS = {
    "flat16": FLAT16,                               # the hiprtc SpecEnc kernels (or RuntimeEnc: `kernel`)
    "wide40": wide_schema(40, perm_seed=3),         # over ENC_MAX_FIELDS = 32: always RuntimeEnc
    "wide72": wide_schema(72, perm_seed=13),        # over SPEC_KFIELDS = 64: the wide kernels
    "big_mixed": Schema([(1, Kind.INT64), (300, Kind.STRING), (2, Kind.FLOAT64), (4000, Kind.BIN128),
                         (70, Kind.UINT32), (65535, Kind.BOOL), (256, Kind.BYTES), (255, Kind.INT16)]),
}


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    """Run a test with the schema-specialised kernels (hiprtc) and with the generic kernel."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


def expected(schema, cols, heaps, n):
    stream, ends = oracle_encode(schema, cols, heaps, n)
    frames = spec_amd.make_frames(stream, ends)
    fends = ends.view(np.int64) + 4 * (np.arange(n, dtype=np.int64) + 1)
    return stream, ends, frames, fends


def device_inputs(dev, cols, heaps):
    d_cols = [to_dev(c, dev) for c in cols]
    d_heaps = {f: to_dev(h if h.size else np.zeros(1, np.uint8), dev) for f, h in heaps.items()}
    return d_cols, d_heaps


def check_frames(dev, schema, cols, heaps, n, label, offset=0):
    """spec_encode_flat_frames into a canary-filled buffer at byte phase `offset`, frame ends into
    a canary-padded tensor; against the oracle and against encode_flat + write_frames."""
    want_stream, _, want_frames, want_fends = expected(schema, cols, heaps, n)
    d_cols, d_heaps = device_inputs(dev, cols, heaps)
    enc = spec_amd.Encoder(schema, n, dev)
    unframed = int(enc.size(d_cols).item())
    assert unframed == want_stream.size, f"{label}: size pass {unframed} oracle {want_stream.size}"
    total = unframed + 4 * n
    buf = torch.full((FRONT + offset + total + 64,), CANARY, dtype=torch.uint8, device=dev)
    ebuf = torch.full((n + 16,), ECANARY, dtype=torch.int64, device=dev)
    out = buf[FRONT + offset: FRONT + offset + total]
    assert out.data_ptr() % 16 == offset
    fends = ebuf[8: 8 + n]
    enc.encode_frames_into(d_cols, d_heaps, out, fends)
    torch.cuda.synchronize()
    assert int(enc.total.item()) == total, f"{label}: *total {int(enc.total.item())} want {total}"
    ge = fends.cpu().numpy()
    if not np.array_equal(ge, want_fends):
        i = int(np.nonzero(ge != want_fends)[0][0])
        raise AssertionError(f"{label}: frame_ends[{i}] gpu={ge[i]} want={want_fends[i]}")
    go = out.cpu().numpy()
    if not np.array_equal(go, want_frames):
        j = int(np.nonzero(go != want_frames)[0][0])
        i = int(np.searchsorted(want_fends, j, side="right"))
        s = int(want_fends[i - 1]) if i else 0
        raise AssertionError(f"{label}: byte {j} (frame {i}, +{j - s}) gpu={go[j]:#x} want={want_frames[j]:#x}\n"
                             f"gpu ={go[s:int(want_fends[i])].tobytes().hex()}\n"
                             f"want={want_frames[s:int(want_fends[i])].tobytes().hex()}")
    whole, ewhole = buf.cpu().numpy(), ebuf.cpu().numpy()
    assert (whole[:FRONT + offset] == CANARY).all(), f"{label}: bytes before frames[0] written"
    assert (whole[FRONT + offset + total:] == CANARY).all(), f"{label}: bytes past frames[total] written"
    assert (ewhole[:8] == ECANARY).all() and (ewhole[8 + n:] == ECANARY).all(), f"{label}: frame_ends overrun"
    # the two-pass send path on the device writes the same bytes and ends
    two, two_ends = spec_amd.write_frames(*spec_amd.encode_flat(schema, d_cols, d_heaps, n))
    torch.cuda.synchronize()
    assert torch.equal(out, two), f"{label}: differs from write_frames(encode_flat)"
    assert torch.equal(fends, two_ends), f"{label}: ends differ from write_frames(encode_flat)"
    return out.clone(), fends.clone()


def long_field(schema, cols, heaps, rec, nbytes, seed=1):
    """Point record rec's first string/bytes field at nbytes new heap bytes."""
    f = next(i for i, fld in enumerate(schema.fields) if fld.kind in (Kind.STRING, Kind.BYTES))
    extra = np.random.default_rng(seed).integers(97, 123, size=nbytes, dtype=np.uint8)
    sp = cols[f].view(np.uint32).reshape(-1, 2).copy()
    sp[rec] = (heaps[f].size, nbytes)
    heaps[f] = np.concatenate([heaps[f], extra])
    cols[f] = sp.view(np.uint8).reshape(-1, 8)


# ---- 1. parity across the three encoders -------------------------------------------------

NS = [1, 63, 64, 65, 255, 256, 257, 1000]  # wave boundaries and the ENC_BLOCK boundary


@pytest.mark.parametrize("n", NS)
def test_flat16_frames_parity(dev, kernel, n):
    cols, heaps = workload.flat16(n, seed=n + 3)
    check_frames(dev, FLAT16, cols, heaps, n, f"flat16 {kernel} n={n}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["wide40", "wide72"])
def test_generic_and_wide_frames_parity(dev, name, n):
    s = SCHEMAS[name]
    cols, heaps = workload.gen_columns(s, n, seed=n + len(name), str_len=(0, 40))
    check_frames(dev, s, cols, heaps, n, f"{name} n={n}")


@pytest.mark.parametrize("name", ["flat16", "big_mixed", "wide72"])
def test_big_tables_frames_parity(dev, kernel, name):
    """Tags > 255 (big_mixed: every table big) and one record of more than 65,535 data bytes
    (its table big among small ones): the 6-byte table entries sit behind the head."""
    s = SCHEMAS[name]
    n = 257
    cols, heaps = workload.gen_columns(s, n, seed=31, str_len=(0, 50))
    long_field(s, cols, heaps, 70, 70_000)
    check_frames(dev, s, cols, heaps, n, f"{name} {kernel} big tables")


# ---- 2. alignment and bounds --------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1, 3, 8, 15])
@pytest.mark.parametrize("name", ["flat16", "wide40", "wide72"])
def test_frames_alignment_and_bounds(dev, kernel, name, offset):
    s = SCHEMAS[name]
    n = 321
    cols, heaps = workload.gen_columns(s, n, seed=offset + 40, str_len=(0, 62))
    check_frames(dev, s, cols, heaps, n, f"{name} {kernel} offset={offset}", offset=offset)


# ---- 3. groups over the slab ---------------------------------------------------------------

def over_slab_mix(n):
    """tests/test_gpu_flat.py test_encode_pair_groups_over_slab's mix: whole 64-record groups of
    300-700-byte strings (over the slab) among staged groups, single long records inside staged
    groups — plus group 4 sized to fit the slab unframed but not with its 64 heads."""
    a_cols, a_heaps = workload.flat16(n, seed=21)
    b_cols, b_heaps = workload.gen_columns(FLAT16, n, 22, str_len=(300, 700))
    big = np.zeros(n, bool)
    for g in (2, 9, (n - 1) // 64):
        big[64 * g: 64 * g + 64] = True
    big[5::97] = True
    big[256:320] = False  # group 4 is sized below
    cols = [np.where(big[:, None], b, a) for a, b in zip(a_cols, b_cols)]
    heaps = {}
    for f, h in a_heaps.items():
        heaps[f] = np.concatenate([h, b_heaps[f]])
        sp = cols[f].view(np.uint32).reshape(n, 2).copy()
        sp[big, 0] += h.size
        cols[f] = sp.view(np.uint8).reshape(n, 8)
    # group 4 (records 256..319, one wave): its string lengths set so that the unframed span U
    # satisfies ENC_SLAB - 32 - 256 + 16 < U < ENC_SLAB - 32.  The wave stages its span when
    # head + span + 16 <= ENC_SLAB with head <= 15: U fits at any head, U + 256 at none.
    f = next(i for i, fld in enumerate(FLAT16.fields) if fld.kind == Kind.STRING)
    pool = heaps[f].size
    heaps[f] = np.concatenate([heaps[f], np.full(4096, ord("x"), np.uint8)])
    target = ENC_SLAB - 32 - 120

    def group_span(lens):
        sp = cols[f].view(np.uint32).reshape(n, 2).copy()
        sp[256:320, 0] = pool
        sp[256:320, 1] = lens
        cols[f] = sp.view(np.uint8).reshape(n, 8)
        _, ends = oracle_encode(FLAT16, cols, heaps, n)
        return int(ends[319]) - int(ends[255])

    lens = np.zeros(64, np.uint32)
    lens[:] = (target - group_span(lens)) // 64
    lens[63] += target - group_span(lens)
    u = group_span(lens)
    assert ENC_SLAB - 32 - 256 + 16 < u < ENC_SLAB - 32, u
    return cols, heaps


def test_frames_groups_over_slab(dev, kernel):
    n = 1000
    cols, heaps = over_slab_mix(n)
    check_frames(dev, FLAT16, cols, heaps, n, f"flat16 {kernel} over-slab groups", offset=15)


def test_frames_groups_over_slab_wide(dev):
    """The same threshold through RuntimeEnc's wide kernels: 64 records of a 72-field schema
    with 300-700-byte strings exceed the slab, the short-string groups around them do not."""
    s = SCHEMAS["wide72"]
    n = 1000
    a_cols, a_heaps = workload.gen_columns(s, n, seed=5, str_len=(0, 8))
    b_cols, b_heaps = workload.gen_columns(s, n, seed=6, str_len=(300, 700))
    big = np.zeros(n, bool)
    big[128:192] = True
    big[7::131] = True
    cols = [np.where(big[:, None], b, a) for a, b in zip(a_cols, b_cols)]
    heaps = {}
    for f, h in a_heaps.items():
        heaps[f] = np.concatenate([h, b_heaps[f]])
        sp = cols[f].view(np.uint32).reshape(n, 2).copy()
        sp[big, 0] += h.size
        cols[f] = sp.view(np.uint8).reshape(n, 8)
    check_frames(dev, s, cols, heaps, n, "wide72 over-slab groups", offset=3)


# ---- 4. capacity and errors ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flat16", "wide40", "wide72"])
def test_frames_capacity_and_errors(dev, kernel, name):
    s = SCHEMAS[name]
    n = 300
    cols, heaps = workload.gen_columns(s, n, seed=9, str_len=(0, 40))
    d_cols, d_heaps = device_inputs(dev, cols, heaps)
    enc = spec_amd.Encoder(s, n, dev)
    total = int(enc.size(d_cols).item()) + 4 * n
    buf = torch.full((total + 64,), CANARY, dtype=torch.uint8, device=dev)
    ebuf = torch.full((n + 16,), ECANARY, dtype=torch.int64, device=dev)
    # one byte short: nothing written, *total the framed size
    enc.encode_frames_into(d_cols, d_heaps, buf[:total - 1], ebuf[8:8 + n])
    torch.cuda.synchronize()
    assert int(enc.total.item()) == total
    assert bool((buf == CANARY).all()) and bool((ebuf == ECANARY).all())
    # a span outside its heap: *total all-ones, nothing written
    f = next(i for i, fld in enumerate(s.fields) if fld.kind in (Kind.STRING, Kind.BYTES))
    bad = cols[f].copy()
    bad.view(np.uint32).reshape(n, 2)[n - 3, 0] = heaps[f].size + 1
    bad_cols = list(d_cols)
    bad_cols[f] = to_dev(bad, dev)
    enc.encode_frames_into(bad_cols, d_heaps, buf[:total], ebuf[8:8 + n])
    torch.cuda.synchronize()
    assert int(enc.total.item()) == -1  # all-ones as int64
    assert bool((buf == CANARY).all()) and bool((ebuf == ECANARY).all())
    # exactly enough: written (and the capacity path above left the encoder reusable)
    enc.encode_frames_into(d_cols, d_heaps, buf[:total], ebuf[8:8 + n])
    torch.cuda.synchronize()
    _, _, want_frames, want_fends = expected(s, cols, heaps, n)
    assert int(enc.total.item()) == total
    assert np.array_equal(buf[:total].cpu().numpy(), want_frames)
    assert np.array_equal(ebuf[8:8 + n].cpu().numpy(), want_fends)
    assert bool((buf[total:] == CANARY).all())


# ---- 5. the receive side accepts the frames -----------------------------------------------------

def test_receive_side_accepts_frames(dev, kernel):
    n = 1000
    cols, heaps = workload.flat16(n, seed=77)
    frames, fends = check_frames(dev, FLAT16, cols, heaps, n, f"flat16 {kernel} receive")
    ends, consumed, status = spec_amd.frames_index_device(frames)
    assert status == 0 and ends.numel() == n and consumed == frames.numel()
    assert torch.equal(ends, fends)
    got = spec_amd.decode_frames(FLAT16, frames, fends)
    st, _ = spec_amd.parse_messages(frames, fends, head=4)
    torch.cuda.synchronize()
    assert int((got.status != 0).sum()) == 0
    assert int((st != 0).sum()) == 0
    fr = frames.cpu().numpy()
    for f, fld in enumerate(FLAT16.fields):
        g = got.cols[f].cpu().numpy()
        if fld.kind in (Kind.STRING, Kind.BYTES):
            gs, ws = g.view(np.uint32).reshape(n, 2), cols[f].view(np.uint32).reshape(n, 2)
            assert np.array_equal(gs[:, 1], ws[:, 1]), fld
            for i in range(n):
                assert np.array_equal(fr[gs[i, 0]:gs[i, 0] + gs[i, 1]], heaps[f][ws[i, 0]:ws[i, 0] + ws[i, 1]]), (fld, i)
        else:
            assert np.array_equal(g, cols[f]), fld


# ---- 6. the Python wrappers ------------------------------------------------------------------

def test_encode_flat_frames_wrapper(dev, kernel):
    n = 500
    cols, heaps = workload.flat16(n, seed=12)
    _, _, want_frames, want_fends = expected(FLAT16, cols, heaps, n)
    d_cols, d_heaps = device_inputs(dev, cols, heaps)
    frames, fends = spec_amd.encode_flat_frames(FLAT16, d_cols, d_heaps)
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), want_frames)
    assert np.array_equal(fends.cpu().numpy(), want_fends)
    # an encoder error raises, as encode_flat does
    f = next(i for i, fld in enumerate(FLAT16.fields) if fld.kind == Kind.STRING)
    bad = cols[f].copy()
    bad.view(np.uint32).reshape(n, 2)[5, 0] = heaps[f].size
    bad_cols = list(d_cols)
    bad_cols[f] = to_dev(bad, dev)
    with pytest.raises(spec_amd.SpecError):
        spec_amd.encode_flat_frames(FLAT16, bad_cols, d_heaps, n)
    # n == 0: an empty result
    e_cols = [c[:0] for c in d_cols]
    frames0, fends0 = spec_amd.encode_flat_frames(FLAT16, e_cols, d_heaps, 0)
    torch.cuda.synchronize()
    assert frames0.numel() == 0 and fends0.numel() == 0

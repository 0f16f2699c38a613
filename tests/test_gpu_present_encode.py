"""GPU parity of spec_encode_flat_present / spec_encode_flat_present_frames: record i holds exactly
the fields of its mask, as the oracle Writer writes them (w.Field(tag).<Kind>(v) for those alone,
then Build()) — stream, ends and *total bit exact, unframed and as mpx frames, at the wave and
block edges of the encoder; the per-record big-table rule, garbage spans of absent fields, table
order with absent entries, a repeated tag, two mask words on the wide kernels, a group over the
write slab, capacity, size-only calls, every byte phase of `out`, and the decode -> encode round
trip of a sparse batch."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import spec_amd
from spec_amd import FLAT16, NESTED, Kind, Schema
from tests.gpu_helpers import concat_records, to_dev
from tests.present_helpers import (PATTERNS, check_encode_present, encode_present_abi, oracle_sparse_stream, pack_mask,
                                   patterns, random_columns, write_sparse)

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 255, 256, 257, 300]  # the wave and ENC_BLOCK edges
COMPACT = NESTED.item
ALL_ONES = np.uint64(2**64 - 1)


# ---- 1. the mask patterns ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["flat16", "compact"])
def test_patterns(dev, name, n):
    schema = FLAT16 if name == "flat16" else COMPACT
    cols, heaps = random_columns(schema, n, n)
    for p in PATTERNS:
        bits = patterns(len(schema), n)[p]
        want, want_ends = check_encode_present(dev, schema, cols, heaps, bits, n, f"{name} {p} n={n}")
        if p == "none":  # n records of 00 00 50
            assert want.tobytes() == bytes([0, 0, 80]) * n
        if p == "all":  # byte-identical to the dense encoder on the device
            out, ends = spec_amd.encode_flat(schema, [to_dev(c, dev) for c in cols],
                                             {f: to_dev(h, dev) for f, h in heaps.items()}, n)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(ends.cpu().numpy().view(np.uint64), want_ends)


def test_wrappers(dev):
    n = 257
    cols, heaps = random_columns(FLAT16, n, 3)
    bits = patterns(16, n)["half1"]
    bits[:, 14] |= True
    d_cols = [to_dev(c, dev) for c in cols]
    d_heaps = {f: to_dev(h, dev) for f, h in heaps.items()}
    d_mask = to_dev(pack_mask(bits)[0].view(np.int64), dev)
    for frames in (False, True):
        want, want_ends = oracle_sparse_stream(FLAT16, cols, heaps, bits, n, frames)
        out, ends = spec_amd.encode_flat_present(FLAT16, d_cols, d_heaps, d_mask, frames=frames)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(ends.cpu().numpy().view(np.uint64), want_ends)
    # bits at or above nfields are ignored
    hi = to_dev((pack_mask(bits)[0] | np.uint64(0xFFFF0000)).view(np.int64), dev)
    out, _ = spec_amd.encode_flat_present(FLAT16, d_cols, d_heaps, hi)
    assert np.array_equal(out.cpu().numpy(), oracle_sparse_stream(FLAT16, cols, heaps, bits, n)[0])


# ---- 2. IsBigMessage per record ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 300])
def test_big_table_where_the_big_tag_is_written(dev, n):
    """Tags {1, 2, 300}: a record's table is big exactly where 300 is written."""
    schema = Schema([(1, Kind.INT32), (2, Kind.STRING), (300, Kind.UINT16)])
    cols, heaps = random_columns(schema, n, 8)
    bits = patterns(3, n)["half0"]
    bits[:4] = [[1, 1, 0], [1, 1, 1], [0, 0, 1], [0, 0, 0]][: min(4, n)]
    want, want_ends = check_encode_present(dev, schema, cols, heaps, bits, n, "tags 1 2 300")
    types = want[want_ends.astype(np.int64) - 1]
    assert np.array_equal(types == 81, bits[:, 2])  # TypeBigMessage


def test_big_table_where_the_long_field_is_written(dev):
    """A 70,000-byte bytes field makes its record big when written and leaves it small when not."""
    schema = Schema([(1, Kind.INT32), (2, Kind.BYTES), (3, Kind.BOOL)])
    n = 65
    cols, heaps = random_columns(schema, n, 2)
    heaps[1] = np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8)
    cols[1] = np.tile(np.array([0, 70000], np.uint32).view(np.uint8), (n, 1))
    bits = patterns(3, n)["half2"]
    bits[:3, 1] = [True, False, True]
    want, want_ends = check_encode_present(dev, schema, cols, heaps, bits, n, "70000 bytes")
    types = want[want_ends.astype(np.int64) - 1]
    assert np.array_equal(types == 81, bits[:, 1])


# ---- 3. spans of absent and present fields ----------------------------------------------------------------

def test_garbage_span_of_an_absent_field(dev):
    """An absent string/bytes field with {off, len} past its heap: no error, the bytes of a zero span;
    the same span in a present field: all-ones in *total, nothing written."""
    n = 130
    cols, heaps = random_columns(FLAT16, n, 6)
    bits = patterns(16, n)["half0"]
    bits[:, 13] = False
    bits[64, 14] = False
    want, want_ends = oracle_sparse_stream(FLAT16, cols, heaps, bits, n)
    bad = [c.copy() for c in cols]
    bad[13][:] = np.array([0xFFFFFF00, 0xFFFFFFF0], np.uint32).view(np.uint8)  # past the heap, > MaxSize
    bad[14][64] = np.frombuffer(np.array([heaps[14].size - 1, 2], np.uint32).tobytes(), np.uint8)
    mask = pack_mask(bits)
    for frames in (False, True):
        w, we = oracle_sparse_stream(FLAT16, cols, heaps, bits, n, frames)
        out, _, after, ends, total = encode_present_abi(dev, FLAT16, bad, heaps, mask, n, frames=frames, cap=w.size)
        assert total == w.size and np.array_equal(out, w) and np.array_equal(ends, we) and (after == 0xA5).all()
    # the one-past-the-heap span present: an encoder error
    bits[64, 14] = True
    for frames in (False, True):
        out, _, after, ends, total = encode_present_abi(dev, FLAT16, bad, heaps, pack_mask(bits), n, frames=frames,
                                                        cap=want.size + 4 * n + 64)
        assert total == 2**64 - 1
        assert (out == 0xA5).all() and (after == 0xA5).all() and (ends == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    # and the size-only call reports it too
    assert encode_present_abi(dev, FLAT16, bad, heaps, pack_mask(bits), n, out_null=True)[4] == 2**64 - 1


# ---- 4. table order ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 257])
def test_descending_write_order(dev, n):
    """Tags written in descending order: every table entry moves in front of the ones before it, so an
    absent field shifts the entries written before it, not after."""
    schema = Schema([(9, Kind.INT32), (7, Kind.STRING), (5, Kind.BOOL), (3, Kind.INT64), (1, Kind.UINT16)])
    cols, heaps = random_columns(schema, n, 11)
    for p in ("half0", "half1", "alternating", "first", "last"):
        check_encode_present(dev, schema, cols, heaps, patterns(5, n)[p], n, f"descending {p}")


def test_mixed_write_order_many_fields(dev):
    schema = Schema([(int(t), Kind.INT32) for t in np.random.default_rng(4).permutation(np.arange(1, 61))])
    n = 130
    cols, heaps = random_columns(schema, n, 12)
    check_encode_present(dev, schema, cols, heaps, patterns(60, n)["half0"], n, "60 permuted tags")


def test_repeated_tag(dev):
    """Tags [5, 5]: written later = earlier in the table; both written, and only the second."""
    schema = Schema([(5, Kind.INT32), (5, Kind.INT64), (6, Kind.BOOL)])
    n = 65
    cols, heaps = random_columns(schema, n, 13)
    bits = patterns(3, n)["half1"]
    bits[0, :2] = True
    bits[1, :2] = [False, True]
    bits[2, :2] = [True, False]
    check_encode_present(dev, schema, cols, heaps, bits, n, "tags 5 5")


# ---- 5. the wide kernels and a group over the write slab -----------------------------------------------------

@pytest.mark.parametrize("n", [65, 257])
def test_two_mask_words(dev, n):
    """100 fields (permuted tags, one > 255): two words per record, the wide kernels."""
    kinds = [Kind.INT32, Kind.BOOL, Kind.UINT64, Kind.STRING, Kind.FLOAT32]
    tags = [int(t) for t in np.random.default_rng(7).permutation(np.arange(1, 101))]
    tags[70] = 400
    schema = Schema([(t, kinds[i % 5]) for i, t in enumerate(tags)])
    cols, heaps = random_columns(schema, n, 14, str_len=(0, 12))
    for p in ("all", "none", "half0", "one_field"):
        want, want_ends = check_encode_present(dev, schema, cols, heaps, patterns(100, n)[p], n, f"100 fields {p}")
    # bits at or above nfields (bit 36 of word 1 upward) are ignored
    bits = patterns(100, n)["half1"]
    mask = pack_mask(bits)
    mask[1] |= np.uint64(0xFFFFFFF000000000)
    w, we = oracle_sparse_stream(schema, cols, heaps, bits, n)
    out, _, _, ends, total = encode_present_abi(dev, schema, cols, heaps, mask, n, cap=w.size)
    assert total == w.size and np.array_equal(out, w) and np.array_equal(ends, we)


def test_group_over_the_write_slab(dev):
    """64 records of 400-byte strings: 25 KB, over the 20 KiB slab, written straight to HBM."""
    n = 300
    cols, heaps = random_columns(FLAT16, n, 15)
    heaps[13] = np.random.default_rng(8).integers(32, 127, 4096, dtype=np.uint8)
    span = cols[13].view(np.uint32)
    span[64:128] = [17, 400]
    span[:64] = [3, 20]
    span[128:] = [1, 33]
    bits = patterns(16, n)["half2"]
    bits[64:128, 13] = True
    check_encode_present(dev, FLAT16, cols, heaps, bits, n, "over slab")


# ---- 6. capacity and placement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [False, True])
def test_capacity_and_size_only(dev, frames):
    n = 257
    cols, heaps = random_columns(FLAT16, n, 16)
    bits = patterns(16, n)["half0"]
    mask = pack_mask(bits)
    want, _ = oracle_sparse_stream(FLAT16, cols, heaps, bits, n, frames)
    # out_cap = total - 1: nothing written, *total reported
    out, _, after, ends, total = encode_present_abi(dev, FLAT16, cols, heaps, mask, n, frames=frames, cap=want.size - 1)
    assert total == want.size
    assert (out == 0xA5).all() and (after == 0xA5).all() and (ends == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    # out == NULL: sizes only
    assert encode_present_abi(dev, FLAT16, cols, heaps, mask, n, frames=frames, out_null=True)[4] == want.size
    enc = spec_amd.Encoder(FLAT16, n, dev)
    t = enc.size_present([to_dev(c, dev) for c in cols], {f: to_dev(h, dev) for f, h in heaps.items()},
                         to_dev(mask[0].view(np.int64), dev), frames=frames)
    assert int(t.item()) == want.size


@pytest.mark.parametrize("phase", [0, 1, 3])
@pytest.mark.parametrize("n", [65, 300])
def test_byte_phases(dev, n, phase):
    cols, heaps = random_columns(FLAT16, n, 17 + phase)
    check_encode_present(dev, FLAT16, cols, heaps, patterns(16, n)["half1"], n, f"phase {phase}", phase=phase)
    schema = Schema([(i + 1, Kind.INT32) for i in range(70)])
    cols, heaps = random_columns(schema, n, 18)
    check_encode_present(dev, schema, cols, heaps, patterns(70, n)["half1"], n, f"wide phase {phase}", phase=phase)


# ---- 7. the round trip: a sparse batch decoded and encoded again --------------------------------------------------

@pytest.mark.parametrize("frames", [False, True])
@pytest.mark.parametrize("n", [65, 300])
def test_round_trip(dev, n, frames):
    """The oracle's sparse Flat16 stream through decode_flat_present (frames: its mpx frames through
    decode_frames_present), then encode_flat_present with the stream itself as every string / bytes
    heap and the decoded spans as columns: the original stream and ends."""
    cols, heaps = random_columns(FLAT16, n, 19)
    bits = patterns(16, n)["half0"]
    stream, ends = concat_records(write_sparse(FLAT16, cols, heaps, bits, n))
    if frames:
        buf = to_dev(spec_amd.make_frames(stream, ends), dev)
        fends = to_dev((ends + 4 * (np.arange(n, dtype=np.uint64) + 1)).view(np.int64), dev)
        got, pm = spec_amd.decode_frames_present(FLAT16, buf, fends)
    else:
        buf = to_dev(stream, dev)
        got, pm = spec_amd.decode_flat_present(FLAT16, buf, to_dev(ends.view(np.int64), dev))
    assert not got.status.cpu().numpy().any()
    out, out_ends = spec_amd.encode_flat_present(FLAT16, got.cols, {13: buf, 14: buf}, pm.contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), stream)
    assert np.array_equal(out_ends.cpu().numpy().view(np.uint64), ends)
    # the same batch sent as frames, and opened again where they lie
    fr, fr_ends = spec_amd.encode_flat_present(FLAT16, got.cols, {13: buf, 14: buf}, pm.contiguous(), frames=True)
    again, pm2 = spec_amd.decode_frames_present(FLAT16, fr, fr_ends)
    torch.cuda.synchronize()
    assert np.array_equal(fr.cpu().numpy(), spec_amd.make_frames(stream, ends))
    assert np.array_equal(pm2.cpu().numpy(), pm.cpu().numpy()) and not again.status.cpu().numpy().any()
    assert np.array_equal(pm.cpu().numpy().view(np.uint64), pack_mask(bits)[0])

"""spec_frames_write on the GPU: the frames equal spec_amd.make_frames byte for byte, frame_ends
equal the reader's walk (oracle frames_read), nothing outside the output is touched (64 canary
bytes on both sides), and Flat16 frames decode in place through decode_frames exactly as the
oracle decodes the records.  Record counts around a group of 64, record sizes that put several
heads into one 16-byte granule (empty and 1-byte records), a record far over the slab between
small ones, group spans around the slab's 18 KiB, and stream / output views at odd byte offsets
of aligned allocations."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, Kind, workload
from tests.gpu_helpers import oracle_encode, to_dev

pytestmark = pytest.mark.gpu

CANARY, PAD = 0xC3, 64
NS = (0, 1, 63, 64, 65, 129, 1000)
OFFSETS = ((0, 0), (1, 3), (3, 8), (8, 15), (15, 1))  # (stream, output) byte offsets


def _records(sizes, seed):
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.uint64)
    return rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8), np.cumsum(sizes, dtype=np.uint64)


def _span_group(span):
    """three groups of 64 records; the middle one spans exactly `span` bytes"""
    mid = [span // 64] * 63 + [span - 63 * (span // 64)]
    return [40] * 64 + mid + [33] * 64


@functools.lru_cache(maxsize=None)
def flat16(n):
    cols, heaps = workload.flat16(n, seed=300 + n)
    stream, ends = oracle_encode(FLAT16, cols, heaps, n)
    want_cols, want_status = O.decode_flat_batch(FLAT16.tags, FLAT16.kinds, stream, ends, FLAT16.widths)
    for a in (stream, ends, want_status, *want_cols):
        a.setflags(write=False)
    return stream, ends, want_cols, want_status


@functools.lru_cache(maxsize=None)
def shaped(kind):
    rng = np.random.default_rng(11)
    K = 1024
    sizes = {
        "empty": [0] * 129,
        "one": [1] * 129,
        "small": rng.integers(0, 41, 1000),
        # records over 1 KiB (copied wave-wide) among small ones, in a group that fits its slab
        "mid": [20] * 30 + [1024, 1025, 0, 3000] + [7] * 20 + [5000] + [20] * 60,
        "big": [int(x) for x in rng.integers(0, 41, 70)] + [40 * K] + [int(x) for x in rng.integers(0, 41, 129)],
        **{f"span{k}{d:+d}": _span_group(k * K + d) for k in (17, 18) for d in (-1, 0, 1)},
    }[kind]
    stream, ends = _records(sizes, 7)
    want = spec_amd.make_frames(stream, ends)
    for a in (stream, ends, want):
        a.setflags(write=False)
    return stream, ends, want


def run(dev, stream, ends, want, so, oo):
    n, total = len(ends), stream.size + 4 * len(ends)
    sbuf = torch.zeros(stream.size + 32, dtype=torch.uint8, device=dev)
    d_stream = sbuf[so:so + stream.size]
    if stream.size:
        d_stream.copy_(torch.from_numpy(np.array(stream)))
    d_ends = to_dev(np.array(ends).view(np.int64), dev)
    obuf = torch.full((2 * PAD + total + 32,), CANARY, dtype=torch.uint8, device=dev)
    out = obuf[PAD + oo:PAD + oo + total]
    assert sbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    frames, fends = spec_amd.write_frames(d_stream, d_ends, out=out)
    torch.cuda.synchronize()
    assert frames.data_ptr() == out.data_ptr() and frames.numel() == total
    host = obuf.cpu().numpy()
    assert (host[:PAD + oo] == CANARY).all() and (host[PAD + oo + total:] == CANARY).all(), "wrote outside the output"
    got = host[PAD + oo:PAD + oo + total]
    if not np.array_equal(got, want):
        j = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"byte {j} of {total}: gpu={got[j]:#x} want={want[j]:#x} (offsets {so}, {oo})")
    want_ends, used = O.frames_read(want, max(n, 1))
    assert used == total and np.array_equal(fends.cpu().numpy().view(np.uint64), want_ends)
    return frames, fends


@pytest.mark.parametrize("n", NS)
def test_flat16_counts_decode_in_place(dev, n):
    """Flat16 records: the frames, their ends, and the in-place decode of what was written."""
    stream, ends, want_cols, want_status = flat16(n)
    want = spec_amd.make_frames(stream, ends)
    for so, oo in ((0, 0), (3, 8)):
        frames, fends = run(dev, stream, ends, want, so, oo)
    if n == 0:
        return
    got = spec_amd.decode_frames(FLAT16, frames, fends)
    torch.cuda.synchronize()
    assert np.array_equal(got.status.cpu().numpy(), want_status)
    head = 4 * (np.arange(n, dtype=np.uint32) + 1)
    for f in range(len(FLAT16)):
        w = np.array(want_cols[f])
        if FLAT16.kinds[f] in (Kind.STRING, Kind.BYTES):  # spans point into the framed buffer
            sp = w.view(np.uint32).reshape(n, 2).copy()
            sp[:, 0] += np.where(sp[:, 1] > 0, head, 0).astype(np.uint32)
            w = sp.view(np.uint8).reshape(n, 8)
        assert np.array_equal(got.cols[f].cpu().numpy(), w), f


@pytest.mark.parametrize("kind", ["empty", "one", "small", "mid", "big"] +
                         [f"span{k}{d:+d}" for k in (17, 18) for d in (-1, 0, 1)])
def test_record_shapes(dev, kind):
    stream, ends, want = shaped(kind)
    for so, oo in (OFFSETS if kind in ("small", "one", "empty") else ((0, 0), (15, 1))):
        run(dev, stream, ends, want, so, oo)


def test_flat16_every_offset(dev):
    stream, ends, _, _ = flat16(1000)
    want = spec_amd.make_frames(stream, ends)
    for so, oo in OFFSETS[1:]:
        run(dev, stream, ends, want, so, oo)


def test_frame_ends_optional_and_capacity(dev):
    """frame_ends == NULL writes the same frames; a short frames_cap is SPEC_E_CAPACITY."""
    import ctypes as C

    stream, ends, want = shaped("small")
    L = spec_amd.lib()
    d_stream, d_ends = to_dev(np.array(stream), dev), to_dev(np.array(ends).view(np.int64), dev)
    out = torch.full((want.size + 16,), CANARY, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.spec_frames_write(p(d_stream), stream.size, p(d_ends), len(ends), p(out), want.size - 1, None, None) == -4
    assert L.spec_frames_write(p(d_stream), stream.size, p(d_ends), len(ends), p(out), want.size, None, None) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.array_equal(host[:want.size], want) and (host[want.size:] == CANARY).all()

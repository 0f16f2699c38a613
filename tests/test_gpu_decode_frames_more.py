"""The flat decoder's field error masks over mpx frames (spec_decode_frames_errors) against the
oracle's *Err getters on the unframed records, and the host pipeline over frames
(spec_host_decoder_run_frames) against the same pipeline over the unframed batch."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, Kind, Schema, SpecError, workload
from tests.gpu_helpers import concat_records, oracle_encode, to_dev
from tests.test_gpu_flat import ALL_KINDS, _extreme_values, write_record

pytestmark = pytest.mark.gpu

SPAN_KINDS = (Kind.STRING, Kind.BYTES)
CANARY = 0xA5


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


def framed(stream, ends):
    ends = np.ascontiguousarray(ends, dtype=np.uint64).view(np.int64)
    return spec_amd.make_frames(np.ascontiguousarray(stream, dtype=np.uint8), ends), \
        ends + 4 * (np.arange(len(ends), dtype=np.int64) + 1)


def shifted(want, kind, n0=0):
    """The oracle's column of the unframed records as the framed decode gives it: a non-empty
    span 4(k + 1) further on, an empty one at 0 (as spec_decode_frames)."""
    w = want.copy()
    if kind in SPAN_KINDS:
        wv = w.view(np.uint32)
        k = n0 + np.arange(len(w), dtype=np.uint32)
        wv[:, 0] = np.where(wv[:, 1] > 0, wv[:, 0] + 4 * (k + 1), 0)
    return w


# ---- 1. decode_frames_errors ----------------------------------------------------------------------------

WIDE_READ = Schema([(t + 1, ALL_KINDS[(t + 3) % len(ALL_KINDS)]) for t in range(70)])  # two mask words


@functools.lru_cache(maxsize=None)
def malformed(which, n):
    """The malformed-field records of tests/test_gpu_errors.py, n of them, with the oracle's decode:
    "flat16": natural-type records whose decoders still err (float32 +-Inf, bytes corrupted just
    below the table: test_fast_path_errors); "wide": 70 fields of extreme values written as one kind
    and read as another (test_cross_kind_errors)."""
    if which == "flat16":
        schema = FLAT16
        cols, heaps = workload.flat16(n, seed=8)
        f32 = cols[8].view(np.uint32).reshape(-1).copy()
        f32[::7] = 0x7F800000
        f32[3::11] = 0xFF800000
        cols[8] = f32.view(np.uint8).reshape(n, 4)
        stream, ends = oracle_encode(FLAT16, cols, heaps, n)
        stream = stream.copy()
        rng = np.random.default_rng(3)
        for i in rng.integers(0, n, max(1, n // 20)):
            stream[int(ends[i]) - 52 - int(rng.integers(0, 6))] ^= 0x80
    else:
        schema = WIDE_READ
        rng = np.random.default_rng(5)
        m = 48
        per_kind = {k: _extreme_values(k, rng, m) for k in ALL_KINDS}
        base = [write_record([(t + 1, ALL_KINDS[t % len(ALL_KINDS)], per_kind[ALL_KINDS[t % len(ALL_KINDS)]][i])
                              for t in range(70)]) for i in range(m)]
        stream, ends = concat_records([base[i % m] for i in range(n)])
    cols, status = O.decode_flat_batch(schema.tags, schema.kinds, stream, ends, schema.widths, nthreads=4)
    mask = np.atleast_2d(O.decode_flat_errors(schema.tags, schema.kinds, stream, ends))
    assert mask.any()
    frames, fends = framed(stream, ends)
    return schema, frames, fends, cols, status, mask


@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("which", ["flat16", "wide"])
def test_decode_frames_errors(dev, kernel, which, n):
    schema, frames, fends, wcols, wstatus, wmask = malformed(which, n)
    got, mask = spec_amd.decode_frames_errors(schema, to_dev(frames, dev), to_dev(fends, dev))
    torch.cuda.synchronize()
    assert np.array_equal(got.status.cpu().numpy(), wstatus)
    for f, fld in enumerate(schema.fields):
        assert np.array_equal(got.cols[f].cpu().numpy(), shifted(wcols[f], fld.kind)), fld
    gm = np.atleast_2d(mask.cpu().numpy().view(np.uint64))
    assert gm.shape == wmask.shape and np.array_equal(gm, wmask)


@pytest.mark.parametrize("which", ["flat16", "wide"])
def test_decode_frames_errors_sub_range(dev, kernel, which):
    """Records [3, 70) of 1,000: their rows and mask words (word c of record i at errmask[c * r1 + i])
    as the whole decode's; nothing outside the range is written."""
    schema, frames, fends, wcols, wstatus, wmask = malformed(which, 1000)
    n, r0, r1 = 1000, 3, 70
    cols = [torch.full((n, w), CANARY, dtype=torch.uint8, device=dev) for w in schema.widths]
    status = torch.full((n,), CANARY, dtype=torch.uint8, device=dev)
    words = wmask.shape[0]
    em = torch.full((words * r1 + 8,), -3, dtype=torch.int64, device=dev)
    got, mask = spec_amd.decode_frames_errors(schema, to_dev(frames, dev), to_dev(fends, dev), r0, r1, cols=cols,
                                              status=status, errmask=em[: words * r1])
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert np.array_equal(st[r0:r1], wstatus[r0:r1]) and (st[:r0] == CANARY).all() and (st[r1:] == CANARY).all()
    for f, fld in enumerate(schema.fields):
        g = cols[f].cpu().numpy()
        assert np.array_equal(g[r0:r1], shifted(wcols[f][r0:r1], fld.kind, r0)), fld
        assert (g[:r0] == CANARY).all() and (g[r1:] == CANARY).all(), fld
    e = em.cpu().numpy()
    assert (e[words * r1:] == -3).all()
    e = e[: words * r1].reshape(words, r1)
    assert np.array_equal(e[:, r0:].view(np.uint64), wmask[:, r0:r1]) and (e[:, :r0] == -3).all()


# ---- 2. HostDecoder.run_frames ----------------------------------------------------------------------------

def test_host_decoder_run_frames(dev):
    n = 1000
    cols, heaps = workload.flat16(n, seed=21)
    stream, ends = oracle_encode(FLAT16, cols, heaps, n)
    frames, fends = framed(stream, ends)
    h_stream, h_ends = torch.from_numpy(stream).pin_memory(), torch.from_numpy(ends.view(np.int64)).pin_memory()
    h_frames, h_fends = torch.from_numpy(frames).pin_memory(), torch.from_numpy(fends).pin_memory()
    want, wst = O.decode_flat_batch(FLAT16.tags, FLAT16.kinds, stream, ends, FLAT16.widths, nthreads=4)
    for chunks in (1, 3, 8):
        hd = spec_amd.HostDecoder(FLAT16, n, frames.size, dev, chunks=chunks)
        plain = hd.decode(h_stream, h_ends).clone()
        pcols, pst = [[c.clone() for c in x] if isinstance(x, list) else x.clone() for x in hd.columns()]
        out = hd.run_frames(h_frames, h_fends)
        assert out.numel() == plain.numel()  # the same chunk-major layout
        fcols, fst = hd.columns()
        assert np.array_equal(fst.numpy(), pst.numpy()) and np.array_equal(fst.numpy(), wst), chunks
        for f, fld in enumerate(FLAT16.fields):
            assert np.array_equal(pcols[f].numpy(), want[f]), (chunks, fld)
            assert np.array_equal(fcols[f].numpy(), shifted(want[f], fld.kind)), (chunks, fld)
        # frame ends that pass frames_len: refused, nothing launched, the output untouched
        hd.h_out.fill_(CANARY)
        bad = h_fends.clone()
        bad[n - 1] = frames.size + 1
        with pytest.raises(SpecError) as ei:
            hd.run_frames(h_frames, bad.pin_memory())
        assert ei.value.rc == -1  # SPEC_E_INVALID_ARGUMENT
        assert bool((hd.h_out == CANARY).all())
    # n == 0: a no-op
    hd0 = spec_amd.HostDecoder(FLAT16, 0, 64, dev, chunks=1)
    hd0.h_out.fill_(CANARY)
    hd0.run_frames(torch.zeros(0, dtype=torch.uint8).pin_memory(), torch.zeros(0, dtype=torch.int64).pin_memory())
    assert bool((hd0.h_out == CANARY).all())

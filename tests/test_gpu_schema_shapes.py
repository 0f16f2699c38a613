"""GPU parity over the shapes at which the schema-specialised flat kernels change their code
(workload.shape_sweep_schemas(); DESIGN.md §4 says what each shape is there for): the decode wave
pair's split, FAST_MAX_FIELDS, the words of present_ranks' tag set, SpecEnc's two table builders and
its last field count, its string/bytes emission around 16, 32, 64 and 80 bytes at every heap phase,
and jit.cpp's lookup ring.  Every test runs under the specialised and the generic kernels, bit-exact
against the oracle, and its "jit" leg first asserts that the specialised kernels are loaded and will
run on the batch at hand (require_specialised): a module that failed to compile, or a batch whose mean
record has no LDS slab, would otherwise run the generic kernel twice.  The Writer's records of 49
fields and more are over that mean, so their decode batches hold the empty message in every other
record (tests/shape_helpers.py fit_slab).
tests/test_schema_shapes.py checks on the CPU that the inputs are what these tests take them for."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import Kind
from tests.gpu_helpers import (check_decode, check_encode, check_errors, concat_records, oracle_encode,
                               require_specialised, slab_fits, to_dev)
from tests.present_helpers import PATTERNS, check_present, pack_mask, patterns, value_of
from tests.shape_helpers import (ENC_MAX_FIELDS, LENGTH_BATCHES, LENGTH_SCHEMAS, N_DECODE, N_ENCODE, SWEEP, decode_batch,
                                 fuzz_batch, handoff_batch, length_batch, sparse_batch, sweep_columns)
from tests.test_gpu_flat import write_record

pytestmark = pytest.mark.gpu

NAMES = list(SWEEP)


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    """Run a test with the schema-specialised kernels (hiprtc) and with the generic kernel."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


def prove(kernel, name, recs=None, encode=False):
    """The jit leg's proof, before the first launch: the specialised decode kernels will run on the
    batch `recs` (its mean record has an LDS slab), the specialised encoders are loaded.  A schema of
    more than ENC_MAX_FIELDS fields has no specialised encoder: its encode runs the run-time kernels
    under both legs, and prepare says so."""
    if kernel != "jit":
        return
    s = SWEEP[name]
    has_encoder = len(s) <= ENC_MAX_FIELDS
    require_specialised(s, name, decode=None if recs is None else (sum(len(r) for r in recs), len(recs)),
                        encode=encode and has_encoder)
    if encode and not has_encoder:
        assert spec_amd.lib().spec_encode_flat_prepare(C.byref(s.c)) == 0, name


# the records are built once for both legs
cached_decode_batch = functools.lru_cache(maxsize=None)(decode_batch)
cached_handoff_batch = functools.lru_cache(maxsize=None)(handoff_batch)
cached_fuzz_batch = functools.lru_cache(maxsize=None)(fuzz_batch)
sparse_records = functools.lru_cache(maxsize=None)(sparse_batch)


# ---- decode ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_decode_parity(dev, kernel, name):
    """Writer records: columns and status of the plain kernels, then the *Err kernels' masks too."""
    recs = cached_decode_batch(name)
    prove(kernel, name, recs)
    stream, ends = concat_records(recs)
    check_decode(dev, SWEEP[name], stream, ends, f"{name} {kernel}")
    check_errors(dev, SWEEP[name], stream, ends, f"{name} {kernel} errors")


@pytest.mark.parametrize("name", NAMES)
def test_mid_record_handoff(dev, kernel, name):
    """Record i's field i mod N written with another kind: the natural-type check gives the record
    up in another batch and another wave of the pair from record to record."""
    recs = cached_handoff_batch(name)
    prove(kernel, name, recs)
    stream, ends = concat_records(recs)
    check_decode(dev, SWEEP[name], stream, ends, f"{name} hand-off {kernel}")
    check_errors(dev, SWEEP[name], stream, ends, f"{name} hand-off {kernel} errors")


@pytest.mark.parametrize("name", NAMES)
def test_present_decode(dev, kernel, name):
    """Every mask pattern without and with the *Err masks: HasField masks (between canary rows),
    columns and status.  Over tagwords8 the half patterns hold tables with one of two tags that
    alias modulo 64 (63 | 127 | 191 | 255, 64 | 128 | 192) and not the other."""
    for p in PATTERNS:
        recs, bits = sparse_records(name, p)
        prove(kernel, name, recs)
        for errors in (False, True):
            want = check_present(dev, SWEEP[name], recs, f"{name} {p} errors={errors} {kernel}", errors=errors)
            assert np.array_equal(want, pack_mask(bits))  # a Writer's record has exactly the fields it wrote


# foreign tags: in a word the schema has tags in (2, 129), aliasing a schema tag modulo 64 from
# another such word (65 and 193 against 1; 129 against 1 too); for tags3w in the words it has none in
FOREIGN = {"tagwords8": (2, 129, 65, 193), "tags3w": (66, 130)}


@functools.lru_cache(maxsize=None)
def foreign_records(name, n=N_DECODE):
    s = SWEEP[name]
    cols, heaps = sweep_columns(name, n)
    bits = patterns(len(s), n)["half1"].copy()
    bits[::5] = True  # full tables too
    recs = []
    for i in range(n):
        fields = [(fld.tag, fld.kind, value_of(s, cols, heaps, f, i)) for f, fld in enumerate(s.fields) if bits[i, f]]
        if i % 3:  # (every third record stays the schema's own)
            fields.append((FOREIGN[name][i % len(FOREIGN[name])], Kind.INT32, i - 60))
        if i % 7 == 3:  # two foreign tags
            fields.append((FOREIGN[name][(i + 1) % len(FOREIGN[name])], Kind.BOOL, True))
        recs.append(write_record(fields))
    return recs, bits


@pytest.mark.parametrize("name", list(FOREIGN))
def test_present_foreign_tags(dev, kernel, name):
    recs, bits = foreign_records(name)
    prove(kernel, name, recs)
    for errors in (False, True):
        want = check_present(dev, SWEEP[name], recs, f"{name} foreign tags errors={errors} {kernel}", errors=errors)
        assert np.array_equal(want, pack_mask(bits))  # a foreign tag sets no bit


@pytest.mark.parametrize("name", NAMES)
def test_fuzz(dev, kernel, name):
    """Mutated, cut and garbage records (the recipe of test_wide_fuzz) through the plain and the
    present kernels."""
    recs = cached_fuzz_batch(name)
    prove(kernel, name, recs)
    stream, ends = concat_records(recs)
    check_decode(dev, SWEEP[name], stream, ends, f"{name} fuzz {kernel}")
    check_present(dev, SWEEP[name], recs, f"{name} fuzz present {kernel}", errors=True)


# ---- encode ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_encode(dev, kernel, name):
    """Bytes and ends of the oracle Writer; the framed encoder's mpx frames of the same records; the
    device's own bytes decoded on the device."""
    prove(kernel, name, encode=True)
    s, n = SWEEP[name], N_ENCODE
    cols, heaps = sweep_columns(name, n)
    want_stream, want_ends = check_encode(dev, s, cols, heaps, n, f"{name} {kernel}")
    d_cols = [to_dev(c, dev) for c in cols]
    d_heaps = {f: to_dev(h if h.size else np.zeros(1, np.uint8), dev) for f, h in heaps.items()}
    frames, fends = spec_amd.encode_flat_frames(s, d_cols, d_heaps, n)
    torch.cuda.synchronize()
    assert np.array_equal(fends.cpu().numpy().view(np.uint64), want_ends + 4 * (np.arange(n, dtype=np.uint64) + 1)), name
    assert np.array_equal(frames.cpu().numpy(), spec_amd.make_frames(want_stream, want_ends)), name
    # (n full records of 49 fields and more have no LDS slab: this decode then launches the generic
    # kernel under both legs, prepare says so, and the specialised decode of these shapes is
    # test_decode_parity's, on a batch that fits)
    if kernel == "jit":
        rc = spec_amd.lib().spec_decode_flat_prepare(C.byref(s.c), want_stream.size, n)
        assert rc == (1 if slab_fits(want_stream.size, n) else 0), (name, rc)
    out, ends = spec_amd.encode_flat(s, d_cols, d_heaps, n)
    got = spec_amd.decode_flat(s, out, ends)
    torch.cuda.synchronize()
    want_cols, want_status = O.decode_flat_batch(s.tags, s.kinds, want_stream, want_ends, s.widths)
    assert np.array_equal(got.status.cpu().numpy(), want_status) and not want_status.any(), name
    for f in range(len(s)):
        assert np.array_equal(got.cols[f].cpu().numpy(), want_cols[f]), (name, f)


@pytest.mark.parametrize("batch", LENGTH_BATCHES)
@pytest.mark.parametrize("sname", list(LENGTH_SCHEMAS))
def test_encode_length_sweep(dev, kernel, sname, batch):
    """String/bytes lengths around the specialised encoder's emission boundaries at every heap phase,
    heaps packed to their last byte: a wave all on the short path, a wave with one lane off it, a wave
    with one big record (six-byte table entries, a group over the slab) among small ones."""
    s = LENGTH_SCHEMAS[sname]
    if kernel == "jit":
        require_specialised(s, sname, encode=True)
    cols, heaps = length_batch(s, batch)
    check_encode(dev, s, cols, heaps, N_ENCODE, f"{sname} lengths {batch} {kernel}")


# ---- jit.cpp lookup: a thread-local ring of 8 (device, program, schema) answers ---------------------

RING_NAMES = ["n1", "n2", "n8", "n9", "n17p", "n18", "tag255", "tag256", "tagwords8", "tags3w"]


def test_lookup_ring(dev):
    """Ten schemas' decode and encode in turn (twenty answers through a ring of eight), then the first
    again: its kernels are still its own — the results of its first run and the oracle's."""
    spec_amd.set_jit(True)
    n = N_DECODE

    def run(name):
        s = SWEEP[name]
        cols, heaps = sweep_columns(name, n)
        stream, ends = oracle_encode(s, cols, heaps, n)
        require_specialised(s, name, decode=(stream.size, n), encode=True)
        got, _, _ = check_decode(dev, s, stream, ends, f"ring {name}")
        check_encode(dev, s, cols, heaps, n, f"ring {name}")
        out, out_ends = spec_amd.encode_flat(s, [to_dev(c, dev) for c in cols],
                                             {f: to_dev(h if h.size else np.zeros(1, np.uint8), dev) for f, h in heaps.items()}, n)
        torch.cuda.synchronize()
        return [c.cpu().numpy() for c in got.cols] + [got.status.cpu().numpy(), out.cpu().numpy(), out_ends.cpu().numpy()]

    first = run(RING_NAMES[0])
    for name in RING_NAMES[1:]:
        run(name)
    again = run(RING_NAMES[0])
    assert len(first) == len(again) and all(np.array_equal(a, b) for a, b in zip(first, again))

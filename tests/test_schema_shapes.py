"""The shape sweep's conditions that need no GPU (tests/test_gpu_schema_shapes.py runs it): every
catalog schema has the specialised modules the sweep means to run (build() compiled them into the
code-object cache, so the calls here are cache reads), and the sweep's inputs are sound — the oracle
opens every record and gives the input columns back, so no GPU test passes over an all-error batch —
and the length sweep holds every boundary length at every heap phase."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import spec_amd
from oracle import oracle as O
from spec_amd.schema import VARLEN
from tests.gpu_helpers import concat_records, oracle_encode, slab_fits
from tests.present_helpers import PATTERNS
from tests.shape_helpers import (BIG_FIELD, EMPTY, ENC_MAX_FIELDS, LENGTH_BATCHES, LENGTH_SCHEMAS, LENGTHS, N_DECODE,
                                 N_ENCODE, SHORT, SWEEP, decode_batch, fuzz_batch, handoff_batch, handoff_records,
                                 length_batch, sparse_batch, sweep_columns, varlen_fields, writer_records)


def test_catalog_is_the_listed_shapes():
    counts = {name: len(s) for name, s in SWEEP.items()}
    assert [c for name, c in counts.items() if name[0] == "n" and name[1].isdigit()] == \
        [1, 2, 8, 9, 17, 18, 21, 22, 24, 25, 32, 33, 34, 49, 63, 64]
    assert {k: counts[k] for k in ("big21", "big22", "tag255", "tag256", "tagwords8", "tags3w", "heap16")} == \
        {"big21": 21, "big22": 22, "tag255": 2, "tag256": 2, "tagwords8": 8, "tags3w": 3, "heap16": 16}
    assert SWEEP["big21"].tags[:3] == [250, 253, 256] and SWEEP["tag255"].tags == [254, 255]
    assert SWEEP["tag256"].tags == [255, 256] and sorted(SWEEP["tags3w"].tags) == [1, 2, 200]
    assert sorted({t >> 6 for t in SWEEP["tagwords8"].tags}) == [0, 1, 2, 3]
    assert SWEEP["tagwords8"].tags != sorted(SWEEP["tagwords8"].tags)  # a permuted write order
    for name in ("n17p", "n21p", "n24p", "n34p", "n63p"):
        assert SWEEP[name].tags != sorted(SWEEP[name].tags) and sorted(SWEEP[name].tags) == list(range(1, counts[name] + 1))
    for name, s in SWEEP.items():
        if len(s) >= 3:  # every schema of three fields or more has string/bytes fields
            assert varlen_fields(s), name
    kinds = [f.kind for f in SWEEP["heap16"].fields]
    assert kinds.count(spec_amd.Kind.STRING) == 6 and kinds.count(spec_amd.Kind.BYTES) == 6


@pytest.mark.parametrize("name", list(SWEEP))
def test_specialised_modules_compile(name):
    L = spec_amd.lib()
    s = SWEEP[name]
    assert L.spec_decode_flat_jit_compile(C.byref(s.c), 1 << 28, 1 << 20) > 0, name
    enc = L.spec_encode_flat_jit_compile(C.byref(s.c))
    assert (enc > 0) == (len(s) <= ENC_MAX_FIELDS), (name, enc)


def assert_round_trip(schema, cols, heaps, n, label):
    """oracle encode -> oracle decode: every record opens and the input columns come back."""
    stream, ends = oracle_encode(schema, cols, heaps, n)
    got, status = O.decode_flat_batch(schema.tags, schema.kinds, stream, ends, schema.widths)
    assert not status.any(), f"{label}: record {int(np.nonzero(status)[0][0])} does not open"
    for f, fld in enumerate(schema.fields):
        if fld.kind not in VARLEN:
            assert np.array_equal(got[f], cols[f]), f"{label}: field {f}"
            continue
        g, w = got[f].view(np.uint32).reshape(n, 2), cols[f].view(np.uint32).reshape(n, 2)
        assert np.array_equal(g[:, 1], w[:, 1]), f"{label}: field {f} lengths"
        for i in range(n):
            assert np.array_equal(stream[g[i, 0]:g[i, 0] + g[i, 1]], heaps[f][w[i, 0]:w[i, 0] + w[i, 1]]), \
                f"{label}: field {f} record {i}"
    return stream, ends


@pytest.mark.parametrize("name", list(SWEEP))
def test_sweep_inputs_round_trip(name):
    for n in (N_DECODE, N_ENCODE):
        cols, heaps = sweep_columns(name, n)
        assert_round_trip(SWEEP[name], cols, heaps, n, f"{name} n={n}")


@pytest.mark.parametrize("name", list(SWEEP))
def test_handoff_records_open_and_err(name):
    """The hand-off batch: every record opens, and the field written with another kind is the only one
    a getter can reject (some kinds read each other, so not every record errs)."""
    s = SWEEP[name]
    stream, ends = concat_records(handoff_records(name))
    _, status = O.decode_flat_batch(s.tags, s.kinds, stream, ends, s.widths)
    assert not status.any(), name
    mask = O.decode_flat_errors(s.tags, s.kinds, stream, ends).reshape(-1, N_DECODE)[0]
    odd = np.uint64(1) << (np.arange(N_DECODE, dtype=np.uint64) % np.uint64(len(s)))
    assert not (mask & ~odd).any(), name
    assert np.count_nonzero(mask) >= N_DECODE // 4, (name, np.count_nonzero(mask))


def test_slab_limit_arithmetic():
    """tests/gpu_helpers.py slab_fits restates decode_core.hpp decode_slab_bytes: 64 records * 1.04 in
    at most SLAB_MAX_CHUNKS = 40 chunks of 1 KiB, so a mean record of 615 bytes fits and 616 does not."""
    import re

    src = open(os.path.join(os.path.dirname(spec_amd.__file__), "csrc", "decode_core.hpp")).read()
    assert re.search(r"constexpr int SLAB_MAX_CHUNKS = 40;", src)
    assert re.search(r"decode_slab_bytes\(double avg_record, double margin = 1\.04\)", src)
    assert slab_fits(615 * 100, 100) and not slab_fits(616 * 100, 100) and not slab_fits(0, 0)


@pytest.mark.parametrize("name", list(SWEEP))
def test_decode_batches_fit_the_slab(name):
    """Every batch the GPU tests decode under a jit proof launches the specialised kernels (its mean
    record has an LDS slab), and the thinning that makes the 49..64-field batches fit leaves full
    Writer tables in every 64-record group: the kernels' fast paths still meet them."""
    s = SWEEP[name]
    full = writer_records(name, N_DECODE)
    thinned = not slab_fits(sum(len(r) for r in full), N_DECODE)
    assert thinned == (name in ("n49", "n63p", "n64")), name
    batches = {"parity": decode_batch(name), "hand-off": handoff_batch(name), "fuzz": fuzz_batch(name)}
    batches.update({p: sparse_batch(name, p)[0] for p in PATTERNS})
    for what, recs in batches.items():
        assert slab_fits(sum(len(r) for r in recs), len(recs)), (name, what)
    for what in ("parity", "hand-off", "all"):
        recs = batches[what]
        stream, ends = concat_records(recs)
        _, status = O.decode_flat_batch(s.tags, s.kinds, stream, ends, s.widths)
        assert not status.any(), (name, what)
        kept = np.array([r != EMPTY for r in recs])
        for g in range(0, len(recs), 64):
            assert kept[g:g + 64].sum() >= (len(kept[g:g + 64]) + 1) // 2, (name, what, g)
        if thinned:  # both lane parities, so the hand-off meets odd and even fields of an even field count
            assert kept[:64:2].all() and kept[65:128:2].all() and not kept[1:64:2].any()


@pytest.mark.parametrize("batch", LENGTH_BATCHES)
@pytest.mark.parametrize("sname", list(LENGTH_SCHEMAS))
def test_length_batches(sname, batch):
    schema = LENGTH_SCHEMAS[sname]
    n = N_ENCODE
    cols, heaps = length_batch(schema, batch, n)
    stream, ends = assert_round_trip(schema, cols, heaps, n, f"{sname} {batch}")
    vf = varlen_fields(schema)
    spans = {f: cols[f].view(np.uint32).reshape(n, 2) for f in vf}
    for f in vf:  # packed back to back from 0; the last span ends at the heap's end
        off, ln = spans[f][:, 0].astype(np.int64), spans[f][:, 1].astype(np.int64)
        assert off[0] == 0 and np.array_equal(off[1:], (off + ln)[:-1]) and off[-1] + ln[-1] == heaps[f].size
    lens = np.stack([spans[f][:, 1] for f in vf], axis=1).astype(np.int64)
    waves = [slice(w, min(w + 64, n)) for w in range(0, n, 64)]
    if batch == "sweep":  # every boundary length at every phase of off & 3
        seen = {(int(ln), int(off) & 3) for f in vf for off, ln in spans[f]}
        missing = [(x, p) for x in LENGTHS for p in range(4) if (x, p) not in seen]
        assert not missing, missing
    elif batch == "short":  # the only batch on put_heap_short<5>: each of its lengths at every phase too
        assert lens.max() <= 16 and lens.max() == 16
        seen = {(int(ln), int(off) & 3) for f in vf for off, ln in spans[f]}
        missing = [(x, p) for x in SHORT for p in range(4) if (x, p) not in seen]
        assert not missing, missing
    elif batch == "one_long":
        assert sorted(int(lens[w].max()) for w in waves) == [17, 33, 64, 65, 129]
        assert all(np.count_nonzero(lens[w] > 16) == 1 for w in waves)
    else:
        size = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
        assert all(np.count_nonzero(size[w] > 65535) == 1 for w in waves)
        assert all(np.count_nonzero(lens[w] == BIG_FIELD) == 1 for w in waves)
        assert np.sort(size)[-len(waves) - 1] < 8192  # the others are small records

"""Inputs of the schema-shape sweep (tests/test_gpu_schema_shapes.py on the GPU; their conditions
checked on the CPU by tests/test_schema_shapes.py): the catalog of workload.shape_sweep_schemas(),
Writer records whose one field has another kind, mutated records, and string/bytes batches whose
lengths walk the specialised encoder's emission boundaries at every heap phase."""
from __future__ import annotations

import numpy as np

from spec_amd import FLAT16, Kind, Schema, workload
from spec_amd.schema import VARLEN
from tests.gpu_helpers import oracle_encode, slab_fits
from tests.present_helpers import patterns, value_of, write_sparse
from tests.test_gpu_flat import ALL_KINDS, write_record

SWEEP = workload.shape_sweep_schemas()
ENC_MAX_FIELDS = 32  # jit.cpp: the last field count with a specialised encoder
N_DECODE = 130  # two full 64-record groups and a two-record tail
N_ENCODE = 300  # crosses the 256-record encode block: four full waves and one of 44 records


def seed_of(name: str) -> int:
    return sum(name.encode())


def sweep_columns(name: str, n: int):
    return workload.gen_columns(SWEEP[name], n, seed=seed_of(name) + n, str_len=(0, 40))


def split_records(stream, ends):
    return [bytes(stream[(int(ends[i - 1]) if i else 0):int(ends[i])]) for i in range(len(ends))]


def writer_records(name: str, n: int):
    """The oracle Writer's records of sweep_columns(name, n) -> [bytes]"""
    cols, heaps = sweep_columns(name, n)
    return split_records(*oracle_encode(SWEEP[name], cols, heaps, n))


EMPTY = bytes([0, 0, 80])  # the Writer's message without a field


def fit_slab(recs, bits=None):
    """A decode batch that launches the specialised kernels: they parse a 64-record group from an LDS
    slab sized from the batch's mean record, and a batch whose mean is over the largest slab (about
    615 bytes: the Writer's records of 49 fields and more) launches the generic kernel whatever the
    schema.  Such a batch keeps every other record (the even lanes of even groups, the odd lanes of odd
    ones) and holds the empty message in between; any other batch stays as it is.  -> (recs, bits)"""
    if slab_fits(sum(len(r) for r in recs), len(recs)):
        return recs, bits
    keep = np.array([(i + i // 64) % 2 == 0 for i in range(len(recs))])
    recs = [r if k else EMPTY for r, k in zip(recs, keep)]
    if bits is not None:
        bits = bits & keep[:, None]
    assert slab_fits(sum(len(r) for r in recs), len(recs))
    return recs, bits


def decode_batch(name: str):
    return fit_slab(writer_records(name, N_DECODE))[0]


def handoff_batch(name: str):
    return fit_slab(handoff_records(name))[0]


def fuzz_batch(name: str):
    return fuzz_records(fit_slab(writer_records(name, N_ENCODE))[0], 700 + seed_of(name))


def sparse_batch(name: str, pattern: str, n: int = N_DECODE):
    """The oracle Writer's sparse records of a mask pattern of tests/present_helpers.py -> (recs, bits)"""
    s = SWEEP[name]
    cols, heaps = sweep_columns(name, n)
    bits = patterns(len(s), n)[pattern]
    return fit_slab(write_sparse(s, cols, heaps, bits, n), bits)


HANDOFF_SHIFTS = (1, 3, 7)


def handoff_records(name: str, n: int = N_DECODE):
    """Record i holds field i mod N written with the kind `shift` places further on (1, 3 and 7 in
    turn), every other field with its own: the specialised kernels' natural-type check hands the
    record to the generic path from a batch and a wave of the pair that move from record to record."""
    schema = SWEEP[name]
    nf = len(schema)
    cols, heaps = sweep_columns(name, n)
    alts = {}
    for sh in HANDOFF_SHIFTS:
        alt = Schema([(f.tag, ALL_KINDS[(ALL_KINDS.index(f.kind) + sh) % len(ALL_KINDS)]) for f in schema.fields])
        alts[sh] = (alt, *workload.gen_columns(alt, n, seed=seed_of(name) + sh, str_len=(0, 40)))
    recs = []
    for i in range(n):
        alt, acols, aheaps = alts[HANDOFF_SHIFTS[(i + i // nf) % 3]]
        recs.append(write_record([
            (fld.tag, alt.fields[f].kind, value_of(alt, acols, aheaps, f, i)) if f == i % nf else
            (fld.tag, fld.kind, value_of(schema, cols, heaps, f, i)) for f, fld in enumerate(schema.fields)]))
    return recs


def fuzz_records(recs, seed: int):
    """The mutation recipe of tests/test_gpu_wide.py test_wide_fuzz: byte mutations anywhere, in the
    table / trailer region, a cut, a garbage record, or the record as it is."""
    rng = np.random.default_rng(seed)
    out = []
    for r in recs:
        b = bytearray(r)
        x = rng.integers(0, 5)
        if x == 0:
            for _ in range(rng.integers(1, 4)):
                b[rng.integers(0, len(b))] = rng.integers(0, 256)
        elif x == 1:
            b[len(b) - 1 - rng.integers(0, min(len(b), 120))] = rng.integers(0, 256)
        elif x == 2:
            b = b[:rng.integers(0, len(b))]
        elif x == 3:
            b = bytearray(rng.integers(0, 256, rng.integers(0, 300), dtype=np.uint8).tobytes())
        out.append(bytes(b))
    return out


# ---- the length sweep of the specialised encoder's string/bytes emission (encode_core.hpp SpecEnc) ----
# around 16 (put_heap_short<5> | put_heap64), 32 (the second heap prefetch: (off & 3) + len > 32), 64
# (the prefetched part's end) and 80 (Rec::h), then lengths no flat specialised-encoder test wrote
LENGTHS = [0, 1, 3, 4, 5, *range(12, 21), *range(28, 37), *range(60, 69), *range(76, 85), 127, 128, 129, 255, 256,
           257]
SHORT = [x for x in LENGTHS if x <= 16]
LENGTH_SCHEMAS = {"heap16": SWEEP["heap16"], "flat16": FLAT16}
LENGTH_BATCHES = ("sweep", "short", "one_long", "one_big")
BIG_FIELD = 66000  # one field of more than 65535 bytes: a big record (six-byte table entries)


def varlen_fields(schema):
    return [f for f, fld in enumerate(schema.fields) if fld.kind in VARLEN]


def special_lane(wave: int, step: int) -> int:
    """The lane of wave `wave` that differs from the rest (inside the last wave of N_ENCODE, 44 records)."""
    return (5 + step * wave) % 44


def length_of(schema, batch: str):
    """(record, field) -> the span's length in batch `batch`"""
    vf = varlen_fields(schema)

    def sweep(i, f):
        return LENGTHS[(i + 3 * f) % len(LENGTHS)]

    def short(i, f):
        return SHORT[(i + 3 * f) % len(SHORT)]

    def one_long(i, f):  # exactly one lane of every wave holds one span over 16 bytes
        w = i // 64
        if i % 64 == special_lane(w, 13) and f == vf[w % len(vf)]:
            return (17, 33, 64, 65, 129)[w % 5]
        return short(i, f)

    def one_big(i, f):  # exactly one record of every wave holds more than 65535 bytes of data
        w = i // 64
        if i % 64 == special_lane(w, 17) and f == vf[(w + 1) % len(vf)]:
            return BIG_FIELD
        return sweep(i, f)

    return {"sweep": sweep, "short": short, "one_long": one_long, "one_big": one_big}[batch]


def length_batch(schema, batch: str, n: int = N_ENCODE):
    """Columns and heaps of n records whose string/bytes lengths follow length_of(schema, batch), every
    heap packed back to back from offset 0: off & 3 takes every phase and the last span ends at the
    heap's end."""
    cols, _ = workload.gen_columns(schema, n, seed=41 + len(batch), str_len=(0, 0))
    rng = np.random.default_rng(43 + len(batch))
    fn = length_of(schema, batch)
    heaps = {}
    for f in varlen_fields(schema):
        lens = np.array([fn(i, f) for i in range(n)], np.uint32)
        span = np.zeros((n, 2), np.uint32)
        span[1:, 0] = np.cumsum(lens[:-1], dtype=np.uint64).astype(np.uint32)
        span[:, 1] = lens
        lo, hi = (32, 127) if schema.fields[f].kind == Kind.STRING else (0, 256)
        heaps[f] = rng.integers(lo, hi, size=int(lens.sum(dtype=np.uint64)), dtype=np.uint8)
        cols[f] = workload.as_bytes(span, n)
    return cols, heaps

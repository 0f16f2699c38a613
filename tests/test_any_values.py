"""The catalog of tests/any_values.py against the oracle (CPU): the GPU tests over it
(tests/test_gpu_any_values.py) reach what they claim to reach — every branch of DecodeTypeSize's
switch with a well-formed value, every malformed case with an error, every varint length."""
from __future__ import annotations

import struct

import numpy as np

from oracle import oracle as O
from spec_amd.schema import Kind
from tests import any_values as A


def test_classes_are_the_oracles():
    """Every entry's declared class is what the oracle's OpenValue makes of its bytes filling the
    slot; an ok entry's decoded size is all of its bytes."""
    for e in A.catalog():
        cls, off, size = A.open_value(e.data)
        assert cls == e.cls, e.name
        if cls == "ok":
            t, n, err = O.decode("type_size", e.data)
            assert err is None and n == len(e.data) and t == e.data[-1], e.name
            assert (off, size) == (0, len(e.data)), e.name
    names = [e.name for e in A.catalog()]
    assert len(set(names)) == len(names)


def test_every_switch_branch_and_malformed_case_occurs():
    ok = {e.data[-1] for e in A.catalog() if e.cls == "ok"}
    err = {e.data[-1] for e in A.catalog() if e.cls == "err"}
    assert ok == set(A.SWITCH_TYPES)
    assert set(A.MALFORMED_TYPES) <= err
    classes = [e.cls for e in A.catalog()]
    assert classes.count("nil") >= 1 and classes.count("panic") >= 1
    # the malformed cases by what the oracle says of each
    text = {e.name: O.decode("type_size", e.data)[2] for e in A.catalog() if e.cls == "err"}
    assert text["bad_type_99"] == text["bad_type_0"] == "decode: invalid type"
    assert text["bad_int32_varint_to_slot_start"] == text["bad_int64_eleven_byte_varint"] == "decode int: invalid data"
    assert text["bad_uint32_varint_to_slot_start"] == text["bad_uint64_eleven_byte_varint"] == "decode uint: invalid data"
    assert text["bad_float32_3_bytes"] == "decode float32: invalid data"
    assert text["bad_bin256_31_bytes"] == "decode bin256: invalid data"
    assert text["bad_string_size_over_slot"] == text["bad_string_no_room_for_nul"] == "decode string: invalid data"
    assert text["bad_bytes_size_varint"] == "decode bytes: invalid data size"
    assert text["bad_list_table_over_slot"] == "decode list: invalid data"
    assert text["bad_list_data_size_varint"] == "decode list: invalid data size"
    assert text["bad_struct_past_slot"] == "decode struct: invalid data"
    # the struct's malformed size varint is no error (type.go:190 checks n, not m): n < 0
    assert O.decode("type_size", dict((e.name, e.data) for e in A.catalog())["panic_struct_size_varint"])[1:] == (-1, None)
    assert O.decode("type_size", bytes([A.T_STRUCT]))[1:] == (0, None)


def test_junk_placements_keep_class_and_span():
    """Behind 1, 3 and 7 junk bytes in the same slot an entry has the class it has alone and, where
    it is a value, a span of exactly its own bytes.  The exceptions are the entries whose class is a
    property of the slot's start (A.SLOT_BOUND): a fixed-size value one byte short becomes whole, and
    the struct type byte that opened with no bytes reads the junk as its size varint."""
    cat = A.catalog()
    seen = set()
    for p in A.placements():
        e = cat[p.entry]
        assert p.slot == A.JUNK[:p.junk] + e.data and (p.cls, p.off, p.size) == A.open_value(p.slot)
        seen.add((p.entry, p.junk))
        if p.junk == 0 or e.name not in A.SLOT_BOUND:
            assert p.cls == e.cls, (e.name, p.junk)
            assert (p.off, p.size) == ((p.junk, len(e.data)) if e.cls == "ok" else (0, 0)), (e.name, p.junk)
        else:
            assert p.cls == ("panic" if e.cls == "nil" else "ok"), (e.name, p.junk)
    assert seen == {(i, k) for i in range(len(cat)) for k in A.JUNK_LENS}
    assert all(b >= 0x80 and b not in A.SWITCH_TYPES for b in A.JUNK)
    assert {e.name for e in cat if e.name in A.SLOT_BOUND} == set(A.SLOT_BOUND)


def test_every_varint_length_occurs():
    """Integer values of every reverse-varint length the kind can have (1..3, 1..5, 1..10), on both
    sides of every length step; string and bytes with size varints of 1, 2 and 3 bytes."""
    data = {e.name: e.data for e in A.catalog()}
    sc = A.scalars()
    for kind, bits in A.INT_BITS.items():
        k = Kind[kind.upper()]
        lens = {}
        for name, (kk, v) in sc.items():
            if kk == k:
                lens.setdefault(len(data[name]) - 1, []).append(v)
        assert sorted(lens) == list(range(1, A.VARINT_MAX[bits] + 1)), kind
        for ln in range(1, A.VARINT_MAX[bits]):  # the step from ln to ln + 1 bytes: adjacent values
            if kind.startswith("u"):
                assert max(lens[ln]) + 1 == min(lens[ln + 1]), (kind, ln)
            else:
                assert max(lens[ln]) + 1 == min(v for v in lens[ln + 1] if v > 0), (kind, ln)
                assert min(lens[ln]) - 1 == max(v for v in lens[ln + 1] if v < 0), (kind, ln)
        lo, hi = (0, 2 ** bits - 1) if kind.startswith("u") else (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1)
        assert {lo, 1, hi} <= {v for vs in lens.values() for v in vs}
    for kind, nul in (("string", 1), ("bytes", 0)):
        sizes = {len(data[f"{kind}_{ln}"]) - 1 - nul - ln for ln in A.PAYLOAD_LENS}
        assert sizes == {1, 2, 3}, kind


def test_scalar_entries_decode_to_their_values():
    """The oracle's Decode<Kind> of every ok scalar entry returns the Python value it was built from
    (floats by bit pattern: the encoder kept the NaN's payload and the zeros' signs); float32 +-Inf
    is Float32()'s range error and Float64()'s infinity."""
    data = {e.name: e.data for e in A.catalog()}
    for name, (k, v) in A.scalars().items():
        got, n, err = O.decode(k.name.lower(), data[name])
        if name in A.OWN_READER_ERRS:
            assert err.startswith("decode float32: overflow") and (got, n) == (0.0, 0), name
            got, n, err = O.decode("float64", data[name])
            assert err is None and n == len(data[name]) and got == float(name.replace("float32_pos_", "").replace("float32_neg_", "-")), name
            continue
        assert err is None and n == len(data[name]), name
        if k == Kind.FLOAT32:
            got = struct.unpack("<I", struct.pack("<f", got))[0]
        elif k == Kind.FLOAT64:
            got = struct.unpack("<Q", struct.pack("<d", got))[0]
        elif k == Kind.STRING:
            got = got.encode("latin-1")
        assert got == v, name
    # the catalog's containers are what ParseValue accepts
    cat = [e for e in A.catalog() if e.cls == "ok" and e.name not in ("int16_four_byte_varint",) + A.OWN_READER_ERRS]
    stream = np.frombuffer(b"".join(e.data for e in cat), np.uint8)
    ends = np.cumsum([len(e.data) for e in cat]).astype(np.uint64)
    st, sz = O.parse_batch(stream, ends, root=O.PARSE_VALUE)
    assert not st.any() and list(sz) == [len(e.data) for e in cat]


def test_reader_rules_hold_for_the_oracle():
    """What the GPU test asserts of every (reader kind, scalar entry) pair independently of the
    oracle (A.expect_read, written from the reference's decoders) is what the oracle's readers
    return: the two statements of the rules check each other here, the kernel against both on the
    GPU."""
    n = A.check_reads(O.decode_values)
    assert n > 14 * len(A.scalars())  # every reader but Bool() states a rule for every entry
    # the cross-width cases by name
    sc = A.scalars()
    assert A.expect_read(Kind.INT64, *sc["int32_m2147483648"]) == (0, (-2 ** 31).to_bytes(8, "little", signed=True))
    assert A.expect_read(Kind.INT32, *sc["int64_134217728"])[0] == 0
    assert A.expect_read(Kind.INT16, *sc["int32_8191"])[0] == 0 and A.expect_read(Kind.INT16, *sc["int64_m1048577"])[0] == 1
    assert A.expect_read(Kind.UINT16, *sc["uint32_16384"])[0] == 0 and A.expect_read(Kind.UINT32, *sc["uint64_34359738368"])[0] == 1
    assert A.expect_read(Kind.FLOAT32, *sc["float64_over_max_float32"]) == (1, bytes(4))
    err, sub = A.expect_read(Kind.FLOAT32, *sc["float64_float32_subnormal"])
    assert err == 0 and 0 < int.from_bytes(sub, "little") < 0x00800000  # a float32 subnormal
    assert A.expect_read(Kind.FLOAT32, *sc["float64_max"]) == (1, bytes(4))
    assert A.expect_read(Kind.FLOAT64, *sc["float32_pos_inf"]) == (0, (0x7FF0000000000000).to_bytes(8, "little"))
    assert A.expect_read(Kind.FLOAT32, *sc["float32_pos_inf"]) == (1, bytes(4))

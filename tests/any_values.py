"""A catalog of encoded values for `any` fields: every type DecodeTypeSize (internal/decode/
type.go:27-203) switches over, well-formed and malformed, each built with the oracle's own encoders
(no byte layout is restated here beyond the malformed tails, which no encoder will write).

    catalog()      [(name, bytes, cls)]: cls is what OpenValue / OpenValueErr (internal/types/
                   value.go:21-46) make of the bytes when they fill their slot:
                     ok     a value: the span is the slot's last n bytes
                     err    DecodeTypeSize errs: OpenValueErr's error, a nil value
                     nil    no error and no bytes (see below)
                     panic  n < 0: Go slices b[len(b)-n:] past the slot
    scalars()      {name: (Kind, value)} of the ok scalar entries: the Python value each was built
                   from (floats as their bit pattern, string / bytes / bin as the payload bytes)
    field_slot()   the bytes m.Field(tag) hands to OpenValue: in a message, a field's slot runs from
                   the message's first data byte to the field's end (msg.go:108-124), so the fields
                   written before an `any` field are junk before its value too
    placements()   every entry filling its slot and behind 1, 3 and 7 junk bytes in the same slot,
                   each with the oracle's answer for that slot
    open_value(b)  the oracle's OpenValue over a slot: (cls, span offset in the slot, span length)

`nil`: value.go:26 returns nil where len(b) < n, but every branch of DecodeTypeSize that computes
n from a size varint errs on exactly that condition, so no input reaches it.  The one value that
opens with no error and no bytes is a struct's type byte alone in its slot: decodeSize of the empty
prefix returns m = -1, type.go:190 checks n instead of m, and the size is 1 + (-1) + 0 = 0.  With
any byte before it in the slot the same tail reads a size varint, so its junk placements are another
class (SLOT_BOUND below)."""
from __future__ import annotations

import ctypes as C
import functools
import struct
from typing import NamedTuple

import numpy as np

from oracle import oracle as O
from spec_amd.schema import Kind
from tests.test_oracle_parse import _list, _msg, _raw_message, _struct

# Junk before a value in its slot: non-zero, every byte with the continuation bit set (no varint
# ends in it) and none a type code, so no tail of it is a value.
JUNK = bytes([0xA5, 0xC3, 0x96, 0xE1, 0xB7, 0x8D, 0xFA])
JUNK_LENS = (0, 1, 3, 7)

T_TRUE, T_FALSE, T_BYTE = 1, 2, 3
T_INT16, T_INT32, T_INT64, T_UINT16, T_UINT32, T_UINT64 = 10, 11, 12, 20, 21, 22
T_BIN64, T_BIN128, T_BIN256, T_FLOAT32, T_FLOAT64 = 30, 31, 32, 40, 41
T_BYTES, T_STRING, T_LIST, T_BIG_LIST, T_MESSAGE, T_BIG_MESSAGE, T_STRUCT = 50, 60, 70, 71, 80, 81, 90
SWITCH_TYPES = (T_TRUE, T_FALSE, T_BYTE, T_INT16, T_INT32, T_INT64, T_UINT16, T_UINT32, T_UINT64, T_BIN64, T_BIN128,
                T_BIN256, T_FLOAT32, T_FLOAT64, T_BYTES, T_STRING, T_LIST, T_BIG_LIST, T_MESSAGE, T_BIG_MESSAGE,
                T_STRUCT)
# the type byte of at least one malformed entry, per case of the malformed list
MALFORMED_TYPES = (99, 0, T_INT32, T_UINT32, T_INT64, T_FLOAT32, T_BIN256, T_STRING, T_BYTES, T_LIST, T_STRUCT)

PAYLOAD_LENS = (0, 1, 127, 128, 16383, 16384)  # the size varint moves 1 -> 2 -> 3 bytes
INT_BITS = {"int16": 16, "int32": 32, "int64": 64, "uint16": 16, "uint32": 32, "uint64": 64}
VARINT_MAX = {16: 3, 32: 5, 64: 10}

# float32 +-Inf is a value to OpenValue, and a range error to its own reader: DecodeFloat32 compares
# against +-MaxFloat32 (internal/decode/float.go:24-27).  Float64() reads both.
OWN_READER_ERRS = ("float32_pos_inf", "float32_neg_inf")

# Entries whose class is a property of where the slot starts, not of the value's bytes: the slot is
# too short for a fixed-size value (a byte more makes it whole), or the tail reads the empty prefix.
SLOT_BOUND = ("bad_byte_no_data", "bad_float32_3_bytes", "bad_bin256_31_bytes", "bad_string_no_room_for_nul",
              "nil_struct_type_only")


class Entry(NamedTuple):
    name: str
    data: bytes
    cls: str


class Placement(NamedTuple):
    entry: int   # index into catalog()
    junk: int    # junk bytes before the value in the slot
    slot: bytes  # JUNK[:junk] + data
    cls: str     # the oracle's class of the slot
    off: int     # the value's span within the slot (0, 0 unless cls is ok)
    size: int


def open_value(slot: bytes):
    """OpenValue(slot) by the oracle's DecodeTypeSize: (cls, span offset within the slot, length)."""
    if not slot:
        return "nil", 0, 0
    _, n, err = O.decode("type_size", slot)
    if err is not None:
        return "err", 0, 0
    if n < 0:
        return "panic", 0, 0
    if n == 0 or n > len(slot):
        return "nil", 0, 0
    return "ok", len(slot) - n, n


def field_slot(record: bytes, path) -> bytes:
    """The slot of field path[-1] of the message `record` (under the sub-messages path[:-1]): the
    message's data up to the field's end, b"" where the field is absent — found with the oracle's
    message table lookup, not with its tree reader."""
    L = O.lib()
    L.so_message_field_raw.restype = C.c_void_p
    L.so_message_field_raw.argtypes = [C.POINTER(O.CMessage), C.c_uint16, C.POINTER(C.c_size_t)]
    m = O.Message(record)
    assert m.err is None
    cur = m.m
    for tag in path[:-1]:
        sub = O.CMessage()
        L.so_message_message(C.byref(cur), tag, C.byref(sub))
        cur = sub
    ln = C.c_size_t(0)
    p = L.so_message_field_raw(C.byref(cur), path[-1], C.byref(ln))
    if not p or not ln.value:
        return b""
    off = p - m._base
    assert 0 <= off and off + ln.value <= len(record)
    return record[off: off + ln.value]


def int_values(kind: str):
    """min, -1, 0, 1, max and both sides of every reverse-varint length step of the kind (through
    zigzag for the signed kinds: the step to k + 1 bytes lies between 2^(7k-1) - 1 and 2^(7k-1),
    and between -2^(7k-1) and -2^(7k-1) - 1)."""
    bits = INT_BITS[kind]
    if kind.startswith("u"):
        lo, hi = 0, 2 ** bits - 1
        vals = {lo, 1, hi}
        for k in range(1, VARINT_MAX[bits]):
            vals |= {2 ** (7 * k) - 1, 2 ** (7 * k)}
    else:
        lo, hi = -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
        vals = {lo, -1, 0, 1, hi}
        for k in range(1, VARINT_MAX[bits]):
            h = 2 ** (7 * k - 1)
            vals |= {h - 1, h, -h, -h - 1}
    return sorted(v for v in vals if lo <= v <= hi)


F32 = {"pos_zero": 0x00000000, "neg_zero": 0x80000000, "min_subnormal": 0x00000001, "max": 0x7F7FFFFF,
       "pos_inf": 0x7F800000, "neg_inf": 0xFF800000, "nan_payload": 0x7FC12345}
F64 = {"pos_zero": 0, "neg_zero": 1 << 63, "min_subnormal": 1, "max": 0x7FEFFFFFFFFFFFFF,
       "pos_inf": 0x7FF0000000000000, "neg_inf": 0xFFF0000000000000, "nan_payload": 0x7FF8000012345678,
       "over_max_float32": 0x47EFFFFFE0000001,  # MaxFloat32 = 0x47EFFFFFE0000000 as a float64
       "float32_subnormal": struct.unpack("<Q", struct.pack("<d", 1e-40))[0]}


def _enc(kind, v):
    b, n, err = O.encode(kind, v)
    assert err is None and n == len(b), (kind, v, err)
    return b


@functools.lru_cache(maxsize=None)
def _build():
    rng = np.random.default_rng(1234)
    out, values = [], {}

    def add(name, data, cls, kind=None, value=None):
        assert name not in {e.name for e in out}, name
        out.append(Entry(name, bytes(data), cls))
        if kind is not None:
            values[name] = (kind, value)

    add("bool_true", _enc("bool", 1), "ok", Kind.BOOL, True)
    add("bool_false", _enc("bool", 0), "ok", Kind.BOOL, False)
    for v in (0, 255):
        add(f"byte_{v}", _enc("byte", v), "ok", Kind.BYTE, v)
    for kind in INT_BITS:
        for v in int_values(kind):
            add(f"{kind}_{v}".replace("-", "m"), _enc(kind, v), "ok", Kind[kind.upper()], v)
    for name, bits in F32.items():
        add(f"float32_{name}", _enc("float32", struct.unpack("<f", struct.pack("<I", bits))[0]), "ok", Kind.FLOAT32,
            bits)
    for name, bits in F64.items():
        add(f"float64_{name}", _enc("float64", struct.unpack("<d", struct.pack("<Q", bits))[0]), "ok", Kind.FLOAT64,
            bits)
    for w in (64, 128, 256):
        raw = rng.integers(0, 256, w // 8, dtype=np.uint8).tobytes()
        add(f"bin{w}", _enc(f"bin{w}", raw), "ok", Kind[f"BIN{w}"], raw)
    for kind in ("string", "bytes"):
        for ln in PAYLOAD_LENS:
            raw = rng.integers(1 if kind == "string" else 0, 256, ln, dtype=np.uint8).tobytes()
            add(f"{kind}_{ln}", _enc(kind, raw), "ok", Kind[kind.upper()], raw)
    add("string_embedded_nul", _enc("string", b"ab\0cd"), "ok", Kind.STRING, b"ab\0cd")

    i64, s = _enc("int64", 7), _enc("string", b"hey")
    small = _msg([(1, "int64", 5), (2, "string", "abc")])
    add("list_empty", _list([]), "ok")
    add("list_three_scalars", _list([i64, s, _enc("float64", 1.5)]), "ok")
    add("list_300_elements", _list([i64] * 300), "ok")  # big by count
    add("list_data_over_65535", _list([_enc("bytes", bytes(40000)), _enc("bytes", bytes(range(256)) * 120)]), "ok")
    add("message_empty", _msg([]), "ok")
    add("message_small", small, "ok")
    add("message_big_tag", _msg([(1, "int32", -3), (300, "int32", 5)]), "ok")
    add("message_list_message", _raw_message([i64, _list([small, _msg([(2, "string", "x")])])]), "ok")
    add("struct_0", _struct(b""), "ok")
    add("struct_127", _struct(bytes(range(127))), "ok")
    add("struct_128", bytes(range(128)) + _enc("struct", 128), "ok")
    # DecodeTypeSize takes any varint of up to ten bytes for any integer type (type.go:52-66):
    # well-formed to OpenValue, a range error to Int16() (internal/decode/int.go)
    add("int16_four_byte_varint", bytes([0x01, 0x80, 0x80, 0x80, T_INT16]), "ok")

    add("bad_type_99", bytes([1, 2, 99]), "err")
    add("bad_type_0", bytes([5, 0]), "err")
    add("bad_int32_varint_to_slot_start", bytes([0x80, 0x81, T_INT32]), "err")
    add("bad_uint32_varint_to_slot_start", bytes([0x80, T_UINT32]), "err")
    add("bad_int64_eleven_byte_varint", bytes([0x01] + [0x80] * 10 + [T_INT64]), "err")
    add("bad_uint64_eleven_byte_varint", bytes([0x01] + [0x80] * 10 + [T_UINT64]), "err")
    add("bad_byte_no_data", bytes([T_BYTE]), "err")
    add("bad_float32_3_bytes", bytes([1, 2, 3, T_FLOAT32]), "err")
    add("bad_bin256_31_bytes", bytes(range(1, 32)) + bytes([T_BIN256]), "err")
    add("bad_string_size_over_slot", b"abc\0" + O.put_reverse_uint32(100) + bytes([T_STRING]), "err")
    add("bad_string_no_room_for_nul", b"abc" + O.put_reverse_uint32(3) + bytes([T_STRING]), "err")
    add("bad_bytes_size_varint", bytes([0x80, 0x80, T_BYTES]), "err")
    add("bad_list_table_over_slot", bytes([0]) + O.put_reverse_uint32(100) + bytes([T_LIST]), "err")
    add("bad_list_data_size_varint", bytes([0x80]) + O.put_reverse_uint32(2) + bytes([T_LIST]), "err")
    add("bad_message_table_over_slot", bytes([0]) + O.put_reverse_uint32(200) + bytes([T_MESSAGE]), "err")
    add("bad_struct_past_slot", _struct(b"", ds=9), "err")
    add("panic_struct_size_varint", bytes([0x80, T_STRUCT]), "panic")  # "m unchecked": n = 1 - 2 < 0
    add("nil_struct_type_only", bytes([T_STRUCT]), "nil")
    return tuple(out), values


def catalog():
    return list(_build()[0])


def scalars():
    return dict(_build()[1])


@functools.lru_cache(maxsize=None)
def placements():
    out = []
    for i, e in enumerate(catalog()):
        for k in JUNK_LENS:
            slot = JUNK[:k] + e.data
            out.append(Placement(i, k, slot, *open_value(slot)))
    return tuple(out)


def heap_and_spans(pls):
    """The slots of `pls` back to back: (heap uint8, slot spans uint32 [len(pls), 2])."""
    spans, off = np.zeros((len(pls), 2), np.uint32), 0
    for j, p in enumerate(pls):
        spans[j] = (off, len(p.slot))
        off += len(p.slot)
    return np.frombuffer(b"".join(p.slot for p in pls), np.uint8).copy(), spans


# ---- what each reader makes of each scalar entry, from the reference's decoders ------------------

SIGNED = {Kind.INT16: 16, Kind.INT32: 32, Kind.INT64: 64}
UNSIGNED = {Kind.UINT16: 16, Kind.UINT32: 32, Kind.UINT64: 64}
FLOATS = (Kind.FLOAT32, Kind.FLOAT64)
WIDTHS = {Kind.BOOL: 1, Kind.BYTE: 1, Kind.INT16: 2, Kind.INT32: 4, Kind.INT64: 8, Kind.UINT16: 2, Kind.UINT32: 4,
          Kind.UINT64: 8, Kind.FLOAT32: 4, Kind.FLOAT64: 8, Kind.BIN64: 8, Kind.BIN128: 16, Kind.BIN256: 32,
          Kind.STRING: 8, Kind.BYTES: 8}
MAX_FLOAT32 = struct.unpack("<d", struct.pack("<Q", 0x47EFFFFFE0000000))[0]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def expect_read(reader: Kind, kind: Kind, v):
    """Value.<reader>Err() of an ok scalar entry of `kind` built from v -> (err, column bytes, or
    the payload for string / bytes), or None where no rule is stated here.  From the reference:
    an integer reader takes any integer type of its signedness and range-checks the value
    (internal/decode/int.go, uint.go); Float64() widens a float32, Float32() takes a float64 within
    +-MaxFloat32 or NaN and rounds it (float.go:15-32: +-Inf is out of range, of either width); any
    other reader of another type errs "invalid type", and every error returns the zero value.
    Bool() takes any type without error (byte.go): only bool entries are stated."""
    zero = b"" if reader in (Kind.STRING, Kind.BYTES) else bytes(WIDTHS[reader])
    if reader in SIGNED and kind in SIGNED or reader in UNSIGNED and kind in UNSIGNED:
        bits, signed = {**SIGNED, **UNSIGNED}[reader], reader in SIGNED
        lo, hi = (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if signed else (0, 2 ** bits - 1)
        return (0, v.to_bytes(bits // 8, "little", signed=signed)) if lo <= v <= hi else (1, zero)
    if reader in FLOATS and kind in FLOATS:
        x = _f32(v) if kind == Kind.FLOAT32 else _f64(v)  # (struct widens a float32 as Go's float64(f) does)
        if reader == Kind.FLOAT64:
            return 0, v.to_bytes(8, "little") if kind == Kind.FLOAT64 else struct.pack("<d", x)
        if x == x and abs(x) > MAX_FLOAT32:
            return 1, zero
        return 0, v.to_bytes(4, "little") if kind == Kind.FLOAT32 else struct.pack("<f", x)
    if reader == Kind.BOOL:
        return (0, bytes([1 if v else 0])) if kind == Kind.BOOL else None
    if reader != kind:
        return 1, zero
    if kind == Kind.BYTE:
        return 0, bytes([v])
    return 0, bytes(v)  # bin: the bytes; string / bytes: the payload


def check_reads(read):
    """Every ok scalar entry, alone and behind junk, through every reader kind: `read(kind, stream
    uint8, spans uint32 [n, 2]) -> (values uint8 [n, width], err uint8 [n])` gives what expect_read
    states.  A string / bytes value is a span of absolute stream offsets whose bytes are the payload
    ((0, 0) for an empty one).  Returns the number of (reader, value) pairs checked."""
    cat, sc = catalog(), scalars()
    pls = [p for p in placements() if cat[p.entry].name in sc]
    heap, spans = heap_and_spans(pls)
    for j, p in enumerate(pls):
        assert p.cls == "ok" and p.size == len(cat[p.entry].data)
        spans[j] = (spans[j, 0] + p.off, p.size)
    checked = 0
    for reader in (Kind(k) for k in range(1, 16)):
        vals, err = read(reader, heap, spans)
        vals, err = np.asarray(vals), np.asarray(err)
        assert vals.shape == (len(pls), WIDTHS[reader]) and err.shape == (len(pls),)
        for j, p in enumerate(pls):
            name = cat[p.entry].name
            want = expect_read(reader, *sc[name])
            if want is None:
                continue
            checked += 1
            got = bytes(vals[j])
            assert int(err[j]) == want[0], (reader.name, name, p.junk, int(err[j]))
            if reader in (Kind.STRING, Kind.BYTES):
                off, ln = struct.unpack("<II", got)
                assert ln == len(want[1]) and (off, ln) != (0, 0) or (off, ln) == (0, 0) and not want[1], (reader.name, name)
                assert bytes(heap[off: off + ln]) == want[1], (reader.name, name, p.junk)
                if ln:  # the payload lies inside the value's own span
                    assert spans[j, 0] <= off and off + ln < spans[j, 0] + spans[j, 1], (reader.name, name)
            else:
                assert got == want[1], (reader.name, name, p.junk, got.hex(), want[1].hex())
    return checked

"""Builders for the parse validator's tests (spec_parse_messages / spec_parse_batch, validate.hip) and a
CPU-side statement of every condition those tests rely on.

    levels(record, root)   the deepest chain of containers (lists and messages whose tables decode) on
                           any path of the record, the root container included: a walk over the
                           oracle's table decoders, independent of the kernel.  validate.hip keeps one
                           stack frame per container of the current path, so a record of more than 32
                           levels is parsed again by deep_kernel, one of more than 8,192 by its
                           whole-arena thread.
    nest(depth, inner, via)  `inner` wrapped in `depth` containers of the kinds `via` names from the
                           outermost inward (cycled): message, list, big_message (tag 300), big_list
                           (300 elements)
    slab_bytes / group_fits  decode_core.hpp's decode_slab_bytes and make_group's in_lds, restated
    check_parse            the C entry point on a device batch against the oracle, with canaries round
                           status and sizes, a stream placed anywhere in its allocation, sizes = NULL
    value_placements()     tests/any_values.py's 720 placements plus the 16-bit integers just outside
                           their range, each with the status ParseValue must give where a rule is
                           stated here (scalar_rule)
    the batches of the tests: value_batches, depth_batch, deep_mode_batch — built once per process"""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

from oracle import oracle as O
from tests import any_values as A
from tests.gpu_helpers import concat_records
from tests.test_oracle_parse import _list, _msg, _raw_message

ROOT_MESSAGE, ROOT_LIST, ROOT_VALUE = O.PARSE_MESSAGE, O.PARSE_LIST, O.PARSE_VALUE
ROOTS = (ROOT_MESSAGE, ROOT_LIST, ROOT_VALUE)
VAL_MAX_DEPTH = 32       # validate.hip: frames of the main pass's stack
ARENA_SLICE = 8192       # validate.hip: DEEP_ARENA / sizeof(Frame) / DEEP_THREADS frames per deep thread
DEEP_LIST_CAP = 1 << 16  # validate.hip: records the main pass can list for the deep pass
LIST_TYPES, MESSAGE_TYPES = (A.T_LIST, A.T_BIG_LIST), (A.T_MESSAGE, A.T_BIG_MESSAGE)
ST_PANIC, ST_INVALID_VALUE, ST_TOO_DEEP = 6, 7, 8


# ---- levels ----------------------------------------------------------------------------------------

def levels(record: bytes, root: int, want_big=None) -> int:
    """The deepest container count on any path of `record` under `root`.  A container counts when
    its table decodes (DecodeMessageTable / DecodeListTable); its entries are followed as ParseMessage
    and ParseList follow them (an end past the data or an empty slice is skipped, a list element whose
    start lies past its end is not entered).  want_big: a list that receives (level, big) of every
    container met, level 1 = the root container."""
    record = bytes(record)
    if not record:
        return 0
    L = O.lib()
    buf = C.create_string_buffer(record, len(record))
    base = C.addressof(buf)
    mt, lt, n = O.MessageTable(), O.ListTable(), C.c_int(0)
    mf, s64, e64 = O.MessageField(), C.c_int64(0), C.c_int64(0)
    best = 0
    work = [(0, len(record), {ROOT_MESSAGE: "m", ROOT_LIST: "l", ROOT_VALUE: "v"}[root], 0)]
    while work:
        lo, e, kind, d = work.pop()
        if e <= lo:
            continue
        if kind == "v":
            t = record[e - 1]
            if t not in LIST_TYPES and t not in MESSAGE_TYPES:
                continue
            kind = "l" if t in LIST_TYPES else "m"
        p = C.cast(base + lo, C.c_char_p)
        if kind == "m":
            if L.so_decode_message_table(p, e - lo, C.byref(mt), C.byref(n)) is not None:
                continue
            ds, big = e - n.value, bool(mt.big)
            for i in range(L.so_message_table_len(C.byref(mt))):
                L.so_message_table_field(C.byref(mt), i, C.byref(mf))
                if 0 < mf.offset <= mt.data:
                    work.append((ds, ds + mf.offset, "v", d + 1))
        else:
            if L.so_decode_list_table(p, e - lo, C.byref(lt), C.byref(n)) is not None:
                continue
            ds, big = e - n.value, bool(lt.big)
            for i in range(L.so_list_table_len(C.byref(lt))):
                L.so_list_table_offset(C.byref(lt), i, C.byref(s64), C.byref(e64))
                if s64.value < e64.value <= lt.data:
                    work.append((ds + s64.value, ds + e64.value, "v", d + 1))
        best = max(best, d + 1)
        if want_big is not None:
            want_big.append((d + 1, big))
    return best


# ---- nest --------------------------------------------------------------------------------------------

VIA_KINDS = ("message", "list", "big_message", "big_list")


def _trailer(kind: str, n: int) -> bytes:
    """The trailer of a container of `kind` whose one non-empty entry is the n bytes before it."""
    if kind == "message":
        t, _, err = O.encode_message_table(n, [(1, n)])
    elif kind == "big_message":  # a tag over 255 makes the table big (internal/format/msg.go:43-61)
        t, _, err = O.encode_message_table(n, [(300, n)])
    elif kind == "list":
        t, _, err = O.encode_list_table(n, [n])
    elif kind == "big_list":     # more than 255 elements; elements 1.. are empty and skipped
        t, _, err = O.encode_list_table(n, [n] * 300)
    else:
        raise ValueError(kind)
    assert err is None, err
    return t


def nest(depth: int, inner: bytes, via=("message",)) -> bytes:
    """`inner` inside `depth` containers, each holding only the next: level d from the outside
    (0 = the outermost) is of kind via[d % len(via)].  Trailers are appended to one growing
    bytearray (a container's data is everything written so far)."""
    b = bytearray(inner)
    for d in range(depth - 1, -1, -1):
        b += _trailer(via[d % len(via)], len(b))
    return bytes(b)


# ---- slab and group --------------------------------------------------------------------------------

SLAB_GUARD, CHUNK, SLAB_MAX_CHUNKS, SLAB_MARGIN = 48, 1024, 40, 1.04


def slab_bytes(avg: float) -> int:
    """decode_core.hpp decode_slab_bytes(avg): the LDS bytes per group of a batch whose mean record
    (stream_len / n) is avg; 0: every group parses from HBM."""
    chunks = int(avg * 64 * SLAB_MARGIN / CHUNK) + 1
    return 0 if chunks > SLAB_MAX_CHUNKS else SLAB_GUARD + chunks * CHUNK + 32


def group_fits(ends, head: int, base: int, slab: int) -> bool:
    """make_group's in_lds for the group of up to 64 records from `base`: the span from the first
    record's start (rounded down to 16) to the last record's end, in whole 1 KiB chunks, plus the
    guard and 16 bytes, fits the slab."""
    n = len(ends)
    nrec = min(64, n - base)
    lo = (int(ends[base - 1]) if base else 0) + head
    hi = int(ends[base + nrec - 1])
    origin = lo & ~15
    granules = (hi - origin + 15) >> 4 if hi > origin else 0
    staged = ((granules + 63) >> 6) * CHUNK
    return slab > 0 and hi >= lo and SLAB_GUARD + staged + 16 <= slab


def batch_paths(stream_len: int, ends, head: int = 0):
    """(slab, [in_lds of every group]) of a batch as launch_parse sees it."""
    slab = slab_bytes(stream_len / len(ends))
    return slab, [group_fits(ends, head, b, slab) for b in range(0, len(ends), 64)]


# ---- running the entry point -----------------------------------------------------------------------

CANARY = 64


def run_parse(dev, stream, ends, head=0, root=ROOT_MESSAGE, sizes=True, offset=0, stream_len=None):
    """spec_parse_batch through the C entry point: the stream `offset` bytes into an allocation that
    ends where the stream ends, status and sizes each between two 64-byte canaries.  Returns
    (rc, status, sizes or None); asserts the canaries are intact."""
    import torch

    import spec_amd

    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    n = len(ends)
    slen = stream.size if stream_len is None else stream_len
    d_alloc = torch.empty(max(offset + stream.size, 1), dtype=torch.uint8, device=dev)
    d_alloc[offset:offset + stream.size] = torch.from_numpy(stream).to(dev)
    d_ends = torch.from_numpy(ends.view(np.int64)).to(dev)
    d_st = torch.full((n + 2 * CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    d_sz = torch.full((n + 2 * CANARY // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rc = spec_amd.lib().spec_parse_batch(root, d_alloc.data_ptr() + offset, slen, d_ends.data_ptr(), n, head,
                                         d_st.data_ptr() + CANARY, d_sz.data_ptr() + CANARY if sizes else None,
                                         None)
    torch.cuda.synchronize()
    st, sz = d_st.cpu().numpy(), d_sz.cpu().numpy().view(np.uint32)
    assert (st[:CANARY] == 0xA5).all() and (st[CANARY + n:] == 0xA5).all(), "status canary"
    w = CANARY // 4
    assert (sz[:w] == 0x5A5A5A5A).all() and (sz[w + n:] == 0x5A5A5A5A).all(), "sizes canary"
    if not sizes:
        assert (sz == 0x5A5A5A5A).all(), "sizes written with sizes = NULL"
    return rc, st[CANARY:CANARY + n].copy(), sz[w:w + n].copy() if sizes else None


def check_parse(dev, stream, ends, head=0, label="", root=ROOT_MESSAGE, sizes=True, offset=0, want=None):
    """run_parse == O.parse_batch on the same bytes, bit for bit (want: the oracle's answer where the
    caller has it already).  Returns (status, sizes or None)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    want_st, want_sz = want if want is not None else O.parse_batch(stream, ends, head, root=root)
    rc, st, sz = run_parse(dev, stream, ends, head, root, sizes, offset)
    assert rc == 0, f"{label}: rc {rc}"
    if not np.array_equal(st, want_st):
        i = int(np.nonzero(st != want_st)[0][0])
        raise AssertionError(f"{label}: record {i}: status gpu={st[i]} oracle={want_st[i]}")
    if sizes and not np.array_equal(sz, want_sz):
        i = int(np.nonzero(sz != want_sz)[0][0])
        raise AssertionError(f"{label}: record {i}: size gpu={sz[i]} oracle={want_sz[i]}")
    return st, sz


# ---- the value catalog ------------------------------------------------------------------------------

CONTAINER_TYPES = LIST_TYPES + MESSAGE_TYPES
# ParseValue runs the type's own decoder (internal/types/value.go:49-113), which checks what
# DecodeTypeSize does not: DecodeFloat32 compares against +-MaxFloat32 (internal/decode/float.go:
# 24-27: +-Inf errs), DecodeInt16 / DecodeUint16 read a 32-bit varint and range-check it
# (internal/decode/int.go:16-62, uint.go:16-56).  The catalog's ok entries that these reject:
RANGE_ERRS = ("float32_pos_inf", "float32_neg_inf",
              "int16_four_byte_varint")  # bytes 01 80 80 80: 1 << 21, zigzag 1 << 20 > 32767


def _retyped(kind: str, v: int, type_byte: int) -> bytes:
    """v written by the 32-bit encoder of `kind` under a 16-bit type byte: the varint is the one
    DecodeInt16 / DecodeUint16 read, which no encoder of theirs writes for a value out of range."""
    b, _, err = O.encode(kind, v)
    assert err is None
    return b[:-1] + bytes([type_byte])


def extra_entries():
    """The 16-bit integers just outside their range (any_values holds the ones just inside):
    (name, bytes)."""
    return [("uint16_65536", _retyped("uint32", 65536, A.T_UINT16)),
            ("uint16_131071", _retyped("uint32", 0x1FFFF, A.T_UINT16)),
            ("uint16_131072", _retyped("uint32", 0x20000, A.T_UINT16)),
            ("uint16_max_uint32", _retyped("uint32", 0xFFFFFFFF, A.T_UINT16)),
            ("int16_32768", _retyped("int32", 32768, A.T_INT16)),
            ("int16_m32769", _retyped("int32", -32769, A.T_INT16)),
            ("int16_min_int32", _retyped("int32", -2 ** 31, A.T_INT16))]


class Value(NamedTuple):
    name: str
    junk: int
    slot: bytes  # JUNK[:junk] + the value
    rule: tuple  # (status, size) ParseValue(slot) must give by scalar_rule, or None
    large: bool  # over LARGE bytes: not in the batches that parse from LDS


LARGE = 300


def scalar_rule(name: str, data: bytes, cls: str):
    """ParseValue of the slot junk + data, stated apart from the oracle: an ok catalog entry whose
    type is a scalar of DecodeTypeSize's switch parses to its own length whatever lies before it,
    except RANGE_ERRS (7).  The extra entries are range errors.  None: no rule stated here."""
    if cls == "extra" or name in RANGE_ERRS:
        return ST_INVALID_VALUE, 0
    if cls == "ok" and data[-1] in A.SWITCH_TYPES and data[-1] not in CONTAINER_TYPES:
        return 0, len(data)
    return None


@functools.lru_cache(maxsize=None)
def value_placements():
    cat = A.catalog()
    out = [Value(cat[p.entry].name, p.junk, p.slot, scalar_rule(*cat[p.entry]), len(p.slot) > LARGE)
           for p in A.placements()]
    for name, data in extra_entries():
        out += [Value(name, k, A.JUNK[:k] + data, scalar_rule(name, data, "extra"), False) for k in A.JUNK_LENS]
    return tuple(out)


I64 = O.encode("int64", 7)[0]
# (embedding, the roots it runs under, slot -> record)
EMBEDDINGS = (
    ("alone", (ROOT_VALUE,), lambda s: s),
    ("list_middle", (ROOT_LIST, ROOT_VALUE), lambda s: _list([I64, s, I64])),
    ("message_second", (ROOT_MESSAGE, ROOT_VALUE), lambda s: _raw_message([I64, s])),
    ("message_list", (ROOT_MESSAGE,), lambda s: _raw_message([_list([s])])),
)


class Batch(NamedTuple):
    stream: np.ndarray
    ends: np.ndarray
    keys: tuple  # per record: an index into value_placements(), or -1 for a filler


def _batch(recs, keys):
    stream, ends = concat_records(recs)
    return Batch(stream, ends, tuple(keys))


def _dealt(idx, size_of):
    """idx dealt into groups of 64 of about equal bytes (largest first, round-robin over the groups
    that still have room; the last group is the partial one), so that every group's span stays near
    64 mean records."""
    order = sorted(idx, key=size_of, reverse=True)
    g = (len(order) + 63) // 64
    room = [64] * (g - 1) + [len(order) - 64 * (g - 1)]
    groups, k = [[] for _ in range(g)], 0
    for i in order:
        while len(groups[k % g]) == room[k % g]:
            k += 1
        groups[k % g].append(i)
        k += 1
    return [i for x in groups for i in x]


OVER_SLAB = 8192   # the filler record of the group-level fallback
FALLBACK_PAD = 448  # empty records behind it: they keep the batch's mean record, hence its slab, small


@functools.lru_cache(maxsize=None)
def value_batches(embedding: str):
    """The batches of one embedding, by the instantiation of parse_record they are built for:
        lds       the small values, every group within the batch's slab    (LdsSrc, LocalStack)
        fallback  the same records, each group of 64 led by one record of OVER_SLAB bytes, behind
                  FALLBACK_PAD empty records: slab > 0, no group of values fits (GlobalSrc, LocalStack)
        hbm       every value, the large ones among them: a mean record with no slab (GlobalSrc, LocalStack)
        deep      every value in messages up to 33 levels                     (GlobalSrc, ArenaStack)
    """
    embed = {e[0]: e[2] for e in EMBEDDINGS}[embedding]
    vals = value_placements()
    recs = [embed(v.slot) for v in vals]
    small = _dealt([i for i, v in enumerate(vals) if not v.large], lambda i: len(recs[i]))
    out = {"lds": _batch([recs[i] for i in small], small)}
    filler = O.encode("bytes", bytes(OVER_SLAB))[0]
    r, k = [], []
    for j, i in enumerate(small):
        if j % 63 == 0:
            r.append(filler)
            k.append(-1)
        r.append(recs[i])
        k.append(i)
    out["fallback"] = _batch(r + [b""] * FALLBACK_PAD, k + [-1] * FALLBACK_PAD)
    out["hbm"] = _batch(recs, range(len(recs)))
    deep = [nest(VAL_MAX_DEPTH + 1 - levels(rec, ROOT_VALUE), rec) for rec in recs]
    out["deep"] = _batch(deep, range(len(recs)))
    return out


# ---- depth boundaries --------------------------------------------------------------------------------

SMALL_DEPTHS = (31, 32, 33, 34)
LARGE_DEPTHS = (8191, 8192, 8193)
FORMS = ("good", "bad_value", "swapped_list")
GOOD_VALUE = O.encode("int32", 7)[0]
BAD_VALUE = bytes([1, 2, 3, 99])  # an unsupported type
SWAPPED_LIST = I64 + I64 + O.encode_list_table(2 * len(I64), [2 * len(I64), len(I64)])[0]  # start > end: Go panics
FORM_STATUS = {"good": 0, "bad_value": ST_INVALID_VALUE, "swapped_list": ST_PANIC}


def vias(total: int, wraps: int):
    """The five nestings of the `wraps` outer containers of a record of `total` levels: messages,
    lists, both alternating, and messages / lists with a big one at the level that crosses the nearest
    boundary below `total` (level 33 or 8,193 from the outside), or at the innermost of the wraps
    where the record stays under both or crosses with a level of its inner value."""
    cross = ARENA_SLICE if total > ARENA_SLICE else VAL_MAX_DEPTH
    at = min(cross, wraps - 1)  # index from the outside

    def one_big(kind):
        return tuple(("big_" + kind) if d == at else kind for d in range(wraps))

    return {"messages": ("message",), "lists": ("list",), "alternating": ("message", "list"),
            "big_message": one_big("message"), "big_list": one_big("list")}


class DepthRecord(NamedTuple):
    name: str
    levels: int
    form: str
    via: str
    data: bytes


@functools.lru_cache(maxsize=None)
def depth_records(depths=SMALL_DEPTHS + LARGE_DEPTHS):
    """Every depth x nesting x form.  The swapped list is a level of its own (its table decodes), so
    it sits inside one container fewer."""
    out = []
    for total in depths:
        for form in FORMS:
            wraps = total - 1 if form == "swapped_list" else total
            inner = {"good": GOOD_VALUE, "bad_value": BAD_VALUE, "swapped_list": SWAPPED_LIST}[form]
            for vname, via in vias(total, wraps).items():
                out.append(DepthRecord(f"{total}_{vname}_{form}", total, form, vname, nest(wraps, inner, via)))
    return tuple(out)


# records of the batch that holds every depth (the batch of the boundary at 32 alone: 128 fewer); n % 64
# is 63 and 1: the last deep record is the last of a partial group
DEPTH_BATCH_SIZES = (255, 257)


def shallow_records():
    """What lies between the deep records of a batch: good and bad ones of up to three levels."""
    good = _msg([(1, "int64", 5), (2, "string", "abc")])
    return [good, _list([I64, good]), I64, _raw_message([BAD_VALUE]), b"", nest(3, GOOD_VALUE, ("list", "message")),
            _raw_message([SWAPPED_LIST]), bytes([0xFF, 80])]


@functools.lru_cache(maxsize=None)
def depth_batch(n: int, depths=SMALL_DEPTHS + LARGE_DEPTHS):
    """n records: depth_records(depths) at record 0, at record n - 1 and spread evenly between, shallow
    records everywhere else.  Returns (stream, ends, {record index: DepthRecord})."""
    deep = depth_records(depths)
    assert n >= 2 * len(deep) - 1
    at = {int(round(k * (n - 1) / (len(deep) - 1))): d for k, d in enumerate(deep)}
    assert len(at) == len(deep) and 0 in at and n - 1 in at
    fill = shallow_records()
    recs = [at[i].data if i in at else fill[i % len(fill)] for i in range(n)]
    stream, ends = concat_records(recs)
    return stream, ends, at


def frame_batch(stream, ends):
    """The batch as mpx frames: (frames, frame ends) for head = 4."""
    import spec_amd

    fr = spec_amd.make_frames(stream, ends)
    fends, _ = spec_amd.frames_index(fr)
    return fr, np.asarray(fends, dtype=np.uint64)


# ---- deep_kernel's two modes ---------------------------------------------------------------------------

DEEP_BLOCK = 64  # distinct records of the tiled block


@functools.lru_cache(maxsize=None)
def deep_mode_batch(count: int):
    """A batch with exactly `count` records of more than 32 levels: a block of DEEP_BLOCK distinct
    records (48 of 33 levels and about 220 bytes, 6 of them with a malformed innermost value; 8 shallow
    good ones; 8 shallow bad ones) tiled with np.tile, one record of 8,193 levels in the middle, and
    33-level records behind to make the count exact.  Returns (stream, ends, deep per record)."""
    block, deep = [], []
    for k in range(DEEP_BLOCK):
        tail = O.encode("int32", 1000 + k)[0]
        if k % 8 == 6:
            block.append(_raw_message([tail, O.encode("int64", k)[0]]))
            deep.append(False)
        elif k % 8 == 7:
            block.append(_raw_message([tail, BAD_VALUE]))
            deep.append(False)
        else:
            inner = _raw_message([tail, BAD_VALUE if k % 8 == 3 else O.encode("int64", k)[0]])
            block.append(nest(VAL_MAX_DEPTH, inner, ("message", "list") if k % 2 else ("message",)))
            deep.append(True)
    per = sum(deep)
    whole = nest(ARENA_SLICE + 1, GOOD_VALUE)
    reps = (count - 1) // per
    rest = count - 1 - reps * per
    bstream, bends = concat_records(block)
    half = reps // 2
    extra = [r for r, d in zip(block, deep) if d][:rest]
    xs, xe = concat_records(extra) if extra else (np.zeros(0, np.uint8), np.zeros(0, np.uint64))
    parts, ends, off = [], [], 0
    for s, e, rep in ((bstream, bends, half), (np.frombuffer(whole, np.uint8), np.array([len(whole)], np.uint64), 1),
                      (bstream, bends, reps - half), (xs, xe, 1)):
        if not len(e) or not rep:
            continue
        parts.append(np.tile(s, rep))
        ends.append((e[None, :] + (np.arange(rep, dtype=np.uint64) * np.uint64(s.size))[:, None]).ravel() + np.uint64(off))
        off += s.size * rep
    is_deep = np.concatenate([np.tile(np.array(deep), half), [True], np.tile(np.array(deep), reps - half),
                              np.ones(len(extra), bool)])
    return np.concatenate(parts), np.concatenate(ends), is_deep

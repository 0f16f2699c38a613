"""Shared helpers of the optional-field tests (tests/test_gpu_present_decode.py,
tests/test_gpu_present_encode.py): sparse records from the oracle Writer (only the setters of a
record's mask), HasField masks from the oracle Message, and the device calls through the C ABI on
prefilled buffers with canary rows."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import Kind, workload
from spec_amd.schema import NP_DTYPE, VARLEN
from tests.gpu_helpers import concat_records, to_dev
from tests.test_gpu_flat import ORACLE_NAME

BINS = (Kind.BIN64, Kind.BIN128, Kind.BIN256)
CANARY = 0x5CA1AB1E0DDBA11
PAD = 8  # canary words on either side of a mask


def words_of(schema) -> int:
    return max(1, (len(schema) + 63) // 64)


def value_of(schema, cols, heaps, f, i):
    """Record i's value of field f, as the oracle Writer's setter takes it."""
    kind = schema.fields[f].kind
    row = cols[f][i]
    if kind in BINS:
        return bytes(row)
    if kind in VARLEN:
        off, ln = (int(x) for x in row.view(np.uint32))
        return bytes(heaps[f][off:off + ln])
    if kind in (Kind.FLOAT32, Kind.FLOAT64):  # (the columns hold the floats' bits)
        return float(row.view(np.float32 if kind == Kind.FLOAT32 else np.float64)[0])
    v = row.view(NP_DTYPE[kind])[0]
    return bool(v) if kind == Kind.BOOL else int(v)


def write_sparse(schema, cols, heaps, bits, n):
    """bits: bool [n, nfields].  The oracle Writer's records: w.Field(tag_f).<Kind_f>(v) for exactly the
    f with bits[i, f], in schema order, then Build() -> [bytes]."""
    recs = []
    for i in range(n):
        w = O.Writer()
        w.message()
        for f, fld in enumerate(schema.fields):
            if bits[i, f]:
                err = w.field(fld.tag, ORACLE_NAME[fld.kind], value_of(schema, cols, heaps, f, i))
                assert err is None, err
        data, err = w.end()
        assert err is None, err
        w.close()
        recs.append(data)
    return recs


def pack_mask(bits: np.ndarray) -> np.ndarray:
    """bool [n, nfields] -> uint64 [words, n], word-major (bit f & 63 of word f >> 6)."""
    n, nf = bits.shape
    words = max(1, (nf + 63) // 64)
    m = np.zeros((words, n), np.uint64)
    for f in range(nf):
        m[f >> 6] |= bits[:, f].astype(np.uint64) << np.uint64(f & 63)
    return m


def oracle_present(schema, recs) -> np.ndarray:
    """m.HasField(tag_f) on the m of OpenMessageErr(record) -> uint64 [words, n]."""
    bits = np.zeros((len(recs), len(schema)), bool)
    for i, r in enumerate(recs):
        m = O.Message(r)
        for f, fld in enumerate(schema.fields):
            bits[i, f] = m.has_field(fld.tag)
    return pack_mask(bits)


def patterns(nf: int, n: int):
    """The mask patterns of the issue: name -> bool [n, nfields]."""
    out = {"all": np.ones((n, nf), bool), "none": np.zeros((n, nf), bool)}
    for seed in range(3):
        out[f"half{seed}"] = np.random.default_rng(900 + seed).random((n, nf)) < 0.5
    one = np.zeros((n, nf), bool)
    one[np.arange(n), np.arange(n) % nf] = True  # record i holds only field i mod nfields
    out["one_field"] = one
    first = np.zeros((n, nf), bool)
    first[:, 0] = True
    out["first"] = first
    last = np.zeros((n, nf), bool)
    last[:, nf - 1] = True
    out["last"] = last
    alt = np.zeros((n, nf), bool)
    alt[:, ::2] = True
    out["alternating"] = alt
    return out


PATTERNS = ["all", "none", "half0", "half1", "half2", "one_field", "first", "last", "alternating"]


def canaried(words: int, n: int, dev, fill=0xA5):
    """A mask buffer of words * n int64 between PAD canary words on both sides, prefilled."""
    host = np.full(words * n + 2 * PAD, np.uint64(int.from_bytes(bytes([fill]) * 8, "little")), np.uint64)
    host[:PAD] = CANARY
    host[PAD + words * n:] = CANARY
    return torch.from_numpy(host.view(np.int64)).to(dev)


def mask_of(buf: torch.Tensor, words: int, n: int) -> np.ndarray:
    """The mask rows of a canaried buffer (checks the canaries) -> uint64 [words, n]."""
    host = buf.cpu().numpy().view(np.uint64)
    assert (host[:PAD] == CANARY).all() and (host[PAD + words * n:] == CANARY).all(), "mask canary overwritten"
    return host[PAD:PAD + words * n].reshape(words, n)


def decode_present_abi(dev, schema, stream, ends, *, errors=False, frames=None):
    """spec_decode_flat_present (frames = None) or spec_decode_frames_present (frames = (r0, r1)) on
    buffers prefilled with 0xA5 -> (cols [np], status, present [words, rows], errmask or None); rows = n,
    or r1 for frames."""
    L = spec_amd.lib()
    n = len(ends)
    rows = n if frames is None else frames[1]
    words = words_of(schema)
    d_stream = to_dev(stream if stream.size else np.zeros(1, np.uint8), dev)[: stream.size]
    d_ends = to_dev(np.ascontiguousarray(ends, np.uint64).view(np.int64), dev)
    cols = [torch.full((n, w), 0xA5, dtype=torch.uint8, device=dev) for w in schema.widths]
    status = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    pm = canaried(words, rows, dev)
    em = canaried(words, rows, dev) if errors else None
    ptrs = (C.c_void_p * max(1, len(cols)))(*[c.data_ptr() for c in cols])
    pp = C.c_void_p(pm.data_ptr() + 8 * PAD)
    ep = C.c_void_p(em.data_ptr() + 8 * PAD) if errors else None
    if frames is None:
        rc = L.spec_decode_flat_present(C.byref(schema.c), C.c_void_p(d_stream.data_ptr()), stream.size,
                                        C.c_void_p(d_ends.data_ptr()), n, ptrs, C.c_void_p(status.data_ptr()), ep, pp,
                                        None)
    else:
        rc = L.spec_decode_frames_present(C.byref(schema.c), C.c_void_p(d_stream.data_ptr()), stream.size,
                                          C.c_void_p(d_ends.data_ptr()), frames[0], frames[1], 0, ptrs,
                                          C.c_void_p(status.data_ptr()), ep, pp, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ([c.cpu().numpy() for c in cols], status.cpu().numpy(), mask_of(pm, words, rows),
            mask_of(em, words, rows) if errors else None)


def _hex(stream, ends, i):
    s = int(ends[i - 1]) if i else 0
    return bytes(stream[s:int(ends[i])]).hex()


def check_present(dev, schema, recs, label="", errors=False):
    """spec_decode_flat_present over recs against the oracle: columns and status of decode_flat_batch,
    the HasField masks of the oracle Message, with errors the *Err bits of decode_flat_errors; every
    prefilled byte of the outputs replaced.  -> the expected masks uint64 [words, n]."""
    stream, ends = concat_records(recs)
    n = len(recs)
    want_cols, want_status = O.decode_flat_batch(schema.tags, schema.kinds, stream, ends, schema.widths)
    want_pm = oracle_present(schema, recs)
    cols, status, pm, em = decode_present_abi(dev, schema, stream, ends, errors=errors)
    assert np.array_equal(status, want_status), f"{label}: status"
    for f in range(len(schema)):
        if not np.array_equal(cols[f], want_cols[f]):
            i = int(np.nonzero((cols[f] != want_cols[f]).any(axis=1))[0][0])
            raise AssertionError(f"{label}: field {f} record {i}: gpu={cols[f][i].tobytes().hex()} "
                                 f"oracle={want_cols[f][i].tobytes().hex()} record={_hex(stream, ends, i)}")
    if not np.array_equal(pm, want_pm):
        c, i = (int(x) for x in np.argwhere(pm != want_pm)[0])
        raise AssertionError(f"{label}: present word {c} record {i}: gpu={int(pm[c, i]):x} oracle={int(want_pm[c, i]):x} "
                             f"status={want_status[i]} record={_hex(stream, ends, i)}")
    assert (want_pm[:, want_status != 0] == 0).all()  # a record that does not open: the empty Message
    if errors:
        want_em = O.decode_flat_errors(schema.tags, schema.kinds, stream, ends).reshape(words_of(schema), n)
        assert np.array_equal(em, want_em), f"{label}: errmask"
        assert not (em & ~want_pm).any(), f"{label}: an absent field errs"
    return want_pm


def random_columns(schema, n, seed, str_len=(0, 40)):
    return workload.gen_columns(schema, n, seed, str_len=str_len)


def encode_present_abi(dev, schema, cols, heaps, mask: np.ndarray, n, *, frames=False, phase=0, cap=None,
                       out_null=False, room=64):
    """spec_encode_flat_present[_frames] through the C ABI.  mask: uint64 [words, n].  out starts `phase`
    bytes into a buffer prefilled with 0xA5, `room` spare bytes behind the capacity `cap` (default: room
    for the oracle-sized output is the caller's business: cap bytes) -> (out bytes [cap] or None,
    before [phase], after [room], ends uint64 [n] (prefilled 0xA5...), total)."""
    L = spec_amd.lib()
    enc = spec_amd.Encoder(schema, n, dev)
    d_cols = [to_dev(c, dev) for c in cols]
    d_heaps = {f: to_dev(h if h.size else np.zeros(1, np.uint8), dev)[: h.size] for f, h in heaps.items()}
    hp, hl, _keep = enc._heapptrs(d_heaps)
    d_mask = to_dev(np.ascontiguousarray(mask, np.uint64).view(np.int64), dev)
    buf = torch.full((phase + (cap or 0) + room,), 0xA5, dtype=torch.uint8, device=dev)
    ends = torch.full((max(n, 1),), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)  # 0xA5A5...
    enc.total.fill_(-0x5A5A5A5A5A5A5A5B)
    fn = L.spec_encode_flat_present_frames if frames else L.spec_encode_flat_present
    rc = fn(C.byref(schema.c), enc._colptrs(d_cols), hp, hl, C.c_void_p(d_mask.data_ptr()), n,
            None if out_null else C.c_void_p(buf.data_ptr() + phase), cap or 0,
            None if out_null else C.c_void_p(ends.data_ptr()), C.c_void_p(enc.workspace.data_ptr()), enc.ws_bytes,
            C.c_void_p(enc.total.data_ptr()), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    total = int(enc.total.cpu().numpy().view(np.uint64)[0])
    return (host[phase:phase + (cap or 0)], host[:phase], host[phase + (cap or 0):],
            ends.cpu().numpy().view(np.uint64)[:n], total)


def oracle_sparse_stream(schema, cols, heaps, bits, n, frames=False):
    """The oracle Writer's sparse records as (stream, ends), or their mpx frames and frame ends."""
    recs = write_sparse(schema, cols, heaps, bits, n)
    stream, ends = concat_records(recs)
    if frames:
        return spec_amd.make_frames(stream, ends), ends + 4 * (np.arange(n, dtype=np.uint64) + 1)
    return stream, ends


def check_encode_present(dev, schema, cols, heaps, bits, n, label="", phase=0):
    """Unframed and framed device encodes of the masked batch against the oracle Writer's records, bit
    exact: stream, ends, *total, and nothing written outside out[0, total).  -> the oracle stream, ends."""
    mask = pack_mask(bits)
    res = None
    for frames in (False, True):
        want, want_ends = oracle_sparse_stream(schema, cols, heaps, bits, n, frames)
        out, before, after, ends, total = encode_present_abi(dev, schema, cols, heaps, mask, n, frames=frames,
                                                             phase=phase, cap=want.size)
        what = f"{label} {'frames' if frames else 'stream'}"
        assert total == want.size, f"{what}: total {total} oracle {want.size}"
        assert np.array_equal(ends, want_ends), f"{what}: ends"
        if not np.array_equal(out, want):
            j = int(np.nonzero(out != want)[0][0])
            i = int(np.searchsorted(want_ends, j, side="right"))
            s = int(want_ends[i - 1]) if i else 0
            raise AssertionError(f"{what}: byte {j} (record {i}) gpu={out[s:int(want_ends[i])].tobytes().hex()} "
                                 f"oracle={want[s:int(want_ends[i])].tobytes().hex()}")
        assert (before == 0xA5).all() and (after == 0xA5).all(), f"{what}: wrote outside out[0, total)"
        if not frames:
            res = (want, want_ends)
    return res

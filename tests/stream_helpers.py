"""Shared helpers of the stream and thread tests (tests/test_gpu_streams.py, tests/test_gpu_threads.py): the
decoy / stall / gate helper `run_case`, canary-guarded outputs, and the builders of every entry point's case -
its real batch, its decoy, the oracle's answers for both (computed once, on the host) and the calls."""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, NESTED, Kind, workload
from spec_amd import lz4 as LZ
from spec_amd.nested import NestedDecoder, NestedEncoder
from spec_amd.schema import VARLEN
from spec_amd.tree import INPUT_ROLES, ROLE_BEGIN, ROLE_VALUE, TreeDecoder, TreeEncoder
from tests.gpu_helpers import concat_records, require_specialised, to_dev
from tests.present_helpers import oracle_present, write_sparse
from tests.test_oracle_parse import _msg, _raw_message
from tests.tree_helpers import oracle_decode, oracle_encode, oracle_fields

# torch.cuda._sleep(cycles) on an MI355X, timed with a pair of events on a side stream: 0.55 ms for
# 1 M cycles, 4.18 ms for 10 M, 41.7 ms for 100 M (the host returns at once: the event behind it was
# pending every time).  240 M cycles: a stall of about 100 ms.  The gate assertion is the check,
# not this number.
STALL_CYCLES = 240_000_000
CANARY = 0xA5
PAD = 64  # canary bytes on either side of an output
SPAN_KINDS = (Kind.STRING, Kind.BYTES, Kind.ANY)
BM = 64 << 10  # LZ4 block size of the LZ4 cases (the smallest legal one: several blocks in a small batch)


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """A HIP error left behind by a test ends the session: nothing more is launched after it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU error after a stream or thread test: {e}", returncode=3)


# ---- helpers ---------------------------------------------------------------------------------------

def u8(a) -> np.ndarray:
    """Any array as its bytes (the unit of every comparison here)."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Guarded:
    """nbytes of device memory prefilled with a canary, between PAD canary bytes on both sides."""

    def __init__(self, nbytes: int, dev):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), CANARY, dtype=torch.uint8, device=dev)
        self.t = self.buf[PAD:PAD + self.n]

    def view(self, dtype, *shape):
        return self.t.view(dtype).view(*shape) if shape else self.t.view(dtype)

    def numpy(self) -> np.ndarray:
        h = self.buf.cpu().numpy()
        assert (h[:PAD] == CANARY).all() and (h[PAD + self.n:] == CANARY).all(), "canary around an output overwritten"
        return h[PAD:PAD + self.n]


def reverse_records(stream, ends):
    e = [0] + [int(x) for x in ends]
    recs = [bytes(stream[e[i]:e[i + 1]]) for i in range(len(ends))]
    return concat_records(recs[::-1])


def framed(stream, ends):
    ends = np.ascontiguousarray(ends, dtype=np.uint64).view(np.int64)
    return (spec_amd.make_frames(np.ascontiguousarray(stream, dtype=np.uint8), ends),
            ends + 4 * (np.arange(len(ends), dtype=np.int64) + 1))


def shifted(col, owner=None):
    """A span column over unframed records as the decode over their frames gives it: a non-empty span
    4 (k + 1) further on (k: the record that owns it), an empty one at 0."""
    w = np.ascontiguousarray(col).copy()
    wv = w.view(np.uint32).reshape(-1, 2)
    k = np.arange(len(wv), dtype=np.int64) if owner is None else np.asarray(owner, np.int64)
    wv[:, 0] = np.where(wv[:, 1] > 0, wv[:, 0] + 4 * (k + 1), 0).astype(np.uint32)
    return w


def stall(s):
    with torch.cuda.stream(s):
        torch.cuda._sleep(STALL_CYCLES)
    gate = torch.cuda.Event()
    gate.record(s)
    return gate


def copy_on(s, dst: dict, src: dict):
    with torch.cuda.stream(s):
        for k in dst:
            dst[k].copy_(src[k], non_blocking=True)


def compare(got: dict, want: dict, decoy: dict, label: str):
    assert set(got) >= set(want), (label, sorted(set(want) - set(got)))
    for k, w in want.items():
        g, w = u8(got[k]), u8(w)
        if g.shape == w.shape and np.array_equal(g, w):
            continue
        what = "a canary" if g.size and (g == CANARY).all() else "something else"
        if k in decoy and g.shape == u8(decoy[k]).shape and np.array_equal(g, u8(decoy[k])):
            what = "the DECOY's answer (inputs read outside the call's place in the stream)"
        j = int(np.nonzero(g != w)[0][0]) if g.shape == w.shape else -1
        raise AssertionError(f"{label}: output {k!r} differs from the oracle's answer at byte {j} "
                             f"of {w.size} (got {g.size} bytes); it holds {what}")


def run_case(dev, case):
    """The helper of this module's docstring over one Case:
      real, decoy   {name: numpy array}: E's device inputs, same shapes and dtypes
      want, want_decoy  {name: numpy array}: the oracle's outputs for each
      setup(dev) -> ctx                          state kept across calls (a tree decoder), optional
      prepare(I, dev, s, ctx) -> state           allocate outputs (canaries) and encoder objects over inputs I
      enqueue(state, s)                          E itself, cuda_stream = s
      collect(state) -> {name: numpy array}      after s.synchronize()
      gate          False: E waits on the host by contract, only the result is checked"""
    assert any(not np.array_equal(u8(case.want[k]), u8(case.want_decoy[k])) for k in case.want), \
        f"{case.name}: the oracle's outputs for the real batch and the decoy are the same"
    for k, v in case.real.items():
        assert v.shape == case.decoy[k].shape and v.dtype == case.decoy[k].dtype, (case.name, k)
    real = {k: to_dev(v, dev) for k, v in case.real.items()}
    decoy = {k: to_dev(v, dev) for k, v in case.decoy.items()}
    inputs = {k: v.clone() for k, v in decoy.items()}
    ctx = case.setup(dev) if getattr(case, "setup", None) else None
    s = torch.cuda.Stream()
    # once over the decoy: hiprtc compiles, module loads and buffer growth stay out of the gated region
    warm = case.prepare(inputs, dev, s, ctx)
    warm.warm = True
    torch.cuda.synchronize()
    case.enqueue(warm, s)
    s.synchronize()
    compare(case.collect(warm), case.want_decoy, {}, f"{case.name} (warm-up over the decoy)")
    state = case.prepare(inputs, dev, s, ctx)
    state.warm = False
    torch.cuda.synchronize()
    gate = stall(s)
    copy_on(s, inputs, real)
    assert torch.cuda.current_stream() != s
    case.enqueue(state, s)
    copy_on(s, inputs, decoy)
    pending = not gate.query()
    s.synchronize()
    compare(case.collect(state), case.want, case.want_decoy, case.name)
    if case.gate:
        assert pending, (f"{case.name}: the stall ahead of the call had ended when the call returned: the call "
                         f"waited on the host (or the stall is too short), so this run proves nothing")
    torch.cuda.synchronize()


def columns_out(schema, n, dev):
    g = [Guarded(n * w, dev) for w in schema.widths]
    return g, [x.view(torch.uint8, n, w) for x, w in zip(g, schema.widths)]


# ---- flat batches ----------------------------------------------------------------------------------

N_FLAT = 777


@functools.lru_cache(maxsize=None)
def flat_data(schema_name="flat16", n=N_FLAT, seed=31):
    """Sparse Flat16 records (about 60 % of the fields written) and everything the oracle says about them,
    for the batch (real) and for its reverse (decoy)."""
    schema = FLAT16
    cols, heaps = workload.gen_columns(schema, n, seed)
    bits = np.random.default_rng(seed).random((n, len(schema))) < 0.6
    recs = write_sparse(schema, cols, heaps, bits, n)
    out = {}
    for which, rs in (("real", recs), ("decoy", recs[::-1])):
        stream, ends = concat_records(rs)
        v = NS(schema=schema, n=n, stream=stream, ends=ends.view(np.int64), recs=rs)
        v.cols, v.status = O.decode_flat_batch(schema.tags, schema.kinds, stream, ends, schema.widths)
        v.err = O.decode_flat_errors(schema.tags, schema.kinds, stream, ends)
        v.present = oracle_present(schema, rs)[0]
        v.frames, v.fends = framed(stream, ends)
        v.fcols = [shifted(c) if f.kind in VARLEN else c for c, f in zip(v.cols, schema.fields)]
        # encode inputs: the decoded columns, every string / bytes span into the one heap `stream`
        heaps_in = {f: stream for f, fld in enumerate(schema.fields) if fld.kind in VARLEN}
        v.enc_stream, v.enc_ends = O.encode_flat_batch(schema.tags, schema.kinds, v.cols,
                                                        [heaps_in.get(f) for f in range(len(schema))], n)
        pbits = ((v.present[:, None] >> np.arange(len(schema), dtype=np.uint64)) & np.uint64(1)).astype(bool)
        v.penc_stream, v.penc_ends = concat_records(write_sparse(schema, v.cols, heaps_in, pbits, n))
        assert np.array_equal(v.penc_stream, stream)  # decode then encode the present fields: the records themselves
        out[which] = v
    return out["real"], out["decoy"]


def decode_want(v, frames=False, errors=False, present=False):
    w = {"status": v.status}
    w.update({f"col{f}": c for f, c in enumerate(v.fcols if frames else v.cols)})
    if errors:
        w["errmask"] = v.err
    if present:
        w["present"] = v.present
    return w


def flat_decode_case(entry, kernel):
    real, decoy = flat_data()
    schema, n = real.schema, real.n
    frames = "frames" in entry
    errors, present = entry.endswith("errors"), entry.endswith("present")
    if kernel == "jit":
        require_specialised(schema, "Flat16", decode=(real.frames.size if frames else real.stream.size, n))
    key = ("frames", "fends") if frames else ("stream", "ends")

    def prepare(I, dev, s, ctx):
        st = NS(I=I, g=None, res=None)
        if entry in ("decode_flat", "decode_frames"):
            st.g, st.cols = columns_out(schema, n, dev)
            st.gs = Guarded(n, dev)
        return st

    def enqueue(st, s):
        a, b = st.I[key[0]], st.I[key[1]]
        if entry == "decode_flat":
            st.res = (spec_amd.decode_flat(schema, a, b, cols=st.cols, status=st.gs.t, cuda_stream=s),)
        elif entry == "decode_frames":
            st.res = (spec_amd.decode_frames(schema, a, b, cols=st.cols, status=st.gs.t, cuda_stream=s),)
        elif entry == "decode_flat_errors":
            st.res = spec_amd.decode_flat_errors(schema, a, b, cuda_stream=s)
        elif entry == "decode_frames_errors":
            st.res = spec_amd.decode_frames_errors(schema, a, b, cuda_stream=s)
        elif entry == "decode_flat_present":
            st.res = spec_amd.decode_flat_present(schema, a, b, errors=True, cuda_stream=s)
        else:
            st.res = spec_amd.decode_frames_present(schema, a, b, errors=True, cuda_stream=s)

    def collect(st):
        got = {}
        if st.g is not None:
            got["status"] = st.gs.numpy()
            got.update({f"col{f}": g.numpy() for f, g in enumerate(st.g)})
            return got
        c = st.res[0]
        got["status"] = c.status.cpu().numpy()
        got.update({f"col{f}": t.cpu().numpy() for f, t in enumerate(c.cols)})
        if errors:
            got["errmask"] = st.res[1].cpu().numpy()
        if present:
            got["present"], got["errmask"] = st.res[1].cpu().numpy(), st.res[2].cpu().numpy()
        return got

    def ins(v):
        return {key[0]: getattr(v, key[0]), key[1]: getattr(v, key[1])}

    return NS(name=f"{entry}[{kernel}]", real=ins(real), decoy=ins(decoy), gate=True,
              want=decode_want(real, frames, errors or present, present),
              want_decoy=decode_want(decoy, frames, errors or present, present),
              prepare=prepare, enqueue=enqueue, collect=collect)


def flat_encode_inputs(v):
    d = {f"c{f}": c for f, c in enumerate(v.cols)}
    d["heap"] = v.stream
    d["present"] = v.present.view(np.int64)
    return d


def flat_encode_case(entry, kernel):
    """entry: into | frames_into | present_into | present_frames_into | size | size_present, or the
    size-then-allocate wrappers encode_flat | encode_flat_frames | encode_flat_present[_frames]."""
    real, decoy = flat_data()
    schema, n = real.schema, real.n
    if kernel == "jit":
        require_specialised(schema, "Flat16", encode=True)
    frames, pres, wrapper = "frames" in entry, "present" in entry, entry.startswith("encode_flat")
    real_in, decoy_in = flat_encode_inputs(real), flat_encode_inputs(decoy)
    if entry.startswith("size"):
        # the total of the same records in another order is the same total: this one case's decoy is
        # all-zero columns (a valid batch of the same shapes: zero values, empty strings, no field present)
        decoy_in = {k: np.zeros_like(a) for k, a in real_in.items()}
        decoy_in["heap"] = decoy.stream

    def want(v, inputs):
        if entry.startswith("size"):
            heaps = [inputs["heap"] if f.kind in VARLEN else None for f in schema.fields]
            cols = [inputs[f"c{f}"] for f in range(len(schema))]
            if pres:
                pb = ((inputs["present"].view(np.uint64)[:, None] >> np.arange(len(schema), dtype=np.uint64))
                      & np.uint64(1)).astype(bool)
                st, _ = concat_records(write_sparse(schema, cols, dict(enumerate(heaps)), pb, n))
            else:
                st, _ = O.encode_flat_batch(schema.tags, schema.kinds, cols, heaps, n)
            return {"total": np.array([st.size], np.int64)}
        st, en = (v.penc_stream, v.penc_ends) if pres else (v.enc_stream, v.enc_ends)
        if frames:
            st, en = framed(st, en)
        return {"out": st, "ends": np.asarray(en).view(np.int64), "total": np.array([st.size], np.int64)}

    w_real, w_decoy = want(real, real_in), want(decoy, decoy_in)
    total = int(w_real["total"][0])

    def prepare(I, dev, s, ctx):
        st = NS(I=I, cols=[I[f"c{f}"] for f in range(len(schema))],
                heaps={f: I["heap"] for f, fld in enumerate(schema.fields) if fld.kind in VARLEN})
        if not wrapper:
            st.enc = spec_amd.Encoder(schema, n, dev)
            st.enc.total.fill_(-7)
            st.out, st.ends = Guarded(total, dev), Guarded(8 * n, dev)
        return st

    def enqueue(st, s):
        if wrapper:
            if pres:
                st.res = spec_amd.encode_flat_present(schema, st.cols, st.heaps, st.I["present"], n, frames=frames,
                                                      cuda_stream=s)
            else:
                st.res = (spec_amd.encode_flat_frames if frames else spec_amd.encode_flat)(schema, st.cols, st.heaps, n,
                                                                                           cuda_stream=s)
            return
        e, out, ends = st.enc, st.out.t, st.ends.view(torch.int64)
        if entry == "size":
            e.size(st.cols, s)
        elif entry == "size_present":
            e.size_present(st.cols, st.heaps, st.I["present"], False, s)
        elif entry == "into":
            e.encode_into(st.cols, st.heaps, out, ends, s)
        elif entry == "frames_into":
            e.encode_frames_into(st.cols, st.heaps, out, ends, s)
        elif entry == "present_into":
            e.encode_present_into(st.cols, st.heaps, st.I["present"], out, ends, s)
        else:
            e.encode_present_frames_into(st.cols, st.heaps, st.I["present"], out, ends, s)

    def collect(st):
        if wrapper:
            return {"out": st.res[0].cpu().numpy(), "ends": st.res[1].cpu().numpy(),
                    "total": np.array([st.res[0].numel()], np.int64)}
        got = {"total": st.enc.total.cpu().numpy()}
        if not entry.startswith("size"):
            got.update(out=st.out.numpy(), ends=st.ends.numpy())
        return got

    return NS(name=f"{entry}[{kernel}]", real=real_in, decoy=decoy_in, want=w_real, want_decoy=w_decoy,
              gate=not wrapper, prepare=prepare, enqueue=enqueue, collect=collect)


# ---- nested batches --------------------------------------------------------------------------------

N_NESTED = 700


@functools.lru_cache(maxsize=None)
def nested_data(n=N_NESTED, seed=17):
    stream, ends = O.encode_nested_batch(workload.nested(n, seed=seed))
    out = []
    for st, en in ((stream, ends), reverse_records(stream, ends)):
        v = NS(n=n, stream=st, ends=np.asarray(en).view(np.int64))
        v.want = O.decode_nested_batch(st, en)
        v.m = int(v.want["item_begin"][-1])
        v.frames, v.fends = framed(st, en)
        v.owner = np.repeat(np.arange(n), v.want["counts"])
        # encode inputs: the decoded columns, both heaps the stream itself
        w = {k: v.want[k] for k in ("id", "seq", "name", "item_begin", "key", "value", "label")}
        w["name_heap"] = w["label_heap"] = st
        v.enc_in = w
        v.enc_stream, v.enc_ends = O.encode_nested_batch(w)
        out.append(v)
    assert out[0].m == out[1].m
    return out


def nested_want(v, frames):
    w = v.want
    d = {k: w[k] for k in ("status", "item_begin", "id", "seq", "key", "value", "item_status")}
    d["name"] = shifted(w["name"]) if frames else w["name"]
    d["label"] = shifted(w["label"], v.owner) if frames else w["label"]
    d["total"] = np.array([v.m], np.int64)
    return d


def nested_got(d, m):
    """d: a NestedDecoder (total on the device) or the NestedColumns a wrapper returned (total_items read back)."""
    o, it = d.outer, d.items
    total = d.total.cpu().numpy() if hasattr(d, "total") else np.array([d.total_items], np.int64)
    return {"status": d.status.cpu().numpy(), "item_begin": d.item_begin.cpu().numpy(), "id": o[0].cpu().numpy(),
            "seq": o[1].cpu().numpy(), "name": o[2].cpu().numpy(), "key": it[0][:m].cpu().numpy(),
            "value": it[1][:m].cpu().numpy(), "label": it[2][:m].cpu().numpy(),
            "item_status": d.item_status[:m].cpu().numpy(), "total": total}


def nested_decode_case(entry, kernel):
    """entry: twopass | onepass | frames_twopass | frames_onepass (NestedDecoder, asynchronous), or
    decode_nested | decode_nested_onepass | decode_nested_frames (the wrappers: they read the total)."""
    real, decoy = nested_data()
    frames, wrapper = "frames" in entry, entry.startswith("decode_nested")
    key = ("frames", "fends") if frames else ("stream", "ends")
    m = real.m

    def prepare(I, dev, s, ctx):
        st = NS(I=I)
        if not wrapper:
            d = st.d = NestedDecoder(NESTED, I[key[0]], I[key[1]], cuda_stream=s, head=4 if frames else 0)
            d.reserve(m + 64)  # (room past the batch's items: a misplaced item row stays inside the columns)
            d.workspace.zero_()  # (counts a misplaced scan would read: no items, not whatever the allocation held)
            for t in [d.status, d.item_begin, d.item_status, d.total] + d.items + [c for c in d.outer if c is not None]:
                t.view(torch.uint8).fill_(CANARY)
        return st

    def enqueue(st, s):
        a, b = st.I[key[0]], st.I[key[1]]
        if wrapper:
            st.res = spec_amd.decode_nested(NESTED, a, b, cuda_stream=s, onepass="onepass" in entry,
                                            item_cap=1 if "onepass" in entry else None, head=4 if frames else 0)
        elif "onepass" in entry:
            st.d.decode_onepass()
        else:
            st.d.index()
            st.d.decode()

    def collect(st):
        return nested_got(st.res if wrapper else st.d, m)

    def ins(v):
        return {key[0]: getattr(v, key[0]), key[1]: getattr(v, key[1])}

    return NS(name=f"nested {entry}[{kernel}]", real=ins(real), decoy=ins(decoy), want=nested_want(real, frames),
              want_decoy=nested_want(decoy, frames), gate=not wrapper, prepare=prepare, enqueue=enqueue,
              collect=collect)


def nested_encode_inputs(v):
    w = v.enc_in
    n, m = v.n, v.m
    return {"id": w["id"], "seq": u8(w["seq"]).reshape(n, 8), "name": u8(w["name"]).reshape(n, 8),
            "item_begin": w["item_begin"].view(np.int32), "key": u8(w["key"]).reshape(m, 4),
            "value": u8(w["value"]).reshape(m, 8), "label": u8(w["label"]).reshape(m, 8), "heap": v.stream}


def nested_encode_case(entry, kernel):
    """entry: encode | encode_frames (NestedEncoder, asynchronous) or the wrappers encode_nested[_frames]."""
    real, decoy = nested_data()
    n, m = real.n, real.m
    frames, wrapper = "frames" in entry, entry.startswith("encode_nested")

    def want(v):
        st, en = (v.enc_stream, v.enc_ends)
        if frames:
            st, en = framed(st, en)
        return {"out": st, "ends": np.asarray(en).view(np.int64), "total": np.array([st.size], np.int64)}

    total = int(want(real)["total"][0])

    def args(I):
        return ([I["id"], I["seq"], I["name"], None], {2: I["heap"]}, I["item_begin"], [I["key"], I["value"], I["label"]],
                {2: I["heap"]})

    def prepare(I, dev, s, ctx):
        st = NS(I=I)
        if not wrapper:
            st.enc = NestedEncoder(NESTED, n, dev)
            st.enc.total.fill_(-7)
            st.out, st.ends = Guarded(total, dev), Guarded(8 * n, dev)
        return st

    def enqueue(st, s):
        oc, oh, ib, ic, ih = args(st.I)
        if wrapper:
            st.res = (spec_amd.encode_nested_frames if frames else spec_amd.encode_nested)(NESTED, oc, oh, ib, ic, ih, n,
                                                                                           cuda_stream=s)
        else:
            (st.enc.encode_frames if frames else st.enc.encode)(oc, oh, ib, ic, ih, m, st.out.t,
                                                                st.ends.view(torch.int64), s)

    def collect(st):
        if wrapper:
            return {"out": st.res[0].cpu().numpy(), "ends": st.res[1].cpu().numpy(),
                    "total": np.array([st.res[0].numel()], np.int64)}
        return {"out": st.out.numpy(), "ends": st.ends.numpy(), "total": st.enc.total.cpu().numpy()}

    return NS(name=f"nested {entry}[{kernel}]", real=nested_encode_inputs(real), decoy=nested_encode_inputs(decoy),
              want=want(real), want_decoy=want(decoy), gate=not wrapper, prepare=prepare, enqueue=enqueue,
              collect=collect)


# ---- schema trees (and a nested schema with halves of more than 64 fields: encoded through the tree encoder
# with stream-ordered scratch, capi.hip nested_encode_wide) ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def tree_data(name="pkg1", n=300, seed=23):
    if name == "pkg1":
        tree = spec_amd.pkg1_tree()
        cols, heaps, _ = workload.tree_batch(tree, n, seed, count=(0, 3))
    else:
        from tests.test_gpu_nested import _wide_nested

        _, tree, list_at = _wide_nested()
        cols, heaps, _ = workload.tree_batch(tree, n, seed, count=(0, 4))
        cols[f"o{list_at}?"] = np.ones_like(cols[f"o{list_at}?"])  # a nested list is always written
    stream, ends = oracle_encode(tree, cols, heaps, n)
    out = []
    for st, en in ((stream, ends), reverse_records(stream, ends)):
        v = NS(tree=tree, n=n, stream=st, ends=np.asarray(en).view(np.int64))
        v.rows, v.want = oracle_decode(tree, st, en)
        v.frames, v.fends = framed(st, en)
        off = np.concatenate([[0], v.fends[:-1]]) + 4
        ln = np.maximum(v.fends - off, 0)
        spans = np.stack([np.where(ln > 0, off, 0), ln], 1).astype(np.uint32)
        v.spans = u8(spans).reshape(-1, 8)
        v.frows, v.fwant = O.decode_tree_spans(oracle_fields(tree), v.frames, spans)
        # encode inputs: the decoded columns, every span into the one heap `stream`
        v.enc_cols = {c.name: w for c, w in zip(tree.columns, v.want) if c.role in INPUT_ROLES}
        v.span_cols = [c.name for c in tree.columns if c.role == ROLE_VALUE and c.kind in SPAN_KINDS]
        v.enc_stream, v.enc_ends = oracle_encode(tree, v.enc_cols, {k: st for k in v.span_cols}, n)
        out.append(v)
    assert out[0].rows == out[1].rows and out[0].frows == out[0].rows
    return out


def tree_want(v, frames):
    d = {c.name: w for c, w in zip(v.tree.columns, v.fwant if frames else v.want)}
    d["rows_out"] = np.array(v.rows, np.int64)
    return d


def tree_columns_out(tree, rows, dev):
    g = [Guarded(max(tree.column_rows(c, rows), 1) * c.width, dev) for c in tree.columns]
    return g, [x.view(torch.uint8, -1, c.width) for x, c in zip(g, tree.columns)]


def tree_collect(tree, rows, g, rows_out):
    got = {c.name: x.numpy()[: tree.column_rows(c, rows) * c.width] for c, x in zip(tree.columns, g)}
    got["rows_out"] = rows_out.cpu().numpy()
    return got


def tree_decode_case(entry, kernel):
    """entry: run | run_frames (asynchronous once the decoder's buffers are grown), or decode_tree |
    decode_tree_frames | decode_tree_spans (index[_frames|_spans] + decode: the index pass returns host row
    counts; the spans are the frames' messages, so the answer is that of the frames)."""
    real, decoy = tree_data()
    tree, rows = real.tree, real.rows
    spans = entry.endswith("spans")
    frames, wrapper = "frames" in entry or spans, entry.startswith("decode_tree")
    key = ("frames", "spans") if spans else ("frames", "fends") if frames else ("stream", "ends")

    def setup(dev):
        d = TreeDecoder(tree)  # (looks its kernels up on its first pass: built under the leg's set_jit)
        d.reserve(rows)  # the warm-up run grows the rest: DevBuf::reserve frees and reallocates, which waits
        return d

    def prepare(I, dev, s, d):
        st = NS(I=I, d=d)
        if not wrapper:
            st.g, st.cols = tree_columns_out(tree, rows, dev)
            st.rows_out = torch.full((len(tree.tables),), -7, dtype=torch.int64, device=dev)
            st.caps = d.column_capacity(st.cols)
        return st

    def enqueue(st, s):
        a, b = st.I[key[0]], st.I[key[1]]
        if spans:
            d = TreeDecoder(tree)
            d.index_spans(a, b, s)
            st.res = d.decode(cuda_stream=s)
        elif wrapper:
            st.res = (spec_amd.tree.decode_tree_frames if frames else spec_amd.decode_tree)(tree, a, b, cuda_stream=s)
        else:
            (st.d.run_frames if frames else st.d.run)(a, b, st.cols, st.rows_out, s, st.caps)

    def collect(st):
        if wrapper:
            got = {c.name: t.cpu().numpy() for c, t in zip(tree.columns, st.res.cols)}
            got["rows_out"] = np.array(st.res.rows, np.int64)
            return got
        return tree_collect(tree, rows, st.g, st.rows_out)

    def ins(v):
        return {key[0]: getattr(v, key[0]), key[1]: getattr(v, key[1])}

    return NS(name=f"tree {entry}[{kernel}]", real=ins(real), decoy=ins(decoy), want=tree_want(real, frames),
              want_decoy=tree_want(decoy, frames), gate=not wrapper, setup=None if wrapper else setup, prepare=prepare,
              enqueue=enqueue, collect=collect)


def tree_encode_case(entry, kernel):
    """entry: encode | encode_frames (TreeEncoder, asynchronous) or the wrappers encode_tree[_frames]."""
    real, decoy = tree_data()
    tree, rows, n = real.tree, real.rows, real.n
    frames, wrapper = "frames" in entry, entry.startswith("encode_tree")

    def ins(v):
        d = dict(v.enc_cols)
        d["heap"] = v.stream
        return d

    def want(v):
        st, en = v.enc_stream, v.enc_ends
        if frames:
            st, en = framed(st, en)
        return {"out": st, "ends": np.asarray(en).view(np.int64), "total": np.array([st.size], np.int64)}

    total = int(want(real)["total"][0])
    real_in, decoy_in, want_real = ins(real), ins(decoy), want(real)
    if wrapper:
        # The wrappers are given rows=None: they read the table row counts back from the BEGIN columns
        # (tree_rows).  The reversed batch has the same counts, so here the REAL batch ends every BEGIN column one
        # owner row early (the last owner's list empty): a valid batch of the same shapes with fewer rows than
        # the decoy (row counts read from the decoy would name rows that no owner places, which the encoder
        # reports as an error; never more rows than the columns hold).
        real_in = dict(real_in)
        for c in tree.columns:
            if c.role == ROLE_BEGIN and len(real_in[c.name]) > 1:
                b = real_in[c.name].copy()
                b.view(np.uint32).reshape(-1)[-1] = b.view(np.uint32).reshape(-1)[-2]
                real_in[c.name] = b
        cols2 = {k: a for k, a in real_in.items() if k != "heap"}
        rows2 = spec_amd.tree_rows(tree, n, cols2)
        assert rows2 != rows and all(r2 <= r for r2, r in zip(rows2, rows))
        st2, en2 = oracle_encode(tree, cols2, {k: real.stream for k in real.span_cols}, n)
        if frames:
            st2, en2 = framed(st2, en2)
        want_real = {"out": st2, "ends": np.asarray(en2).view(np.int64), "total": np.array([st2.size], np.int64)}

    def prepare(I, dev, s, ctx):
        st = NS(cols={k: t for k, t in I.items() if k != "heap"}, heaps={k: I["heap"] for k in real.span_cols})
        if not wrapper:
            st.enc = TreeEncoder(tree, rows, dev)
            st.enc.total.fill_(-7)
            st.out, st.ends = Guarded(total, dev), Guarded(8 * n, dev)
        return st

    def enqueue(st, s):
        if wrapper:
            st.res = (spec_amd.encode_tree_frames if frames else spec_amd.encode_tree)(tree, st.cols, st.heaps, n,
                                                                                       cuda_stream=s)
        else:
            (st.enc.encode_frames if frames else st.enc.encode)(st.cols, st.heaps, st.out.t, st.ends.view(torch.int64), s)

    def collect(st):
        if wrapper:
            return {"out": st.res[0].cpu().numpy(), "ends": st.res[1].cpu().numpy(),
                    "total": np.array([st.res[0].numel()], np.int64)}
        return {"out": st.out.numpy(), "ends": st.ends.numpy(), "total": st.enc.total.cpu().numpy()}

    return NS(name=f"tree {entry}[{kernel}]", real=real_in, decoy=decoy_in, want=want_real, want_decoy=want(decoy),
              gate=not wrapper, prepare=prepare, enqueue=enqueue, collect=collect)


def wide_nested_encode_case(entry, kernel):
    """spec_encode_nested[_frames] over halves of 70 and 80 fields (hipMallocAsync scratch on the call's
    stream); the oracle is the tree oracle over the equivalent tree, as in tests/test_gpu_nested.py."""
    from tests.test_gpu_nested import _wide_nested

    schema, tree, list_at = _wide_nested()
    real, decoy = tree_data("wide_nested", 200, 29)
    n, m = real.n, real.rows[1]
    frames, wrapper = "frames" in entry, entry.startswith("encode_nested")
    lp = f"o{list_at}"
    okinds, ikinds = [f.kind for f in schema.outer.fields], [f.kind for f in schema.item.fields]

    def ins(v):
        d = {f"o{i}": v.enc_cols[f"o{i}"] for i, k in enumerate(okinds) if k != Kind.LIST}
        d.update({f"w{j}": v.enc_cols[f"{lp}[].w{j}"] for j in range(len(ikinds))})
        d["item_begin"] = u8(v.enc_cols[f"{lp}#begin"]).view(np.int32)
        d["heap"] = v.stream
        return d

    def want(v):
        st, en = v.enc_stream, v.enc_ends
        if frames:
            st, en = framed(st, en)
        return {"out": st, "ends": np.asarray(en).view(np.int64), "total": np.array([st.size], np.int64)}

    total = int(want(real)["total"][0])

    def prepare(I, dev, s, ctx):
        st = NS(I=I)
        if not wrapper:
            st.enc = NestedEncoder(schema, n, dev)
            st.enc.total.fill_(-7)
            st.out, st.ends = Guarded(total, dev), Guarded(8 * n, dev)
        return st

    def enqueue(st, s):
        I = st.I
        oc = [None if k == Kind.LIST else I[f"o{i}"] for i, k in enumerate(okinds)]
        oh = {i: I["heap"] for i, k in enumerate(okinds) if k in VARLEN}
        ic = [I[f"w{j}"] for j in range(len(ikinds))]
        ih = {j: I["heap"] for j, k in enumerate(ikinds) if k in VARLEN}
        if wrapper:
            st.res = (spec_amd.encode_nested_frames if frames else spec_amd.encode_nested)(
                schema, oc, oh, I["item_begin"], ic, ih, n, cuda_stream=s)
        else:
            (st.enc.encode_frames if frames else st.enc.encode)(oc, oh, I["item_begin"], ic, ih, m, st.out.t,
                                                                st.ends.view(torch.int64), s)

    def collect(st):
        if wrapper:
            return {"out": st.res[0].cpu().numpy(), "ends": st.res[1].cpu().numpy(),
                    "total": np.array([st.res[0].numel()], np.int64)}
        return {"out": st.out.numpy(), "ends": st.ends.numpy(), "total": st.enc.total.cpu().numpy()}

    return NS(name=f"wide nested {entry}[{kernel}]", real=ins(real), decoy=ins(decoy), want=want(real),
              want_decoy=want(decoy), gate=not wrapper, prepare=prepare, enqueue=enqueue, collect=collect)


def decode_values_case(entry, kernel):
    rng = np.random.default_rng(5)
    vals = [O.encode("int64", int(x))[0] for x in rng.integers(-2**60, 2**60, 1000)]
    vals = [v[: len(v) - (i % 97 == 0)] for i, v in enumerate(vals)]  # a few truncated ones: decoder errors
    out = []
    for vs in (vals, vals[::-1]):
        stream, ends = concat_records(vs)
        starts = np.concatenate([[0], ends[:-1]]).astype(np.uint32)
        spans = np.stack([starts, (ends - starts).astype(np.uint32)], 1).astype(np.uint32)
        wv, we = O.decode_values(int(Kind.INT64), stream, spans)
        out.append((dict(stream=stream, spans=u8(spans).reshape(-1, 8)), dict(values=wv, err=we)))

    def enqueue(st, s):
        st.res = spec_amd.decode_values(Kind.INT64, st.I["stream"], st.I["spans"], cuda_stream=s)

    return NS(name="decode_values", real=out[0][0], decoy=out[1][0], want=out[0][1], want_decoy=out[1][1], gate=True,
              prepare=lambda I, dev, s, ctx: NS(I=I), enqueue=enqueue,
              collect=lambda st: {"values": st.res[0].cpu().numpy(), "err": st.res[1].cpu().numpy()})


# ---- frames, LZ4, validation -----------------------------------------------------------------------------

def frames_case(entry, kernel):
    """entry: write_frames | frames_index_device_c (the C call: asynchronous) | frames_index_device (the wrapper
    reads count, consumed and status back)."""
    real, decoy = flat_data()
    n = real.n
    L = spec_amd.lib()
    if entry == "write_frames":
        def prepare(I, dev, s, ctx):
            return NS(I=I, out=Guarded(real.frames.size, dev))

        def enqueue(st, s):
            st.res = spec_amd.write_frames(st.I["stream"], st.I["ends"], out=st.out.t, cuda_stream=s)

        return NS(name=entry, real=dict(stream=real.stream, ends=real.ends), decoy=dict(stream=decoy.stream, ends=decoy.ends),
                  want=dict(frames=real.frames, fends=real.fends), want_decoy=dict(frames=decoy.frames, fends=decoy.fends),
                  gate=True, prepare=prepare, enqueue=enqueue,
                  collect=lambda st: {"frames": st.out.numpy(), "fends": st.res[1].cpu().numpy()})
    cap = n + 8

    def want(v):
        return {"ends": v.fends, "scalars": np.array([n, v.frames.size, 0], np.int64)}

    def prepare(I, dev, s, ctx):
        wsb = L.spec_frames_index_device_workspace_size(real.frames.size)
        return NS(I=I, ends=Guarded(8 * cap, dev), out=torch.zeros(3, dtype=torch.int64, device=dev), wsb=wsb,
                  ws=torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev))

    def enqueue(st, s):
        if entry == "frames_index_device":
            st.res = spec_amd.frames_index_device(st.I["frames"], cap, cuda_stream=s)
            return
        p = st.out.data_ptr()
        rc = L.spec_frames_index_device(C.c_void_p(st.I["frames"].data_ptr()), st.I["frames"].numel(),
                                        C.c_void_p(st.ends.t.data_ptr()), cap, C.c_void_p(p), C.c_void_p(p + 8),
                                        C.c_void_p(p + 16), C.c_void_p(st.ws.data_ptr()), st.wsb, C.c_void_p(s.cuda_stream))
        assert rc == 0, rc

    def collect(st):
        if entry == "frames_index_device":
            e, used, status = st.res
            return {"ends": e.cpu().numpy(), "scalars": np.array([e.numel(), used, status], np.int64)}
        return {"ends": st.ends.numpy()[: 8 * n], "scalars": st.out.cpu().numpy()}

    return NS(name=entry, real=dict(frames=real.frames), decoy=dict(frames=decoy.frames), want=want(real),
              want_decoy=want(decoy), gate=entry != "frames_index_device", prepare=prepare, enqueue=enqueue,
              collect=collect)


@functools.lru_cache(maxsize=None)
def lz4_data():
    """About 350 KB of mpx frames (six 64 KiB blocks) and their reverse, each as an LZ4 frame of the oracle's
    writer, the compressed bytes padded to one length so that both are inputs of the same size."""
    n = 1400
    cols, heaps = workload.flat16(n, seed=12)
    stream, ends = O.encode_flat_batch(FLAT16.tags, FLAT16.kinds, cols, [heaps.get(f) for f in range(16)], n)
    out = []
    for st, en in ((stream, ends), reverse_records(stream, ends)):
        v = NS(data=framed(st, en)[0])
        v.frame = O.lz4_frame_write(v.data, None, BM, content_checksum=False, close=True)
        v.blocks, used, bmax, rc = LZ.frame_blocks(v.frame)
        assert rc == 0 and bmax == BM and used == v.frame.size
        v.digest = O.xxh32(v.data)
        out.append(v)
    size = max(v.frame.size for v in out) + 64
    for v in out:
        v.src = np.zeros(size, np.uint8)
        v.src[: v.frame.size] = v.frame
        nb = len(v.blocks)
        v.sizes = np.array([min(BM, v.data.size - i * BM) for i in range(nb)], np.int32)
        v.slots = np.zeros(nb * BM, np.uint8)
        v.slots[: v.data.size] = v.data  # (block i of BM bytes sits in slot i of BM bytes)
    assert len(out[0].blocks) == len(out[1].blocks) > 3
    return out


def lz4_case(entry, kernel):
    """entry: decompress_c | pack | content | compress_into (the C calls: asynchronous) or the wrappers
    decompress | compress_frame | digest (they read a total or the digest back)."""
    real, decoy = lz4_data()
    L = spec_amd.lib()
    nb, n = len(real.blocks), real.data.size
    vp = C.c_void_p

    def block_bytes(slots, sizes):
        return np.concatenate([slots[i * BM: i * BM + int(z)] for i, z in enumerate(sizes)])

    if entry in ("decompress_c", "decompress"):
        def ins(v):
            return dict(src=v.src, blocks=u8(v.blocks))

        def want(v):
            d = dict(data=v.data, sizes=v.sizes, status=np.zeros(nb, np.uint8))
            return d

        def prepare(I, dev, s, ctx):
            return NS(I=I, slots=Guarded(nb * BM, dev), sizes=Guarded(4 * nb, dev), status=Guarded(nb, dev))

        def enqueue(st, s):
            if entry == "decompress":  # the block table is a host argument of the wrapper: that of the bytes it reads
                st.res = LZ.decompress(st.I["src"], (decoy if st.warm else real).blocks, BM, cuda_stream=s)
                return
            rc = L.spec_lz4_decompress(vp(st.I["src"].data_ptr()), st.I["src"].numel(), vp(st.I["blocks"].data_ptr()), nb,
                                       vp(st.slots.t.data_ptr()), BM, vp(st.sizes.t.data_ptr()), vp(st.status.t.data_ptr()),
                                       vp(s.cuda_stream))
            assert rc == 0, rc

        def collect(st):
            if entry == "decompress":
                o, z, t = st.res
                return dict(data=o.cpu().numpy(), sizes=z.cpu().numpy(), status=t.cpu().numpy())
            z = st.sizes.numpy().view(np.int32)
            ok = np.array_equal(z, real.sizes) or np.array_equal(z, decoy.sizes)
            return dict(data=block_bytes(st.slots.numpy(), z) if ok else np.zeros(0, np.uint8), sizes=z,
                        status=st.status.numpy())
    elif entry == "pack":
        def ins(v):
            return dict(slots=v.slots, sizes=v.sizes)

        def want(v):
            return dict(data=v.data, total=np.array([n], np.int64))

        def prepare(I, dev, s, ctx):
            wsb = L.spec_lz4_pack_workspace_size(nb)
            return NS(I=I, out=Guarded(nb * BM, dev), total=torch.full((1,), -7, dtype=torch.int64, device=dev), wsb=wsb,
                      ws=torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev))

        def enqueue(st, s):
            rc = L.spec_lz4_pack(vp(st.I["slots"].data_ptr()), BM, vp(st.I["sizes"].data_ptr()), nb, vp(st.out.t.data_ptr()),
                                 nb * BM, vp(st.total.data_ptr()), vp(st.ws.data_ptr()), st.wsb, vp(s.cuda_stream))
            assert rc == 0, rc

        def collect(st):
            return dict(data=st.out.numpy()[:n], total=st.total.cpu().numpy())
    elif entry in ("content", "digest"):
        def ins(v):
            return dict(data=v.data)

        def want(v):
            return dict(digest=np.array([v.digest], np.uint32))

        def prepare(I, dev, s, ctx):
            return NS(I=I, cc=LZ.ContentChecksum(dev))

        def enqueue(st, s):
            half = n // 2 + 3  # two updates: the state carries 16 buffered bytes across calls
            st.cc.update(st.I["data"][:half], s)
            st.cc.update(st.I["data"][half:], s)
            if entry == "digest":
                st.res = st.cc.digest(s)
            else:
                st.cc.digest_device(s)

        def collect(st):
            return dict(digest=np.array([st.res], np.uint32) if entry == "digest" else st.cc.out.cpu().numpy())
    else:
        flags = LZ.OPEN | LZ.CLOSE

        def ins(v):
            return dict(data=v.data)

        def want(v):
            return dict(decompressed=v.data)

        def prepare(I, dev, s, ctx):
            wsb = L.spec_lz4_compress_workspace_size(n, BM)
            return NS(I=I, out=Guarded(LZ.frame_bound(n, BM, flags), dev), ws=torch.empty(max(wsb, 16), dtype=torch.uint8,
                                                                                           device=dev),
                      total=torch.full((1,), -7, dtype=torch.int64, device=dev))

        def enqueue(st, s):
            if entry == "compress_frame":
                st.res = LZ.compress_frame(st.I["data"], BM, open=True, close=True, cuda_stream=s)
            else:
                LZ.compress_frame_into(st.I["data"], st.out.t, st.total, BM, flags, None, workspace=st.ws, cuda_stream=s)

        def collect(st):
            # (the compressor's choice of matches is its own: what it wrote is read back by the oracle's reader)
            if entry == "compress_frame":
                f = st.res.cpu().numpy()
            else:
                t = int(st.total.item())
                assert 0 < t <= st.out.n, t
                f = st.out.numpy()[:t]
            rc, got, used = O.lz4_frame_read(f, n + 16)
            assert rc == 0 and used == f.size, (rc, used, f.size)
            return dict(decompressed=got)

    return NS(name=f"lz4 {entry}", real=ins(real), decoy=ins(decoy), want=want(real), want_decoy=want(decoy),
              gate=entry in ("decompress_c", "pack", "content", "compress_into"), prepare=prepare, enqueue=enqueue,
              collect=collect)


def parse_case(entry, kernel):
    """parse_messages over flat records with a few nested deeper than 32 among them: the deep pass and its
    stream-ordered scratch (validate.hip launch_parse) run."""
    def nest(d, inner=None):
        b = inner if inner is not None else _msg([(1, "int32", 7)])
        for _ in range(d):
            b = _raw_message([b])
        return b

    recs = list(flat_data()[0].recs[:600])
    bad = _raw_message([bytes([1, 2, 3, 99])])
    for k, r in enumerate([nest(40), nest(500), nest(40, bad), nest(33), nest(3), nest(40, bad)]):
        recs.insert(50 + 90 * k, r)
    out = []
    for rs in (recs, recs[::-1]):
        stream, ends = concat_records(rs)
        st, sz = O.parse_batch(stream, ends)
        out.append((dict(stream=stream, ends=ends.view(np.int64)), dict(status=st, sizes=sz)))
    assert (out[0][1]["status"] != 0).any()

    def enqueue(st, s):
        st.res = spec_amd.parse_messages(st.I["stream"], st.I["ends"], cuda_stream=s)

    return NS(name="parse_messages", real=out[0][0], decoy=out[1][0], want=out[0][1], want_decoy=out[1][1], gate=True,
              prepare=lambda I, dev, s, ctx: NS(I=I), enqueue=enqueue,
              collect=lambda st: {"status": st.res[0].cpu().numpy(), "sizes": st.res[1].cpu().numpy()})


ALL_KINDS = [Kind(k) for k in range(1, 16)]

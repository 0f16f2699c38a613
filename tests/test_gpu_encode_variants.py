"""The flat encoder's whole dispatch matrix through the C ABI against the oracle Writer's bytes:
{schema-specialised kernels on, off} x {5 fields, 65 fields (the wide kernels)} x {dense, present
all ones, present alternating bits} x {plain, mpx frames}, every cell at n = 1, 63, 64, 65 (one lane,
the wave boundary from both sides) and 257 (two encode blocks: the scan's offsets count).  Every
cell is one instantiation of encode_size_kernel / encode_scan_kernel / encode_write_kernel
(spec_amd/csrc/encode_flat.hip) or, for the dense 5-field schema with the specialised kernels on,
the schema's hiprtc module.  Each schema has one string field, so heaps are attached."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import spec_amd
from spec_amd import Kind, Schema
from spec_amd.schema import VARLEN
from tests.gpu_helpers import concat_records, oracle_encode, require_specialised, to_dev
from tests.present_helpers import encode_present_abi, pack_mask, patterns, random_columns, write_sparse
from tests.shape_helpers import split_records
from tests.test_gpu_flat import ALL_KINDS

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 257]
SPARE = 32  # bytes of capacity past the oracle's total: the encoder must leave them alone
FIXED = [k for k in ALL_KINDS if k not in VARLEN]
# write order differs from tag order in both; the string sits at an even index, so the
# alternating pattern (fields 0, 2, 4, ...) writes it
NARROW = Schema([(3, Kind.INT32), (1, Kind.BOOL), (4, Kind.STRING), (2, Kind.UINT64), (5, Kind.FLOAT64)])
# (65 fields: every eighth of another fixed-width kind, the rest BOOL, so a wave of the alternating
# batch fits the write pass's LDS slab and a wave of the dense one may not: both ways out)
WIDE = Schema([(int(t), Kind.STRING if i == 8 else FIXED[i // 8 * 2 % len(FIXED)] if i % 8 == 0 else Kind.BOOL)
               for i, t in enumerate(np.random.default_rng(65).permutation(np.arange(1, 66)))])
SCHEMAS = {"narrow5": NARROW, "wide65": WIDE}


@pytest.fixture(params=["jit", "generic"])
def kernel(request):
    """Run a test with the schema-specialised kernels (hiprtc) on and off."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


@functools.lru_cache(maxsize=None)
def columns(width: str, n: int):
    return random_columns(SCHEMAS[width], n, 7 * n + len(width), str_len=(0, 40))


@functools.lru_cache(maxsize=None)
def reference(width: str, mode: str, n: int):
    """The oracle Writer's records of the cell's batch -> (stream, ends, frames, frame ends); computed
    once and shared by the kernel and framing legs, which only read it."""
    schema = SCHEMAS[width]
    cols, heaps = columns(width, n)
    if mode == "alternating":
        stream, ends = concat_records(write_sparse(schema, cols, heaps, bits_of(width, mode, n), n))
    else:  # every field written: the dense batch
        stream, ends = oracle_encode(schema, cols, heaps, n)
    ends = np.ascontiguousarray(ends).view(np.uint64)
    assert len(split_records(stream, ends)) == n and int(ends[-1]) == stream.size
    frames = spec_amd.make_frames(stream, ends)
    out = (stream, ends, frames, ends + 4 * (np.arange(n, dtype=np.uint64) + 1))
    for a in out:
        a.setflags(write=False)
    return out


def bits_of(width: str, mode: str, n: int) -> np.ndarray:
    return patterns(len(SCHEMAS[width]), n)["alternating" if mode == "alternating" else "all"]


def encode_dense_abi(dev, schema, cols, heaps, n, *, frames, cap, room=64):
    """spec_encode_flat[_frames] and spec_encode_flat_size through the C ABI, out and ends prefilled
    with 0xA5 -> (out bytes [cap], after [room], ends uint64 [n], total, the size-only total)."""
    L = spec_amd.lib()
    enc = spec_amd.Encoder(schema, n, dev)
    d_cols = [to_dev(c, dev) for c in cols]
    d_heaps = {f: to_dev(h if h.size else np.zeros(1, np.uint8), dev)[: h.size] for f, h in heaps.items()}
    hp, hl, _keep = enc._heapptrs(d_heaps)
    buf = torch.full((cap + room,), 0xA5, dtype=torch.uint8, device=dev)
    ends = torch.full((n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)  # 0xA5A5...
    enc.total.fill_(-0x5A5A5A5A5A5A5A5B)
    fn = L.spec_encode_flat_frames if frames else L.spec_encode_flat
    rc = fn(C.byref(schema.c), enc._colptrs(d_cols), hp, hl, n, C.c_void_p(buf.data_ptr()), cap,
            C.c_void_p(ends.data_ptr()), C.c_void_p(enc.workspace.data_ptr()), enc.ws_bytes,
            C.c_void_p(enc.total.data_ptr()), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    total = int(enc.total.cpu().numpy().view(np.uint64)[0])
    enc.total.fill_(-0x5A5A5A5A5A5A5A5B)
    rc = L.spec_encode_flat_size(C.byref(schema.c), enc._colptrs(d_cols), n, C.c_void_p(enc.workspace.data_ptr()),
                                 enc.ws_bytes, C.c_void_p(enc.total.data_ptr()), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    size = int(enc.total.cpu().numpy().view(np.uint64)[0])
    host = buf.cpu().numpy()
    return host[:cap], host[cap:], ends.cpu().numpy().view(np.uint64), total, size


@pytest.mark.parametrize("framed", [False, True], ids=["plain", "framed"])
@pytest.mark.parametrize("mode", ["dense", "ones", "alternating"])
@pytest.mark.parametrize("width", ["narrow5", "wide65"])
def test_cell(dev, kernel, width, mode, framed):
    schema = SCHEMAS[width]
    if kernel == "jit" and width == "narrow5":  # (no wider schema has specialised encode kernels)
        require_specialised(schema, width, encode=True)
    for n in NS:
        what = f"{kernel} {width} {mode} {'framed' if framed else 'plain'} n={n}"
        cols, heaps = columns(width, n)
        stream, ends, frames, fends = reference(width, mode, n)
        want, want_ends = (frames, fends) if framed else (stream, ends)
        cap = want.size + SPARE
        dense = None
        if mode != "alternating":
            dense = encode_dense_abi(dev, schema, cols, heaps, n, frames=framed, cap=cap)
        if mode == "dense":
            out, after, got_ends, total, size = dense
            # spec_encode_flat_size sizes the messages; a framed call adds the n four-byte heads
            size += 4 * n if framed else 0
        else:
            mask = pack_mask(bits_of(width, mode, n))
            out, _, after, got_ends, total = encode_present_abi(dev, schema, cols, heaps, mask, n, frames=framed,
                                                                cap=cap)
            size = encode_present_abi(dev, schema, cols, heaps, mask, n, frames=framed, out_null=True)[4]
        assert total == want.size, f"{what}: total {total} oracle {want.size}"
        assert size == total, f"{what}: size-only total {size}, full call {total}"
        assert np.array_equal(got_ends, want_ends), f"{what}: ends"
        if not np.array_equal(out[:total], want):
            j = int(np.nonzero(out[:total] != want)[0][0])
            i = int(np.searchsorted(want_ends, j, side="right"))
            s = int(want_ends[i - 1]) if i else 0
            raise AssertionError(f"{what}: byte {j} (record {i}) gpu={out[s:int(want_ends[i])].tobytes().hex()} "
                                 f"oracle={want[s:int(want_ends[i])].tobytes().hex()}")
        assert out[total] == 0xA5, f"{what}: the byte after total was written"
        assert (out[total:] == 0xA5).all() and (after == 0xA5).all(), f"{what}: wrote past out[total)"
        if mode == "ones":  # every field present: the dense encoder's bytes, on the device too
            assert np.array_equal(out, dense[0]) and np.array_equal(got_ends, dense[2]) and total == dense[3], \
                f"{what}: differs from the dense call"

"""GPU parity of the framed tree encoder (spec_encode_tree_frames): for the same columns its bytes
are spec_amd.make_frames over the oracle's records (oracle/tree.c), its ends the oracle's ends plus
4(k + 1), and both equal spec_frames_write over spec_encode_tree on the device — through the
generated writers (the record-tile writer, the level-fused writer) and the run-time row kernels; at
every output byte phase with canaries on both sides (record 0's head is the first thing a write
below frames[0] would damage), with tiles that outgrow the LDS image, at capacity and on an encoder
error; and the receive side decodes what it wrote."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import spec_amd
from spec_amd import Kind
from spec_amd.tree import ROLE_VALUE, TreeDecoder, TreeEncoder
from tests.test_gpu_tree import to_dev
from tests.test_gpu_tree_runtime import CANARY, PHASES, Canaried, batch
from tests.tree_helpers import span_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["jit", "runtime"])
def kernel(request):
    """Run a test with the generated tree kernels (hiprtc) and with the run-time tree kernels."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """A HIP error left behind by a test ends the session: nothing more is launched after it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU error after a framed tree encode test: {e}", returncode=3)


def expected(b):
    """(frames, frame ends) of the shared batch b: make_frames over the oracle's stream."""
    frames = spec_amd.make_frames(b.stream, b.ends)
    fends = b.ends.view(np.int64) + 4 * (np.arange(b.n, dtype=np.int64) + 1)
    return frames, fends


def assert_frames(got, gends, want, wends, label):
    if not np.array_equal(gends, wends):
        i = int(np.nonzero(gends != wends)[0][0])
        raise AssertionError(f"{label}: frame_ends[{i}] gpu={gends[i]} want={wends[i]}")
    if not np.array_equal(got, want):
        j = int(np.nonzero(got != want)[0][0])
        i = int(np.searchsorted(wends, j, side="right"))
        s = int(wends[i - 1]) if i else 0
        raise AssertionError(f"{label}: byte {j} (frame {i}, +{j - s}) gpu={got[j]:#x} want={want[j]:#x}")


def check_frames(b, dev, label, phases=(0,)):
    """spec_encode_tree_frames into canaried buffers at the byte phases given: the oracle's frames
    and ends, *total right, canaries intact, and equal to write_frames(encode_tree) on the device."""
    want, wends = expected(b)
    d_cols, d_heaps = to_dev(b.cols, dev), to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    enc.total.fill_(-7)
    assert int(enc.encode_frames(d_cols, d_heaps, None, None).item()) == want.size, f"{label}: size only"
    two, two_ends = spec_amd.write_frames(*spec_amd.encode_tree(b.tree, d_cols, d_heaps, b.n, rows=b.rows))
    c = None
    for phase in phases:
        c = Canaried(dev, want.size, b.n, phase)
        enc.total.fill_(-7)
        enc.encode_frames(d_cols, d_heaps, c.out, c.ends)
        torch.cuda.synchronize()
        assert int(enc.total.item()) == want.size, f"{label} phase {phase}: *total"
        assert_frames(c.out.cpu().numpy(), c.ends.cpu().numpy(), want, wends, f"{label} phase {phase}")
        c.assert_outside_intact(f"{label} phase {phase}")
        assert torch.equal(c.out, two), f"{label} phase {phase}: differs from write_frames(encode_tree)"
        assert torch.equal(c.ends, two_ends), f"{label} phase {phase}: ends differ from write_frames(encode_tree)"
    return c.out.clone(), c.ends.clone()


# ---- 1. parity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_pkg1_frames(dev, kernel, n):
    """pkg1 at the wave and 64-record tile boundaries (300: five tiles, a ragged last one)."""
    check_frames(batch(f"pkg1_n{n}"), dev, f"pkg1 {kernel} n={n}")


def test_pkg1_tiles_over_image_frames(dev, kernel):
    """200 records with strings of up to 3,000 bytes: tiles that outgrow the record-tile writer's
    LDS image, their bytes past it (heads included) stored straight to memory."""
    b = batch("pkg1_tiles_over_image")
    starts = np.concatenate([[0], b.ends[:-1]]).astype(np.int64)
    assert max(int(b.ends[min(b.n, t + 64) - 1]) - int(starts[t]) for t in range(0, b.n, 64)) > 72 * 1024
    check_frames(b, dev, f"tiles over image {kernel}", phases=(0, 3))


@pytest.mark.parametrize("name", ["shapes_lists", "nested_n300", "wide_n65", "many_tables_n300", "spec_pkg1.Message"])
def test_other_trees_frames(dev, kernel, name):
    """Big lists by count, structs in structs, a root of more than 64 direct fields (the
    level-fused writer's BEmit16), many tables, and the .spec file's pkg1.Message."""
    check_frames(batch(name), dev, f"{name} {kernel}")


# ---- 2. byte phases and bounds -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pkg1_n65", "pkg1_n300", "wide_n65"])
def test_frames_byte_phases(dev, kernel, name):
    """`frames` at five byte phases of a 16-byte chunk, canaries in front (at least 64 bytes) and
    behind: nothing outside frames[0, total) or frame_ends[0, n) is written."""
    check_frames(batch(name), dev, f"{name} {kernel}", phases=PHASES)


# ---- 3. capacity, errors, size only ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["pkg1_n300", "shapes_lists"])
def test_frames_capacity_one_short(dev, kernel, name):
    b = batch(name)
    total = b.stream.size + 4 * b.n
    d_cols, d_heaps = to_dev(b.cols, dev), to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    for phase in (0, 3):
        c = Canaried(dev, total - 1, b.n, phase)
        enc.total.fill_(-7)
        enc.encode_frames(d_cols, d_heaps, c.out, c.ends)
        torch.cuda.synchronize()
        assert int(enc.total.item()) == total
        c.assert_untouched(f"{name} {kernel} phase {phase}")


@pytest.mark.parametrize("col", ["string", "strings[]"])
def test_frames_span_outside_heap(dev, kernel, col):
    """A span one past its heap's end, in a record column and in a list-item column: *total
    all-ones, nothing written; the same encoder then writes the frames from the good columns."""
    b = batch("pkg1_n300")
    want, wends = expected(b)
    tc = b.tree.column(col)
    assert tc.kind in (Kind.STRING, Kind.BYTES, Kind.ANY)
    sp = b.cols[col].copy().view(np.uint32).reshape(-1, 2)
    row = int(np.argmax(sp[:, 1] > 0))
    sp[row, 0] = b.heaps[col].size + 1
    bad = dict(b.cols)
    bad[col] = sp.view(np.uint8).reshape(-1, 8)
    d_heaps = to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    c = Canaried(dev, want.size, b.n, 1)
    enc.total.fill_(-7)
    enc.encode_frames(to_dev(bad, dev), d_heaps, c.out, c.ends)
    torch.cuda.synchronize()
    assert int(enc.total.item()) == -1  # all-ones as int64
    c.assert_untouched(f"{kernel} {col}")
    enc.total.fill_(-7)
    enc.encode_frames(to_dev(b.cols, dev), d_heaps, c.out, c.ends)
    torch.cuda.synchronize()
    assert int(enc.total.item()) == want.size
    assert_frames(c.out.cpu().numpy(), c.ends.cpu().numpy(), want, wends, f"{kernel} after the error")
    c.assert_outside_intact(f"{kernel} after the error")


@pytest.mark.parametrize("name", ["pkg1_n1", "pkg1_n300", "shapes_lists"])
def test_frames_size_only(dev, kernel, name):
    """frames = None: *total = the unframed total + 4n, nothing else."""
    b = batch(name)
    d_cols, d_heaps = to_dev(b.cols, dev), to_dev(b.heaps, dev)
    enc = TreeEncoder(b.tree, b.rows, dev)
    enc.total.fill_(-7)
    unframed = int(enc.encode(d_cols, d_heaps, None, None).item())
    enc.total.fill_(-7)
    framed = int(enc.encode_frames(d_cols, d_heaps, None, None).item())
    assert unframed == b.stream.size and framed == unframed + 4 * b.n


def test_frames_wrapper_and_empty_batch(dev, kernel):
    b = batch("pkg1_n65")
    want, wends = expected(b)
    frames, fends = spec_amd.encode_tree_frames(b.tree, to_dev(b.cols, dev), to_dev(b.heaps, dev), b.n, rows=b.rows)
    torch.cuda.synchronize()
    assert_frames(frames.cpu().numpy(), fends.cpu().numpy(), want, wends, f"wrapper {kernel}")
    # n == 0: *total = 0 and nothing else
    tree = b.tree
    from spec_amd.tree import ROLE_BEGIN

    cols = {c.name: torch.zeros((1, 4), dtype=torch.uint8, device=dev) for c in tree.columns if c.role == ROLE_BEGIN}
    enc = TreeEncoder(tree, [0] * len(tree.tables), dev)
    buf = torch.full((128,), CANARY, dtype=torch.uint8, device=dev)
    enc.total.fill_(-7)
    assert int(enc.encode_frames(cols, {}, buf[64:64], None).item()) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all()


# ---- 4. the receive side decodes the frames ---------------------------------------------------------

@pytest.mark.parametrize("name", ["pkg1_n300", "shapes_lists"])
def test_receive_side_decodes_frames(dev, kernel, name):
    """frames_index_device reports the ends written; a TreeDecoder over the framed buffer (every
    message as a span behind its head: index_spans) decodes the oracle's columns — spans by their
    bytes, since their offsets are the framed buffer's."""
    b = batch(name)
    frames, fends = check_frames(b, dev, f"{name} {kernel} receive")
    ends, consumed, status = spec_amd.frames_index_device(frames)
    assert status == 0 and consumed == frames.numel()
    assert torch.equal(ends, fends)
    st, _ = spec_amd.parse_messages(frames, fends, head=4)
    assert int((st != 0).sum()) == 0
    starts = torch.cat([fends.new_zeros(1), fends[:-1]]) + 4
    spans = torch.stack([starts, fends - starts], dim=1).to(torch.int32).contiguous()
    d = TreeDecoder(b.tree)
    assert d.index_spans(frames, spans) == b.want_rows
    got = [c.cpu().numpy() for c in d.decode().cols]
    torch.cuda.synchronize()
    fr = frames.cpu().numpy()
    for c, g, w in zip(b.tree.columns, got, b.want):
        if c.role == ROLE_VALUE and c.kind in (Kind.STRING, Kind.BYTES, Kind.ANY):
            assert span_bytes(g, fr) == span_bytes(w, b.stream), c.name
        else:
            assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)), c.name

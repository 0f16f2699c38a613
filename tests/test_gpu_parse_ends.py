"""spec_parse_batch at the edges of `ends` and of the stream's placement (include/spec_amd.h states the
contract): empty records, frames shorter than their head, an end that steps back inside its group,
record counts round the group of 64, a stream anywhere in its allocation, a first record shorter than
the 16 bytes the tail loader reads below a value's end, a last record that ends the allocation.  All of
these are defined: status and sizes equal the oracle's bit for bit, and nothing outside status[0, n)
and sizes[0, n) is written (parse_helpers.run_parse's canaries).

For ends the contract leaves undefined (outside their group's span, or past stream_len) the tests
assert only that the call succeeds, writes nothing outside its outputs and leaves every other group's
records as the oracle has them."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import any_values as A
from tests import parse_helpers as H
from tests.gpu_helpers import concat_records
from tests.test_oracle_parse import _list, _msg, parse_cases

pytestmark = pytest.mark.gpu


def pool():
    cat = {e.name: e.data for e in A.catalog()}
    return (list(parse_cases().values()) + H.shallow_records()
            + [cat[k] for k in ("bin256", "string_127", "bytes_128", "message_list_message", "bad_bin256_31_bytes")])


def mixed(n, shift=0):
    p = pool()
    return [p[(i + shift) % len(p)] for i in range(n)]


def framed(recs, stubs=()):
    """recs as mpx frames ([u32 big-endian size][record]); stubs: {record index: k}: k < 4 bytes of a
    frame cut short stand before that record as a record of their own.  Returns (stream, ends)."""
    parts = []
    stubs = dict(stubs)
    for i, r in enumerate(recs):
        if i in stubs:
            parts.append(bytes([0, 0, 0, 9][:stubs[i]]))
        parts.append(len(r).to_bytes(4, "big") + r)
    return concat_records(parts)


@pytest.mark.parametrize("root", H.ROOTS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 513])
def test_record_counts(dev, n, root):
    stream, ends = concat_records(mixed(n, shift=n))
    H.check_parse(dev, stream, ends, root=root, label=f"n={n} root {root}")
    fr, fends = framed(mixed(n, shift=n))
    H.check_parse(dev, fr, fends, head=4, root=root, label=f"frames n={n} root {root}")


@pytest.mark.parametrize("root", H.ROOTS)
def test_equal_consecutive_ends(dev, root):
    """Empty records: the first, the last, across a group boundary, a whole group of them."""
    recs = mixed(300)
    for i in [0, 1, 62, 63, 64, 65, 130, 299] + list(range(180, 260)):
        recs[i] = b""
    stream, ends = concat_records(recs)
    assert (np.diff(ends.astype(np.int64)) == 0).sum() >= 85
    slab, fits = H.batch_paths(stream.size, ends)
    assert slab > 0 and fits[0] and fits[3]  # (group 3 holds empty records only)
    st, sz = H.check_parse(dev, stream, ends, root=root, label=f"empty records root {root}")
    assert (st[180:260] == (H.ST_INVALID_VALUE if root == H.ROOT_VALUE else 0)).all() and not sz[180:260].any()
    H.check_parse(dev, np.zeros(0, np.uint8), np.zeros(70, np.uint64), root=root, label="an empty stream")


@pytest.mark.parametrize("root", H.ROOTS)
def test_frames_shorter_than_their_head(dev, root):
    """head = 4 and ends[r] - ends[r - 1] < 4: the record is empty on both sides (its start is clamped to
    its end), and the records behind it are the frames they were."""
    recs = mixed(200)
    stubs = {0: 3, 1: 0, 40: 1, 63: 2, 64: 3, 65: 0, 128: 2, 199: 1}
    stream, ends = framed(recs, stubs)
    gaps = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
    assert (gaps < 4).sum() == len(stubs) and len(ends) == 208
    st, sz = H.check_parse(dev, stream, ends, head=4, root=root, label=f"short frames root {root}")
    want, _ = O.parse_batch(*concat_records(recs), root=root)
    assert np.array_equal(st[gaps >= 4], want)
    assert (st[gaps < 4] == (H.ST_INVALID_VALUE if root == H.ROOT_VALUE else 0)).all()
    # only short frames: no record has a byte
    H.check_parse(dev, np.zeros(3 * 70, np.uint8), np.arange(1, 71, dtype=np.uint64) * 3, head=4, root=root,
                  label="short frames only")


def step_back(ends, rows):
    ends = ends.copy()
    for r in rows:
        assert 3 <= r % 64 < 63 and r + 1 < len(ends)  # the end it steps back to lies in its group's span
        ends[r] = ends[r - 3]
    return ends


@pytest.mark.parametrize("root", H.ROOTS)
@pytest.mark.parametrize("path", ["lds", "hbm"])
def test_end_steps_back_inside_its_group(dev, path, root):
    """make_group's rule: a record whose end lies below its start is empty; the next one starts at that
    end.  The group's span is unchanged, so it parses from where it did."""
    if path == "lds":
        stream, ends = concat_records(mixed(200))
    else:
        stream, ends, _ = H.depth_batch(H.DEPTH_BATCH_SIZES[0] - 128, H.SMALL_DEPTHS)
        stream = np.concatenate([stream, np.zeros(1 << 20, np.uint8)])  # an unused tail: no slab for this mean
    ends = step_back(ends, [20, 64 + 37, 64 + 61, 64 + 62] if path == "lds" else [5, 64 + 30])
    slab, fits = H.batch_paths(stream.size, ends)
    assert (slab > 0 and all(fits)) if path == "lds" else slab == 0
    st, sz = H.check_parse(dev, stream, ends, root=root, label=f"step back {path} root {root}")
    assert not sz[20 if path == "lds" else 5]


@pytest.mark.parametrize("frames", [False, True], ids=["records", "frames"])
@pytest.mark.parametrize("offset", [1, 15])
def test_stream_anywhere_in_its_allocation(dev, offset, frames):
    recs = mixed(130)
    stream, ends = framed(recs) if frames else concat_records(recs)
    for root in H.ROOTS:
        H.check_parse(dev, stream, ends, head=4 if frames else 0, root=root, offset=offset,
                      label=f"offset {offset} root {root}")
    b = H.value_batches("alone")["hbm"]
    H.check_parse(dev, b.stream, b.ends, root=H.ROOT_VALUE, offset=offset, label=f"offset {offset} from HBM")


FIRST = [bytes([A.T_TRUE]), bytes([A.T_BIN256]), bytes([A.T_STRING]), bytes([A.T_MESSAGE]), bytes([A.T_LIST]),
         O.encode("byte", 7)[0], bytes([0x80, A.T_INT64]), bytes([0, A.T_STRUCT]), bytes([3, A.T_BYTES]),
         O.encode("int32", 1000)[0], _msg([]), _list([]), bytes([0x80, 0x80, A.T_UINT64])]


@pytest.mark.parametrize("root", H.ROOTS)
@pytest.mark.parametrize("path", ["lds", "hbm"])
def test_first_record_shorter_than_a_tail_window(dev, path, root):
    """A first record of 1 to 3 bytes at offset 0 of the stream and of its allocation: what the tail
    loader reads below the record lies below the stream."""
    assert {len(f) for f in FIRST} == {1, 2, 3}
    for first in FIRST:
        recs = [first] + mixed(9)
        if path == "hbm":
            recs.append(O.encode("bytes", bytes(50000))[0])
        stream, ends = concat_records(recs)
        assert (H.slab_bytes(stream.size / len(ends)) > 0) == (path == "lds")
        H.check_parse(dev, stream, ends, root=root, label=f"first record {first.hex()} {path} root {root}")


@pytest.mark.parametrize("root", H.ROOTS)
def test_last_record_ends_the_stream(dev, root):
    """The last record ends at stream_len, where the stream's tensor ends too: values whose payload would
    lie past it, and whole ones."""
    cat = {e.name: e.data for e in A.catalog()}
    for last in (cat["bin256"], cat["string_127"], bytes([A.T_BIN256]), cat["message_small"], bytes([0xFF, 80]),
                 _list([cat["bin128"]])):
        for n in (1, 64, 65):
            stream, ends = concat_records(mixed(n - 1) + [last])
            assert ends[-1] == stream.size
            H.check_parse(dev, stream, ends, root=root, label=f"last record {last[-2:].hex()} n={n} root {root}")


# ---- ends outside the contract ---------------------------------------------------------------------
# validate.hip reads the stream through a buffer descriptor over [stream, stream + stream_len) (GlobalSrc,
# stage_span) and parses from its LDS slab only a lane whose record lies inside the span its group staged
# (parse_kernel sends every other lane to GlobalSrc); status and sizes are indexed by record alone.  So
# such ends can change what their own group's records parse to, and nothing else.

def undefined_batch(path):
    recs = mixed(256)
    if path == "hbm":
        recs[3] = O.encode("bytes", bytes(200000))[0]
    stream, ends = concat_records(recs)
    slab, fits = H.batch_paths(stream.size, ends)
    assert (slab > 0 and all(fits)) if path == "lds" else slab == 0
    return stream, ends


def check_other_groups(dev, stream, ends, bad_ends, root, label):
    """The call succeeds (run_parse checks the canaries) and every group whose ends are as they were has
    the oracle's records.  (The oracle never sees the bad ends: it would read outside its stream.)"""
    want_st, want_sz = O.parse_batch(stream, ends, root=root)
    rc, st, sz = H.run_parse(dev, stream, bad_ends, root=root)
    assert rc == 0, label
    changed = np.nonzero(bad_ends != ends)[0]
    # (a group's last end is the next group's first start)
    assert len(changed) and ((changed % 64 != 63) | (changed == len(ends) - 1)).all()
    same = ~np.isin(np.arange(len(ends)) // 64, changed // 64)
    assert same.sum() >= 64
    assert np.array_equal(st[same], want_st[same]) and np.array_equal(sz[same], want_sz[same]), label


@pytest.mark.parametrize("root", [H.ROOT_MESSAGE, H.ROOT_VALUE])
@pytest.mark.parametrize("path", ["lds", "hbm"])
def test_end_outside_its_group(dev, path, root):
    stream, ends = undefined_batch(path)
    bad = ends.copy()
    bad[64 + 10] = ends[127] + 1000          # beyond its group's last end
    bad[128 + 20] = ends[127] - 100          # below its group's first start
    bad[128 + 21] = 0
    assert bad.max() <= stream.size
    check_other_groups(dev, stream, ends, bad, root, f"end outside its group {path} root {root}")


@pytest.mark.parametrize("root", [H.ROOT_MESSAGE, H.ROOT_VALUE])
@pytest.mark.parametrize("path", ["lds", "hbm"])
def test_ends_past_the_stream(dev, path, root):
    stream, ends = undefined_batch(path)
    bad = ends.copy()
    bad[250] = stream.size + 64
    bad[254] = stream.size + 7
    bad[255] = stream.size + 1000            # the group's span ends past the stream
    check_other_groups(dev, stream, ends, bad, root, f"ends past the stream {path} root {root}")
    bad[192:] = stream.size + 1 + np.arange(64, dtype=np.uint64) * 50000  # past any slab
    check_other_groups(dev, stream, ends, bad, root, f"a group past the stream {path} root {root}")

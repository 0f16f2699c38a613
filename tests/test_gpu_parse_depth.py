"""spec_parse_batch at its depth constants (validate.hip): VAL_MAX_DEPTH = 32 frames of the main pass's
stack (31, 32, 33 and 34 levels), the 8,192 frames of a deep thread's arena slice (8,191, 8,192 and
8,193 levels), and DEEP_LIST_CAP = 65,536 records listed for the deep pass (65,536 and 65,537 of them).
Records nest through messages, lists, both, and a big message / big list at the level that crosses the
boundary; each well formed, with a malformed innermost value and with a swapped list table innermost.
tests/test_parse_inputs.py asserts every level count, path and deep-record count on the CPU.

Expected values are the oracle's alone, whose recursion has no limit."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import parse_helpers as H

pytestmark = pytest.mark.gpu

ALL_DEPTHS = H.SMALL_DEPTHS + H.LARGE_DEPTHS


@functools.lru_cache(maxsize=None)
def oracle_of(n, depths, root, frames=False):
    stream, ends, _ = H.depth_batch(n, depths)
    if frames:
        stream, ends = H.frame_batch(stream, ends)
    return O.parse_batch(stream, ends, 4 if frames else 0, root=root)


def check_forms(st, at, root):
    """Under ParseValue every depth record parses from its root container: the form's status."""
    if root == H.ROOT_VALUE:
        for i, d in at.items():
            assert st[i] == H.FORM_STATUS[d.form], d.name
    assert not (st == H.ST_TOO_DEEP).any()


@pytest.mark.parametrize("root", H.ROOTS)
@pytest.mark.parametrize("n", H.DEPTH_BATCH_SIZES)
def test_depth_32_from_lds(dev, n, root):
    """31 to 34 levels in a batch that parses from LDS: 33 and 34 go to the deep pass."""
    stream, ends, at = H.depth_batch(n - 128, H.SMALL_DEPTHS)
    st, _ = H.check_parse(dev, stream, ends, root=root, label=f"depth 32 lds n={n - 128} root {root}",
                          want=oracle_of(n - 128, H.SMALL_DEPTHS, root))
    check_forms(st, at, root)


@pytest.mark.parametrize("root", H.ROOTS)
@pytest.mark.parametrize("n", H.DEPTH_BATCH_SIZES)
def test_depth_boundaries(dev, n, root):
    """Every depth in one batch (from HBM: its mean record has no slab), the deep records at record 0,
    at the last record of a partial last group and in between, shallow good and bad records round them."""
    stream, ends, at = H.depth_batch(n, ALL_DEPTHS)
    st, _ = H.check_parse(dev, stream, ends, root=root, label=f"depths n={n} root {root}",
                          want=oracle_of(n, ALL_DEPTHS, root))
    check_forms(st, at, root)


@pytest.mark.parametrize("root", H.ROOTS)
@pytest.mark.parametrize("depths", [H.SMALL_DEPTHS, ALL_DEPTHS], ids=["lds", "hbm"])
def test_depth_frames(dev, depths, root):
    """The same batches as mpx frames, head = 4: deep_one works out a record's bounds by itself."""
    n = H.DEPTH_BATCH_SIZES[1] - (128 if depths == H.SMALL_DEPTHS else 0)
    stream, ends, at = H.depth_batch(n, depths)
    fr, fends = H.frame_batch(stream, ends)
    want = oracle_of(n, depths, root, frames=True)
    assert np.array_equal(want[0], oracle_of(n, depths, root)[0])  # framing changes no record
    st, _ = H.check_parse(dev, fr, fends, head=4, root=root, label=f"frames root {root}", want=want)
    check_forms(st, at, root)


def test_depth_no_sizes(dev):
    """sizes = NULL: the statuses alone, from the main pass and from the deep pass; nothing is written
    where sizes would be (run_parse's canaries and its untouched sizes buffer)."""
    n = H.DEPTH_BATCH_SIZES[0]
    stream, ends, at = H.depth_batch(n, ALL_DEPTHS)
    st, sz = H.check_parse(dev, stream, ends, sizes=False, label="no sizes", want=oracle_of(n, ALL_DEPTHS, H.ROOT_MESSAGE))
    assert sz is None and {0, H.ST_PANIC, H.ST_INVALID_VALUE} <= set(st.tolist())


@pytest.mark.parametrize("count", [H.DEEP_LIST_CAP, H.DEEP_LIST_CAP + 1], ids=["listed_65536", "scanned_65537"])
def test_deep_kernel_modes(dev, count):
    """65,536 records over 32 levels are the most deep_kernel takes from the main pass's list; with
    65,537 it scans every record's status instead.  Among them shallow good and bad records, deep
    records with a malformed innermost value and one record of 8,193 levels for the whole-arena thread.
    (DEEP_LIST_CAP fixes the size: these are the smallest batches that reach either side.)"""
    stream, ends, is_deep = H.deep_mode_batch(count)
    assert int(is_deep.sum()) == count
    st, sz = H.check_parse(dev, stream, ends, label=f"{count} deep records")
    assert not (st == H.ST_TOO_DEEP).any()
    assert set(st[is_deep].tolist()) == {0, H.ST_INVALID_VALUE} and (sz[is_deep & (st == 0)] > 0).all()

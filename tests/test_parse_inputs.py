"""What the parse validator's GPU tests (test_gpu_parse_values.py, test_gpu_parse_depth.py,
test_gpu_parse_ends.py) assume about their inputs, checked without a GPU: the rule the catalog's
scalars are held to, which batch parses from LDS and which from HBM, how many levels every depth record
has, and how many records of the deep-list batches the main pass must hand to the deep pass."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import any_values as A
from tests import parse_helpers as H


def test_scalar_rule_against_the_oracle():
    """ParseValue of every scalar the rule covers, alone and behind junk: status 0 and the value's own
    length, or an error for the range errors — the rule is written from value.go and the decoders, the
    oracle only confirms it.  Every scalar type of DecodeTypeSize's switch is covered by an ok value,
    and both 16-bit integer types by a value on either side of either bound."""
    vals = H.value_placements()
    ruled = [v for v in vals if v.rule is not None]
    assert len(vals) == 720 + 4 * len(H.extra_entries()) and len(ruled) >= 4 * 150
    seen = set()
    for v in ruled:
        n, err = O.parse_value(v.slot)
        if v.rule[0] == 0:
            assert err is None and n == v.rule[1] == len(v.slot) - v.junk, (v.name, v.junk, n, err)
            seen.add(v.slot[-1])
        else:
            assert err is not None and "index out of range" not in err, (v.name, v.junk, err)
    assert seen == set(A.SWITCH_TYPES) - set(H.CONTAINER_TYPES)
    names = {v.name for v in ruled}
    assert {"uint16_65535", "uint16_65536", "int16_32767", "int16_32768", "int16_m32768", "int16_m32769"} <= names
    assert {v.rule[0] for v in ruled if v.name in ("uint16_65536", "int16_32768", "int16_m32769") + H.RANGE_ERRS} == {7}


@pytest.mark.parametrize("embedding", [e[0] for e in H.EMBEDDINGS])
def test_value_batches_take_the_path_they_claim(embedding):
    b = H.value_batches(embedding)
    slab, fits = H.batch_paths(b["lds"].stream.size, b["lds"].ends)
    assert slab > 0 and all(fits) and len(fits) > 1 and len(b["lds"].ends) % 64
    slab, fits = H.batch_paths(b["fallback"].stream.size, b["fallback"].ends)
    keys = np.array(b["fallback"].keys)
    with_values = [bool((keys[g:g + 64] >= 0).any()) for g in range(0, len(keys), 64)]
    assert slab > 0 and sum(with_values) > 1
    assert not any(f for f, w in zip(fits, with_values) if w)  # the group-level fallback
    assert sorted(k for k in keys if k >= 0) == sorted(b["lds"].keys)
    slab, fits = H.batch_paths(b["hbm"].stream.size, b["hbm"].ends)
    assert slab == 0 and not any(fits)
    vals = H.value_placements()
    assert list(b["hbm"].keys) == list(range(len(vals)))
    assert sorted(b["lds"].keys) == [i for i, v in enumerate(vals) if not v.large] and sum(v.large for v in vals) == 24
    # every record of the deep batch: one level more than the main pass's stack holds
    ends = b["deep"].ends
    for i in range(len(ends)):
        rec = bytes(b["deep"].stream[int(ends[i - 1]) if i else 0:int(ends[i])])
        assert H.levels(rec, H.ROOT_MESSAGE) == H.levels(rec, H.ROOT_VALUE) == H.VAL_MAX_DEPTH + 1, (embedding, i)


def test_levels_counts_what_the_validator_stacks():
    i64 = H.I64
    assert H.levels(i64, H.ROOT_VALUE) == 0 and H.levels(b"", H.ROOT_MESSAGE) == 0
    assert H.levels(H.nest(1, i64), H.ROOT_MESSAGE) == H.levels(H.nest(1, i64), H.ROOT_VALUE) == 1
    assert H.levels(H.nest(1, i64), H.ROOT_LIST) == 0  # not a list: nothing decodes
    assert H.levels(H.nest(5, i64, ("list", "big_message")), H.ROOT_LIST) == 5
    assert H.levels(H.nest(4, H.BAD_VALUE, ("big_list",)), H.ROOT_VALUE) == 4
    assert H.levels(H.SWAPPED_LIST, H.ROOT_LIST) == 1
    assert H.levels(H.nest(2, bytes([0xFF, 80])), H.ROOT_MESSAGE) == 2  # a message whose table does not decode
    wide = H._list([H.nest(2, i64), H.nest(7, i64, ("list",)), i64])
    assert H.levels(wide, H.ROOT_VALUE) == 8


def test_depth_records_have_the_levels_their_names_say():
    """levels() of every depth record under ParseValue, where the root container counts as a level like
    any other, and under the root of its outermost container; the big container of the big nestings
    sits at the level that crosses the boundary; ParseValue's answer is the form's."""
    recs = H.depth_records()
    assert len(recs) == 7 * 5 * 3 and len({r.name for r in recs}) == len(recs)
    st, _ = O.parse_batch(*H.concat_records([r.data for r in recs]), root=H.ROOT_VALUE)
    for r, s in zip(recs, st):
        bigs = []
        assert H.levels(r.data, H.ROOT_VALUE, bigs) == r.levels == int(r.name.split("_")[0]), r.name
        if r.levels <= 34 or r.via == "alternating":
            own = H.ROOT_LIST if r.data[-1] in H.LIST_TYPES else H.ROOT_MESSAGE
            assert H.levels(r.data, own) == r.levels, r.name
        assert s == H.FORM_STATUS[r.form], r.name
        cross = H.ARENA_SLICE if r.levels > H.ARENA_SLICE else H.VAL_MAX_DEPTH
        wraps = r.levels - (r.form == "swapped_list")
        if r.via.startswith("big_"):
            assert (min(cross, wraps - 1) + 1, True) in bigs, r.name
        if r.levels <= 34:
            assert sum(b for _, b in bigs) == r.via.startswith("big_"), r.name


@pytest.mark.parametrize("n", H.DEPTH_BATCH_SIZES)
def test_depth_batches_place_and_path(n):
    """The deep records sit at record 0, at the last record of a partial last group and in between; the
    batch of the boundary at 32 parses from LDS, the batch with the 8,192 boundary from HBM."""
    assert n % 64 in (1, 63)
    for depths, small in ((H.SMALL_DEPTHS, True), (H.SMALL_DEPTHS + H.LARGE_DEPTHS, False)):
        m = n if not small else n - 128
        stream, ends, at = H.depth_batch(m, depths)
        assert len(ends) == m and m % 64 == n % 64 and 0 in at and m - 1 in at and len(at) == 15 * len(depths)
        assert sum(1 for i in range(m) if i not in at) >= m // 2 - 1
        slab, fits = H.batch_paths(stream.size, ends)
        assert (slab > 0 and all(fits)) if small else slab == 0
        fr, fends = H.frame_batch(stream, ends)
        slab, fits = H.batch_paths(fr.size, fends, head=4)
        assert (slab > 0 and all(fits)) if small else slab == 0


@pytest.mark.parametrize("count", [H.DEEP_LIST_CAP, H.DEEP_LIST_CAP + 1])
def test_deep_mode_batches_hold_exactly_their_count(count):
    """levels() > 32 for exactly 65,536 records (the last count deep_kernel takes from its list) and
    65,537 (the first it scans every status for); one of them is over a deep thread's arena slice."""
    stream, ends, is_deep = H.deep_mode_batch(count)
    memo, deep, over_slice = {}, 0, 0
    lo = 0
    buf = stream.tobytes()
    for i, e in enumerate(ends):
        rec = buf[lo:int(e)]
        lo = int(e)
        if rec not in memo:
            memo[rec] = H.levels(rec, H.ROOT_MESSAGE)
        assert (memo[rec] > H.VAL_MAX_DEPTH) == bool(is_deep[i])
        deep += memo[rec] > H.VAL_MAX_DEPTH
        over_slice += memo[rec] > H.ARENA_SLICE
    assert deep == count == int(is_deep.sum()) and over_slice == 1
    assert set(memo.values()) == {1, H.VAL_MAX_DEPTH + 1, H.ARENA_SLICE + 1}
    assert len(memo) == H.DEEP_BLOCK + 1 and 13 << 20 < stream.size < 16 << 20
    st, _ = O.parse_batch(stream, ends)
    assert set(st[is_deep]) == {0, 7} and set(st[~is_deep]) == {0, 7}

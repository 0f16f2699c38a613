"""The typed-value catalog (tests/any_values.py: every type of DecodeTypeSize's switch, well formed and
malformed, alone and behind junk, plus parse_helpers' 16-bit integers just out of range) through
spec_parse_batch: every value alone, as a list element, as a message field and as a list element inside a
message field, under every root that embedding has, through each instantiation of validate.hip's
parse_record — from LDS, from HBM (a group over the batch's slab; a batch with no slab) and through
deep_kernel (33 levels).  tests/test_parse_inputs.py asserts on the CPU that each batch takes the path
it is built for.

Every run == the oracle bit for bit (status and sizes); the scalars == the rule parse_helpers states
apart from the oracle; and one value has one status whatever path parsed it."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import parse_helpers as H

pytestmark = pytest.mark.gpu

EMBEDDINGS = {e[0]: e[1] for e in H.EMBEDDINGS}
PATHS = ("lds", "fallback", "hbm", "deep")


def path_roots(embedding, path):
    # the deep batch's records are messages whatever they wrap
    return (H.ROOT_MESSAGE, H.ROOT_VALUE) if path == "deep" else EMBEDDINGS[embedding]


@functools.lru_cache(maxsize=None)
def run(dev, embedding, path, root):
    """One batch under one root == the oracle; returns ({value index: status}, {value index: size})."""
    b = H.value_batches(embedding)[path]
    st, sz = H.check_parse(dev, b.stream, b.ends, root=root, label=f"{embedding} {path} root {root}")
    keys = np.array(b.keys)
    sel = keys >= 0
    return dict(zip(keys[sel].tolist(), st[sel].tolist())), dict(zip(keys[sel].tolist(), sz[sel].tolist()))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("embedding", list(EMBEDDINGS))
def test_catalog_values(dev, embedding, path):
    vals = H.value_placements()
    for root in path_roots(embedding, path):
        st, sz = run(dev, embedding, path, root)
        assert len(st) == len(H.value_batches(embedding)[path].ends) - H.value_batches(embedding)[path].keys.count(-1)
        ruled = 0
        for k, s in st.items():
            rule = vals[k].rule
            if rule is None:
                continue
            ruled += 1
            # an error inside any container is INVALID_VALUE; everything round the value is well formed
            assert s == rule[0], (embedding, path, root, vals[k].name, vals[k].junk, s)
            if embedding == "alone" and path != "deep":  # the record is the value: ParseValue's size
                assert sz[k] == rule[1], (embedding, path, root, vals[k].name, vals[k].junk, sz[k])
        assert ruled >= 8
        assert {0, H.ST_PANIC, H.ST_INVALID_VALUE} <= set(st.values())


@pytest.mark.parametrize("embedding", list(EMBEDDINGS))
def test_one_status_whatever_path(dev, embedding):
    """From LDS, from HBM and through deep_kernel, under every root: one value, one status (the roots
    differ only in the class of the root's own trailer, which is well formed in every record here)."""
    seen = {}
    for path in PATHS:
        for root in path_roots(embedding, path):
            for k, s in run(dev, embedding, path, root)[0].items():
                seen.setdefault(k, {})[(path, root)] = s
    vals = H.value_placements()
    assert len(seen) == len(vals)
    for k, by in seen.items():
        assert len(by) == (1 if vals[k].large else 3) * len(EMBEDDINGS[embedding]) + 2
        assert len(set(by.values())) == 1, (embedding, vals[k].name, vals[k].junk, by)

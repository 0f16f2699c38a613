"""Writes tests/golden/precompile_presence_trees.json: the build-time list of the presence tests'
schema trees (tests/tree_presence_helpers.py presence_test_trees) whose schema-specialised kernels
build() precompiles, as flattened descriptors [(path, tag, kind, elem, parent[, 1 = optional]), ...].
tests/test_tree_presence.py checks the file is current.

    python tests/golden/make_precompile_presence_trees.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from spec_amd.tree_catalog import PRESENCE_TREES_JSON  # noqa: E402
from tests.tree_presence_helpers import presence_test_trees  # noqa: E402

if __name__ == "__main__":
    json.dump({k: t.to_fields() for k, t in presence_test_trees().items()}, open(PRESENCE_TREES_JSON, "w"), indent=0)
    print(PRESENCE_TREES_JSON)

"""The unframed spec_encode_nested (config 4, 1M records, the _items workspace) and spec_encode_tree
(pkg1, 262,144 records) through the build of the checkout ROOT, for A/B runs of two builds in
alternating processes (profiles/egress/encode_nested_tree_ab.json): per encoder the mean of 40
back-to-back launches, the median / p10 / p90 of per-launch event pairs, the stream's size and the
first 16 hex digits of its SHA-1.  Prints one line "AB {json}".

    python tools/bench_encode_nested_tree.py [ROOT] [LABEL]     (default: this checkout, "new")
"""
import json
import os
import sys

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
LABEL = sys.argv[2] if len(sys.argv) > 2 else "new"
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import spec_amd  # noqa: E402
from spec_amd import NESTED, workload  # noqa: E402

assert os.path.dirname(spec_amd.LIB_PATH) == os.path.join(ROOT, "spec_amd"), spec_amd.LIB_PATH
dev = torch.device("cuda", 0)
n = 1 << 20
w = workload.nested(n, 0x5EC0DE)
m = len(w["key"])
to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
outer = [to(w["id"]), to(w["seq"].view(np.uint8).reshape(n, 8)), to(w["name"].view(np.uint8).reshape(n, 8)), None]
items = [to(w["key"].view(np.uint8).reshape(m, 4)), to(w["value"].view(np.uint8).reshape(m, 8)),
         to(w["label"].view(np.uint8).reshape(m, 8))]
oh, ih, ib = {2: to(w["name_heap"])}, {2: to(w["label_heap"])}, to(w["item_begin"].view(np.int32))
enc = spec_amd.NestedEncoder(NESTED, n, dev)
sb = int(enc.encode(outer, oh, ib, items, ih, m).item())
s2, e2 = torch.empty(sb, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
f = lambda: enc.encode(outer, oh, ib, items, ih, m, s2, e2)  # noqa: E731
bench.gpu_prewarm(f)
nm = bench.kernel_time_events(f, 40, lead=3, spread=True)
import hashlib  # noqa: E402
nh = hashlib.sha1(s2.cpu().numpy().tobytes()).hexdigest()[:16]

tn = 1 << 18
tree = spec_amd.pkg1_tree()
cols, heaps, rows = workload.tree_batch(tree, tn, 7)
dc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cols.items()}
dh = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in heaps.items()}
tenc = spec_amd.TreeEncoder(tree, rows, dev)
tb = int(tenc.encode(dc, dh, None, None).item())
t2, te = torch.empty(tb, dtype=torch.uint8, device=dev), torch.empty(tn, dtype=torch.int64, device=dev)
g = lambda: tenc.encode(dc, dh, t2, te)  # noqa: E731
bench.gpu_prewarm(g)
tm = bench.kernel_time_events(g, 40, lead=3, spread=True)
th = hashlib.sha1(t2.cpu().numpy().tobytes()).hexdigest()[:16]
r4 = lambda t: [round(x, 4) for x in t]  # noqa: E731
print("AB " + json.dumps({"build": LABEL, "nested_mean_med_p10_p90_ms": r4(nm), "nested_bytes": sb, "nested_sha": nh,
                          "tree_mean_med_p10_p90_ms": r4(tm), "tree_bytes": tb, "tree_sha": th}), flush=True)

"""Schema-tree leg alone (bench.tree_leg: pkg1.Message, 262144 records): one JSON line.

    python tools/bench_tree.py              the bench's tree leg
    python tools/bench_tree.py --presence   the cost of the HASMASK column: pkg1 without
        optional fields (T) against pkg1 with every eligible field optional (T') at all-ones masks, decode
        and encode, the legs taking turns in one process; and T' at has = 0.75.  Medians and the spread
        (min, max) over the rounds; the added algorithmic bytes are 8 W per row per flagged table.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import spec_amd  # noqa: E402
from spec_amd import workload  # noqa: E402
from spec_amd.tree import ROLE_HASMASK  # noqa: E402


def presence_leg(dev, n=1 << 18, seed=7, rounds=5, calls=20):
    legs = {}

    def prepare(name, tree, has):
        cols, heaps, rows = workload.tree_batch(tree, n, seed, has=has)
        dc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cols.items()}
        dh = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in heaps.items()}
        enc = spec_amd.TreeEncoder(tree, rows, dev)
        total = int(enc.encode(dc, dh, None, None).item())
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        ends = torch.empty(n, dtype=torch.int64, device=dev)
        enc.encode(dc, dh, out, ends)
        torch.cuda.synchronize()
        d = spec_amd.TreeDecoder(tree)
        d.index(out, ends)
        dcols = d.alloc(dev)
        rows_out = torch.empty(len(tree.tables), dtype=torch.int64, device=dev)
        col_rows = d.column_capacity(dcols)
        mask_bytes = sum(c.width * rows[c.table] for c in tree.columns if c.role == ROLE_HASMASK)
        legs[name] = {"encode": lambda: enc.encode(dc, dh, out, ends),
                      "decode": lambda: d.run(out, ends, dcols, rows_out, col_rows=col_rows),
                      "stream_bytes": total, "hasmask_bytes": int(mask_bytes), "keep": (enc, d, dc, dh, dcols)}

    prepare("plain", spec_amd.pkg1_tree(), 1.0)
    prepare("presence_ones", spec_amd.pkg1_tree(2, presence=True), 1.0)
    prepare("presence_has075", spec_amd.pkg1_tree(2, presence=True), 0.75)
    times = {k: {"encode": [], "decode": []} for k in legs}
    for _ in range(rounds):
        for name, leg in legs.items():
            for what in ("decode", "encode"):
                bench.gpu_prewarm(leg[what], 0.05)
                ms, _ = bench.kernel_time_events(leg[what], calls)
                times[name][what].append(ms)
    res = {"records": n, "rounds": rounds, "calls_per_round": calls}
    for name, leg in legs.items():
        res[name] = {"stream_bytes": leg["stream_bytes"], "hasmask_bytes": leg["hasmask_bytes"]}
        for what in ("decode", "encode"):
            t = times[name][what]
            res[name][f"{what}_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4),
                                       "max": round(max(t), 4)}
    return res


def main():
    dev = torch.device("cuda", 0)
    if "--presence" in sys.argv[1:]:
        print(json.dumps({"tree_presence": presence_leg(dev)}))
    else:
        print(json.dumps({"tree_pkg1": bench.tree_leg(dev)}))


if __name__ == "__main__":
    main()

"""The receive side over mpx frames against the unframed decoders, on the bench's batches: config 4
(1M Nested records) and pkg1 (262,144 records) through the build of the checkout ROOT.

  (a) unframed decode: spec_decode_nested_onepass / spec_tree_decoder_run (bench.py's nested.decode_ms
      and tree_pkg1.decode_ms), and the two-call forms (index + decode);
  (b) the same records as frames, decoded in place: spec_decode_nested_frames_onepass /
      spec_tree_decoder_run_frames, and the two-call forms;
  (c) tree only, the route before spec_tree_decoder_index_frames: an (off, len) span per frame built
      with torch ops + index_spans + decode, the span construction inside the timed region.

HIP events around every launch, 5 rounds x 20 launches after a warm-up, one process: the median and
the 10th / 90th percentiles of the 100 intervals, and each round's mean.  A checkout without the
framed entry points (the parent commit, for the A/B of the unframed paths) reports (a) only.
Prints one line "INGRESS {json}"; --out FILE also writes the json there.

    python tools/bench_ingress.py [ROOT] [LABEL] [--out FILE] [--unframed-only]
                                                        (default: this checkout, "new")

A/B of the unframed paths (must not pay for `head`): alternate two checkouts' builds, three
processes each, with --unframed-only, and compare nested.decode_ms and tree_pkg1.decode_ms.
"""
import json
import os
import sys

argv = [a for a in sys.argv[1:]]
OUT = None
UNFRAMED_ONLY = "--unframed-only" in argv
if UNFRAMED_ONLY:
    argv.remove("--unframed-only")
if "--out" in argv:
    i = argv.index("--out")
    OUT = argv[i + 1]
    del argv[i:i + 2]
ROOT = os.path.abspath(argv[0] if argv else os.path.join(os.path.dirname(__file__), ".."))
LABEL = argv[1] if len(argv) > 1 else "new"
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import spec_amd  # noqa: E402
from spec_amd import NESTED, workload  # noqa: E402

assert os.path.dirname(spec_amd.LIB_PATH) == os.path.join(ROOT, "spec_amd"), spec_amd.LIB_PATH
FRAMED = hasattr(spec_amd, "decode_nested_frames") and not UNFRAMED_ONLY
ROUNDS, LAUNCHES = 5, 20
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream()


def measure(fn):
    """{median, p10, p90, round_means} in ms of ROUNDS x LAUNCHES event-timed calls of fn."""
    bench.gpu_prewarm(fn, 0.2)
    ms, means = [], []
    for _ in range(ROUNDS):
        for _ in range(3):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)]
        for x, y in evs:
            x.record(s)
            fn()
            y.record(s)
        torch.cuda.synchronize()
        t = [x.elapsed_time(y) for x, y in evs]
        ms += t
        means.append(sum(t) / len(t))
    ms.sort()
    r4 = lambda v: round(v, 4)  # noqa: E731
    return {"median_ms": r4(ms[len(ms) // 2]), "p10_ms": r4(ms[len(ms) // 10]), "p90_ms": r4(ms[9 * len(ms) // 10]),
            "mean_ms": r4(sum(ms) / len(ms)), "round_means_ms": [r4(m) for m in means]}


to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
res = {"build": LABEL, "rounds": ROUNDS, "launches_per_round": LAUNCHES}

# ---- config 4: 1M Nested records ----------------------------------------------------------------
n = 1 << 20
w = workload.nested(n, 0x5EC0DE)
m = len(w["key"])
outer = [to(w["id"]), to(w["seq"].view(np.uint8).reshape(n, 8)), to(w["name"].view(np.uint8).reshape(n, 8)), None]
items = [to(w["key"].view(np.uint8).reshape(m, 4)), to(w["value"].view(np.uint8).reshape(m, 8)),
         to(w["label"].view(np.uint8).reshape(m, 8))]
oh, ih, ib = {2: to(w["name_heap"])}, {2: to(w["label_heap"])}, to(w["item_begin"].view(np.int32))
stream, ends = spec_amd.encode_nested(NESTED, outer, oh, ib, items, ih, n)
torch.cuda.synchronize()


def nested_case(d):
    d.index()
    d.reserve(int(d.total.item()))

    def two():
        d.index()
        d.decode()

    r = {"onepass": measure(d.decode_onepass), "index_decode": measure(two)}
    torch.cuda.synchronize()
    ok = int(d.status.sum()) == 0 and int(d.total.item()) == m and torch.equal(d.items[0], items[0])
    ok = ok and torch.equal(d.item_begin, ib) and torch.equal(d.items[2][:, 4:], items[2][:, 4:])
    r["verified"] = bool(ok)
    return r


nres = {"records": n, "items": m, "stream_bytes": int(stream.numel()),
        "unframed": nested_case(spec_amd.NestedDecoder(NESTED, stream, ends))}
nres["decode_ms"] = nres["unframed"]["onepass"]["mean_ms"]
if FRAMED:
    frames, fends = spec_amd.encode_nested_frames(NESTED, outer, oh, ib, items, ih, n)
    torch.cuda.synchronize()
    nres["frames_bytes"] = int(frames.numel())
    nres["framed"] = nested_case(spec_amd.NestedDecoder(NESTED, frames, fends, head=4))
    for k in ("onepass", "index_decode"):
        nres[f"framed_over_unframed_{k}"] = round(nres["framed"][k]["median_ms"] / nres["unframed"][k]["median_ms"], 4)
    del frames, fends
res["nested"] = nres
del stream, ends, outer, items

# ---- pkg1: 262,144 records ------------------------------------------------------------------------
tn = 1 << 18
tree = spec_amd.pkg1_tree()
cols, heaps, rows = workload.tree_batch(tree, tn, 7)
dc = {k: to(v) for k, v in cols.items()}
dh = {k: to(v) for k, v in heaps.items()}
tstream, tends = spec_amd.encode_tree(tree, dc, dh, tn, rows=rows)
torch.cuda.synchronize()


def tree_case(index, run, first=None):
    d = spec_amd.TreeDecoder(tree)
    got_rows = index(d)
    dcols = d.alloc(dev)
    rows_out = torch.empty(len(tree.tables), dtype=torch.int64, device=dev)
    col_rows = d.column_capacity(dcols)

    def two():
        index(d)
        d.decode(cols=dcols)

    r = {"index_decode": measure(two)}
    if run is not None:
        r["run"] = measure(lambda: run(d, dcols, rows_out, col_rows))
        torch.cuda.synchronize()
        r["verified"] = [int(x) for x in rows_out.cpu()] == got_rows == rows
    else:
        r["verified"] = got_rows == rows
    if first is not None:  # the same columns as the first case's (spans aside: offsets differ by the heads)
        span = {c.index for c in tree.columns if c.role == 0 and int(c.kind) in (14, 15, 19)}
        r["verified"] = r["verified"] and all(torch.equal(a[: b.shape[0]], b[: a.shape[0]]) for i, (a, b) in
                                              enumerate(zip(dcols, first)) if i not in span)
    return r, dcols


tres = {"records": tn, "stream_bytes": int(tstream.numel()), "rows": rows}
tres["unframed"], base_cols = tree_case(lambda d: d.index(tstream, tends),
                                        lambda d, c, ro, cr: d.run(tstream, tends, c, ro, col_rows=cr))
tres["decode_ms"] = tres["unframed"]["run"]["mean_ms"]
if FRAMED:
    tframes, tfends = spec_amd.encode_tree_frames(tree, dc, dh, tn, rows=rows)
    torch.cuda.synchronize()
    tres["frames_bytes"] = int(tframes.numel())
    tres["framed"], _ = tree_case(lambda d: d.index_frames(tframes, tfends),
                                  lambda d, c, ro, cr: d.run_frames(tframes, tfends, c, ro, col_rows=cr), base_cols)

    def index_spans(d):  # (c) the spans of the frames' messages, built with torch ops
        starts = torch.cat([tfends.new_zeros(1), tfends[:-1]]) + 4
        spans = torch.stack([starts, tfends - starts], dim=1).to(torch.int32).contiguous()
        return d.index_spans(tframes, spans)

    tres["spans_workaround"], _ = tree_case(index_spans, None, base_cols)
    tres["framed_over_unframed_run"] = round(tres["framed"]["run"]["median_ms"] / tres["unframed"]["run"]["median_ms"], 4)
    tres["framed_over_unframed_index_decode"] = round(
        tres["framed"]["index_decode"]["median_ms"] / tres["unframed"]["index_decode"]["median_ms"], 4)
    tres["framed_over_spans_workaround_index_decode"] = round(
        tres["framed"]["index_decode"]["median_ms"] / tres["spans_workaround"]["index_decode"]["median_ms"], 4)
res["tree_pkg1"] = tres

print("INGRESS " + json.dumps(res), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)

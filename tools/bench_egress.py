"""The send path on the bench's 1M Flat16 records (272 MB framed): spec_frames_write against a
device-to-device copy of the same bytes in the same run (step "frames"), and the fused framed
encoder spec_encode_flat_frames against spec_encode_flat alone and spec_encode_flat followed by
spec_frames_write (step "fused"); the same three legs for the nested encoder on the bench's
config-4 batch (step "nested_fused": spec_encode_nested_frames) and for the tree encoder on the
bench's pkg1 batch of 262,144 records (step "tree_fused": spec_encode_tree_frames).  Writes
profiles/<run>/egress.json; with --steps only the named steps run and the file's other keys stay.

Every GPU step is a child process of its own under a time limit; a step that fails or runs out
of time ends the run (nothing more is started on the GPU).

    python tools/bench_egress.py [--run NAME] [--out DIR] [--n RECORDS] [--steps a,b]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("frames", 240), ("fused", 300), ("nested_fused", 300), ("tree_fused", 420))
TREE_N = 1 << 18  # bench.py tree_leg's batch
SEED = 0x5EC0DE


def _p(t):
    return C.c_void_p(t.data_ptr())


def step_frames(n):
    import torch

    import bench
    import spec_amd

    dev = torch.device("cuda", 0)
    _, _, _, _, stream, ends = bench.make_batch(n, SEED, dev)
    total = stream.numel() + 4 * n
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    fe = torch.empty(n, dtype=torch.int64, device=dev)
    L = spec_amd.lib()

    def write():
        rc = L.spec_frames_write(_p(stream), stream.numel(), _p(ends), n, _p(out), total, _p(fe),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    src = torch.empty(total, dtype=torch.uint8, device=dev)

    def copy():
        L.spec_copy_d2d(_p(out), _p(src), total, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    bench.gpu_prewarm(copy)
    c_ms, c_med, c_lo, c_hi = bench.kernel_time_events(copy, 20, lead=3, spread=True)
    w_ms, w_med, w_lo, w_hi = bench.kernel_time_events(write, 20, lead=3, spread=True)
    write()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out, spec_amd.make_frames_device(stream, ends)))
    return {"records": n, "stream_bytes": int(stream.numel()), "framed_bytes": int(total),
            "write_ms": round(w_ms, 4), "write_median_ms": round(w_med, 4), "write_p10_p90_ms": [round(w_lo, 4), round(w_hi, 4)],
            "d2d_copy_ms": round(c_ms, 4), "d2d_copy_median_ms": round(c_med, 4),
            "d2d_copy_p10_p90_ms": [round(c_lo, 4), round(c_hi, 4)],
            "write_gb_s": round((stream.numel() + total + 16 * n) / (w_ms * 1e-3) / 1e9, 1),
            "d2d_copy_gb_s": round(2 * total / (c_ms * 1e-3) / 1e9, 1),
            "write_over_copy": round(w_ms / c_ms, 3), "ends_traffic_bytes": 16 * n, "ok": ok}


def step_fused(n, rounds=5, reps=20):
    """(a) spec_encode_flat, (b) spec_encode_flat + spec_frames_write, (c) spec_encode_flat_frames on
    the same columns, timed in alternating rounds in one process.  Per leg: the mean of the rounds'
    back-to-back means, the median of their medians, and [lowest p10, highest p90] over the rounds
    (the widest spread seen, so "c's p90 below b's p10" holds for every pair of rounds)."""
    import torch

    import bench
    import spec_amd

    dev = torch.device("cuda", 0)
    _, _, d_cols, d_heaps, stream, ends = bench.make_batch(n, SEED, dev)
    total = stream.numel() + 4 * n
    enc = spec_amd.Encoder(spec_amd.FLAT16, n, dev)
    s2, e2 = torch.empty_like(stream), torch.empty_like(ends)
    out_b, fe_b = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    out_c, fe_c = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    L = spec_amd.lib()

    def encode():
        enc.encode_into(d_cols, d_heaps, s2, e2)

    def two_pass():
        enc.encode_into(d_cols, d_heaps, s2, e2)
        rc = L.spec_frames_write(_p(s2), s2.numel(), _p(e2), n, _p(out_b), total, _p(fe_b),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def fused():
        enc.encode_frames_into(d_cols, d_heaps, out_c, fe_c)

    legs = {"encode": encode, "encode_then_frames_write": two_pass, "encode_frames": fused}
    seen = _alternate(legs, two_pass, rounds, reps)
    two_pass()
    fused()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out_c, out_b)) and bool(torch.equal(fe_c, fe_b)) and int(enc.total.item()) == total
    return _fused_result(seen, n, int(stream.numel()), total, rounds, reps, ok)


def _alternate(legs, warm, rounds, reps):
    """The legs timed in alternating rounds in one process -> {leg: [(mean, median, p10, p90)]}."""
    import bench

    bench.gpu_prewarm(warm)
    seen = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            seen[k].append(bench.kernel_time_events(fn, reps, lead=3, spread=True))
    return seen


def _fused_result(seen, n, stream_bytes, total, rounds, reps, ok):
    import statistics

    res = {"records": n, "stream_bytes": stream_bytes, "framed_bytes": int(total), "rounds": rounds,
           "reps_per_round": reps}
    for k, rs in seen.items():
        res[k] = {"mean_ms": round(statistics.mean(r[0] for r in rs), 4),
                  "median_ms": round(statistics.median(r[1] for r in rs), 4),
                  "p10_p90_ms": [round(min(r[2] for r in rs), 4), round(max(r[3] for r in rs), 4)],
                  "round_means_ms": [round(r[0], 4) for r in rs]}
    a, b, c = res["encode"], res["encode_then_frames_write"], res["encode_frames"]
    res["fused_over_encode"] = round(c["mean_ms"] / a["mean_ms"], 3)
    res["fused_over_two_pass"] = round(c["mean_ms"] / b["mean_ms"], 3)
    res["fused_p90_below_two_pass_p10"] = c["p10_p90_ms"][1] < b["p10_p90_ms"][0]
    res["ok"] = ok
    return res


def step_nested_fused(n, rounds=5, reps=20):
    """step_fused's three legs for the nested encoder on the bench's config-4 batch (bench.py
    nested_leg: workload.nested(n, SEED), the `_items` workspace): (a) spec_encode_nested, (b) that
    plus spec_frames_write, (c) spec_encode_nested_frames."""
    import numpy as np
    import torch

    import spec_amd
    from spec_amd import NESTED, workload

    dev = torch.device("cuda", 0)
    w = workload.nested(n, SEED)
    m = len(w["key"])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    outer = [to(w["id"]), to(w["seq"].view(np.uint8).reshape(n, 8)), to(w["name"].view(np.uint8).reshape(n, 8)), None]
    items = [to(w["key"].view(np.uint8).reshape(m, 4)), to(w["value"].view(np.uint8).reshape(m, 8)),
             to(w["label"].view(np.uint8).reshape(m, 8))]
    oh, ih, ib = {2: to(w["name_heap"])}, {2: to(w["label_heap"])}, to(w["item_begin"].view(np.int32))
    enc = spec_amd.NestedEncoder(NESTED, n, dev)
    sb = int(enc.encode(outer, oh, ib, items, ih, m).item())
    total = sb + 4 * n
    s2, e2 = torch.empty(sb, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    out_b, fe_b = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    out_c, fe_c = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    L = spec_amd.lib()

    def encode():
        enc.encode(outer, oh, ib, items, ih, m, s2, e2)

    def two_pass():
        enc.encode(outer, oh, ib, items, ih, m, s2, e2)
        rc = L.spec_frames_write(_p(s2), sb, _p(e2), n, _p(out_b), total, _p(fe_b),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def fused():
        enc.encode_frames(outer, oh, ib, items, ih, m, out_c, fe_c)

    legs = {"encode": encode, "encode_then_frames_write": two_pass, "encode_frames": fused}
    seen = _alternate(legs, two_pass, rounds, reps)
    two_pass()
    fused()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out_c, out_b)) and bool(torch.equal(fe_c, fe_b)) and int(enc.total.item()) == total
    res = _fused_result(seen, n, sb, total, rounds, reps, ok)
    res["items"] = m
    return res


def step_tree_fused(n, rounds=5, reps=20):
    """step_fused's three legs for the tree encoder on the bench's pkg1 batch (bench.py tree_leg:
    262,144 records whatever --n says): (a) spec_encode_tree, (b) that plus spec_frames_write,
    (c) spec_encode_tree_frames."""
    import numpy as np
    import torch

    import spec_amd
    from spec_amd import workload

    dev = torch.device("cuda", 0)
    n = TREE_N
    tree = spec_amd.pkg1_tree()
    cols, heaps, rows = workload.tree_batch(tree, n, 7)
    dc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cols.items()}
    dh = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in heaps.items()}
    enc = spec_amd.TreeEncoder(tree, rows, dev)
    sb = int(enc.encode(dc, dh, None, None).item())
    total = sb + 4 * n
    s2, e2 = torch.empty(sb, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    out_b, fe_b = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    out_c, fe_c = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    L = spec_amd.lib()

    def encode():
        enc.encode(dc, dh, s2, e2)

    def two_pass():
        enc.encode(dc, dh, s2, e2)
        rc = L.spec_frames_write(_p(s2), sb, _p(e2), n, _p(out_b), total, _p(fe_b),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def fused():
        enc.encode_frames(dc, dh, out_c, fe_c)

    legs = {"encode": encode, "encode_then_frames_write": two_pass, "encode_frames": fused}
    seen = _alternate(legs, two_pass, rounds, reps)
    two_pass()
    fused()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out_c, out_b)) and bool(torch.equal(fe_c, fe_b)) and int(enc.total.item()) == total
    return _fused_result(seen, n, sb, total, rounds, reps, ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", default="egress")
    ap.add_argument("--out", default=None, help="output directory (default profiles/<run>)")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", default=None, help="comma-separated steps to run (default: all); the output "
                                                  "file's other keys are kept")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print("EGRESS " + json.dumps(globals()["step_" + args.step](args.n)), flush=True)
        return 0
    out_dir = args.out or os.path.join(ROOT, "profiles", args.run)
    os.makedirs(out_dir, exist_ok=True)
    result = {"run": args.run, "records": args.n}
    only = args.steps.split(",") if args.steps else None
    path = os.path.join(out_dir, "egress.json")
    if only:
        unknown = [s for s in only if s not in dict(STEPS)]
        if unknown:
            ap.error(f"unknown steps {unknown}")
        if os.path.exists(path):
            with open(path) as f:
                result = {**json.load(f), **result}
    rc = 0
    for step, limit in STEPS:
        if only and step not in only:
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result[step] = {"error": f"no result within {limit} s"}
            rc = 1
            break
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("EGRESS ")), None)
        if r.returncode != 0 or line is None:
            result[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            rc = 1
            break
        result[step] = json.loads(line[7:])
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main())

"""Sparse flat batches (optional fields): 1M Flat16 records, every field present with p = 0.75,
beside the dense batch, through the build of the checkout ROOT.

  decode   spec_decode_flat on the dense and on the sparse batch (a build without
           spec_decode_flat_present — the parent commit — reports these two only: its sparse records
           leave the fast path for the generic one), spec_decode_flat_present on both;
  encode   spec_encode_flat (schema-specialised, dense) against spec_encode_flat_present (run-time
           kernels) with an all-ones mask and with the 0.75 mask; `ok`: the all-ones bytes equal the
           dense encoder's.

The sparse batch is built by this checkout's device encoder (a 4,096-record sample of it checked
against the oracle Writer) and, with --batch PREFIX, saved as PREFIX.{stream,ends,mask}.npy; a build
without the encoder loads it from there, so both builds decode the same bytes.

HIP events around every call, 5 rounds x 20 calls per leg after a warm-up, the legs alternating
round by round in one process: the median and the 10th / 90th percentiles of a leg's 100 intervals.
Prints one line "SPARSE {json}"; --out FILE also writes the json there.

    python tools/bench_sparse.py [ROOT] [LABEL] [--batch PREFIX] [--out FILE]

A/B against the parent: alternate the two checkouts' processes and compare decode.flat_sparse (parent)
with decode.present_sparse (this build) by the rule of DESIGN.md 9d.
"""
import json
import os
import sys

argv = [a for a in sys.argv[1:]]
OUT = BATCH = None
for flag in ("--out", "--batch"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--out":
            OUT = argv[i + 1]
        else:
            BATCH = argv[i + 1]
        del argv[i:i + 2]
ROOT = os.path.abspath(argv[0] if argv else os.path.join(os.path.dirname(__file__), ".."))
LABEL = argv[1] if len(argv) > 1 else "new"
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import spec_amd  # noqa: E402
from spec_amd import FLAT16, workload  # noqa: E402

assert os.path.dirname(spec_amd.LIB_PATH) == os.path.join(ROOT, "spec_amd"), spec_amd.LIB_PATH
HAVE = hasattr(spec_amd, "encode_flat_present")
ROUNDS, CALLS, N, P_PRESENT, SAMPLE = 5, 20, 1 << 20, 0.75, 4096
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream()
to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731


def measure(legs):
    """{leg: {median, p10, p90, mean, round_means}} in ms; the legs take turns round by round."""
    for fn in legs.values():
        bench.gpu_prewarm(fn, 0.2)
    ms = {k: [] for k in legs}
    means = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            for _ in range(3):
                fn()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
            for x, y in evs:
                x.record(s)
                fn()
                y.record(s)
            torch.cuda.synchronize()
            t = [x.elapsed_time(y) for x, y in evs]
            ms[k] += t
            means[k].append(sum(t) / len(t))
    r4 = lambda v: round(v, 4)  # noqa: E731
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"median_ms": r4(v[len(v) // 2]), "p10_ms": r4(v[len(v) // 10]), "p90_ms": r4(v[9 * len(v) // 10]),
                  "mean_ms": r4(sum(v) / len(v)), "round_means_ms": [r4(m) for m in means[k]]}
    return out


res = {"build": LABEL, "records": N, "p_present": P_PRESENT, "rounds": ROUNDS, "calls_per_round": CALLS}
cols, heaps = workload.flat16(N, 0x5EC0DE)
d_cols = [to(c) for c in cols]
d_heaps = {f: to(h) for f, h in heaps.items()}
dense, dense_ends = spec_amd.encode_flat(FLAT16, d_cols, d_heaps, N)
nf = len(FLAT16)

if HAVE:
    bits = np.random.default_rng(0x5EC0DE).random((N, nf)) < P_PRESENT
    mask = np.zeros(N, np.uint64)
    for f in range(nf):
        mask |= bits[:, f].astype(np.uint64) << np.uint64(f)
    d_mask = to(mask.view(np.int64))
    d_ones = torch.full((N,), (1 << nf) - 1, dtype=torch.int64, device=dev)
    sparse, sparse_ends = spec_amd.encode_flat_present(FLAT16, d_cols, d_heaps, d_mask, N)
    torch.cuda.synchronize()
    # a sample of the sparse batch against the oracle Writer (only the setters of each record's mask)
    sys.path.insert(0, ROOT)
    from tests.present_helpers import write_sparse  # noqa: E402

    want = b"".join(write_sparse(FLAT16, [c[:SAMPLE] for c in cols], heaps, bits[:SAMPLE], SAMPLE))
    got = sparse[: int(sparse_ends[SAMPLE - 1])].cpu().numpy().tobytes()
    res["sample_records"] = SAMPLE
    res["sample_ok"] = got == want
    if BATCH:
        os.makedirs(os.path.dirname(os.path.abspath(BATCH)), exist_ok=True)
        np.save(BATCH + ".stream.npy", sparse.cpu().numpy())
        np.save(BATCH + ".ends.npy", sparse_ends.cpu().numpy())
        np.save(BATCH + ".mask.npy", mask)
else:
    sparse, sparse_ends = to(np.load(BATCH + ".stream.npy")), to(np.load(BATCH + ".ends.npy"))
    mask = np.load(BATCH + ".mask.npy")
res["dense_bytes"], res["sparse_bytes"] = int(dense.numel()), int(sparse.numel())

# ---- decode ---------------------------------------------------------------------------------------
L = spec_amd.lib()
import ctypes as C  # noqa: E402

out_cols = spec_amd.alloc_columns(FLAT16, N, dev)
status = torch.empty(N, dtype=torch.uint8, device=dev)
pm = torch.zeros(N, dtype=torch.int64, device=dev)
ptrs = (C.c_void_p * nf)(*[c.data_ptr() for c in out_cols])
vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def flat(stream, ends):
    return lambda: L.spec_decode_flat(C.byref(FLAT16.c), vp(stream), stream.numel(), vp(ends), N, ptrs, vp(status), None)


def present(stream, ends):
    return lambda: L.spec_decode_flat_present(C.byref(FLAT16.c), vp(stream), stream.numel(), vp(ends), N, ptrs,
                                              vp(status), None, vp(pm), None)


legs = {"flat_dense": flat(dense, dense_ends), "flat_sparse": flat(sparse, sparse_ends)}
if HAVE:
    legs["present_dense"] = present(dense, dense_ends)
    legs["present_sparse"] = present(sparse, sparse_ends)
res["decode"] = measure(legs)
ok = {}
legs["flat_sparse"]()
torch.cuda.synchronize()
ok["flat_sparse_status"] = int(status.sum()) == 0
ref = [c.clone() for c in out_cols]
if HAVE:
    legs["present_sparse"]()
    torch.cuda.synchronize()
    ok["present_sparse"] = (int(status.sum()) == 0 and bool((pm.cpu().numpy().view(np.uint64) == mask).all())
                            and all(torch.equal(a, b) for a, b in zip(out_cols, ref)))
    legs["present_dense"]()
    torch.cuda.synchronize()
    ok["present_dense"] = int(status.sum()) == 0 and bool((pm == (1 << nf) - 1).all())
res["decode"]["ok"] = ok

# ---- encode ---------------------------------------------------------------------------------------
if HAVE:
    enc = spec_amd.Encoder(FLAT16, N, dev)
    out = torch.empty(dense.numel() + 64, dtype=torch.uint8, device=dev)
    ends = torch.empty(N, dtype=torch.int64, device=dev)
    elegs = {"dense_specialised": lambda: enc.encode_into(d_cols, d_heaps, out, ends),
             "present_all_ones": lambda: enc.encode_present_into(d_cols, d_heaps, d_ones, out, ends),
             "present_p75": lambda: enc.encode_present_into(d_cols, d_heaps, d_mask, out, ends)}
    res["encode"] = measure(elegs)
    elegs["present_all_ones"]()
    torch.cuda.synchronize()
    res["encode"]["ok"] = bool(torch.equal(out[: dense.numel()], dense) and torch.equal(ends, dense_ends))

print("SPARSE " + json.dumps(res), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)

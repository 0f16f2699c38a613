"""spec_lz4_compress_frame on the bench's batch: 1M Flat16 records as mpx frames (272 MB, 1,037
blocks of 256 KiB) compressed as one call — mean, median, p10-p90 and input GB/s of the call over
5 rounds x 20 launches (HIP events, one process); the payload ratio next to the oracle's on the
same bytes; the host path the call replaces (the oracle's block compressor over the same blocks
on 16 threads, in the same process); spec_lz4_decompress + spec_lz4_pack over the device-written
frame; and the ratios on the `chunks` and `mixed` data of the GPU tests, whose matches lie up to
a block back.  Writes profiles/<run>/lz4_compress.json.

Every GPU step is a child process of its own under a time limit; a step that fails or runs out
of time ends the run (nothing more is started on the GPU).

    python tools/bench_lz4_compress.py [--run NAME] [--out DIR] [--n RECORDS]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("compress", 420), ("ratios", 120))
SEED = 0x5EC0DE
BM = 256 << 10
HOST_THREADS = 16


def _p(t):
    return C.c_void_p(t.data_ptr())


def _payload(frame, start=7):
    """-> (payload bytes, blocks, stored blocks) of a frame's block records"""
    import numpy as np

    p, pay, nb, st = start, 0, 0, 0
    while p + 4 <= frame.size:
        w = int(np.frombuffer(frame[p:p + 4].tobytes(), "<u4")[0])
        if w == 0:
            break
        pay += w & 0x7FFFFFFF
        nb += 1
        st += w >> 31
        p += 4 + (w & 0x7FFFFFFF)
    return pay, nb, st


def _host_compress(data, threads):
    """The oracle's block compressor over data's 256 KiB blocks on `threads` threads -> (payload
    bytes as the frame writer would keep them, seconds)"""
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    from oracle import oracle as O

    L = O.lib()
    nb = (data.size + BM - 1) // BM
    cap = BM + BM // 255 + 64
    outs = [np.empty(cap, np.uint8) for _ in range(threads)]
    sizes = np.zeros(nb, np.int64)
    base = data.ctypes.data

    def work(t):
        o = outs[t]
        for k in range(t, nb, threads):
            bn = min(BM, data.size - k * BM)
            c = L.so_lz4_compress_block(C.c_void_p(base + k * BM), bn, C.c_void_p(o.ctypes.data), bn - 1)
            sizes[k] = bn if c < 0 else c

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(work, range(threads)))
        dt = time.perf_counter() - t0
    return int(sizes.sum()), dt


def step_compress(n, rounds=5, reps=20):
    import numpy as np
    import torch

    import bench
    import spec_amd
    from spec_amd.lz4 import OPEN, compress_frame_into, frame_blocks, frame_bound

    dev = torch.device("cuda", 0)
    _, _, _, _, stream, ends = bench.make_batch(n, SEED, dev)
    frames = spec_amd.make_frames_device(stream, ends)
    nbytes = frames.numel()
    L = spec_amd.lib()
    out = torch.empty(frame_bound(nbytes, BM, OPEN), dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.spec_lz4_compress_workspace_size(nbytes, BM), dtype=torch.uint8, device=dev)

    def compress():
        compress_frame_into(frames, out, total, BM, OPEN, workspace=ws)

    bench.gpu_prewarm(compress)
    seen = [bench.kernel_time_events(compress, reps, lead=3, spread=True) for _ in range(rounds)]
    compress()
    torch.cuda.synchronize()
    first = out[:int(total.item())].cpu().numpy().copy()
    compress()
    torch.cuda.synchronize()
    frame = out[:int(total.item())].cpu().numpy()
    same = bool(np.array_equal(first, frame))
    pay, nb, stored = _payload(frame)
    mean = statistics.mean(r[0] for r in seen)
    res = {"records": n, "input_bytes": int(nbytes), "blocks": nb, "stored_blocks": int(stored), "block_max": BM,
           "rounds": rounds, "reps_per_round": reps,
           "compress": {"mean_ms": round(mean, 4), "median_ms": round(statistics.median(r[1] for r in seen), 4),
                        "p10_p90_ms": [round(min(r[2] for r in seen), 4), round(max(r[3] for r in seen), 4)],
                        "round_means_ms": [round(r[0], 4) for r in seen],
                        "input_gb_s": round(nbytes / (mean * 1e-3) / 1e9, 2)},
           "frame_bytes": int(frame.size), "payload_bytes": int(pay), "payload_ratio": round(pay / nbytes, 4),
           "workspace_bytes": int(ws.numel()), "same_bytes_twice": same}

    # the receive half over the device-written frame
    blocks, used, bmax, rc = frame_blocks(frame)
    assert rc == 0 and used == frame.size and len(blocks) == nb
    d_frame = torch.from_numpy(frame).to(dev)
    d_blocks = torch.from_numpy(np.ascontiguousarray(blocks).view(np.uint8).copy()).to(dev)
    slots = torch.empty(nb * BM, dtype=torch.uint8, device=dev)
    sizes = torch.empty(nb, dtype=torch.int32, device=dev)
    status = torch.empty(nb, dtype=torch.uint8, device=dev)
    plain = torch.empty(nb * BM, dtype=torch.uint8, device=dev)
    pws = torch.empty(L.spec_lz4_pack_workspace_size(nb) // 8 + 1, dtype=torch.int64, device=dev)
    ptotal = torch.zeros(1, dtype=torch.int64, device=dev)

    def receive():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.spec_lz4_decompress(_p(d_frame), d_frame.numel(), _p(d_blocks), nb, _p(slots), BM, _p(sizes),
                                     _p(status), s) == 0
        assert L.spec_lz4_pack(_p(slots), BM, _p(sizes), nb, _p(plain), plain.numel(), _p(ptotal), _p(pws),
                               pws.numel() * 8, s) == 0

    r_ms, r_med, r_lo, r_hi = bench.kernel_time_events(receive, reps, lead=3, spread=True)
    torch.cuda.synchronize()
    res["round_trip_ok"] = bool(int(ptotal.item()) == nbytes and torch.equal(plain[:nbytes], frames))
    res["decompress_pack_of_device_frame"] = {"mean_ms": round(r_ms, 4), "median_ms": round(r_med, 4),
                                              "p10_p90_ms": [round(r_lo, 4), round(r_hi, 4)],
                                              "of_oracle_frame_ms_design_8": 2.1}

    # the host path the call replaces: the oracle's compressor, 16 threads
    host = frames.cpu().numpy()
    _host_compress(host[: 32 * BM], HOST_THREADS)  # warm: threads, the oracle library
    times, opay = [], 0
    for _ in range(7):
        opay, dt = _host_compress(host, HOST_THREADS)
        times.append(dt * 1e3)
    times.sort()
    res["host_oracle_16_threads"] = {"mean_ms": round(statistics.mean(times), 2), "median_ms": round(statistics.median(times), 2),
                                     "p10_p90_ms": [round(times[0], 2), round(times[-1], 2)], "runs": len(times),
                                     "threads": HOST_THREADS, "input_gb_s": round(nbytes / (statistics.mean(times) * 1e-3) / 1e9, 2)}
    res["oracle_payload_bytes"] = int(opay)
    res["oracle_payload_ratio"] = round(opay / nbytes, 4)
    res["device_p90_below_host_p10"] = res["compress"]["p10_p90_ms"][1] < times[0]
    res["ok"] = res["round_trip_ok"] and same
    return res


def step_ratios(n):
    """Payload ratios, device next to oracle, on data whose matches lie up to a whole block back
    (spec_amd.workload.lz4_data `chunks`, `mixed`) and on the kinds the ratio floor covers."""
    import numpy as np
    import torch

    from oracle import oracle as O
    from spec_amd.lz4 import compress_frame
    import spec_amd
    from spec_amd import FLAT16, workload

    dev = torch.device("cuda", 0)
    res = {}
    for kind in ("chunks", "mixed", "text", "zeros", "period200", "flat16"):
        if kind == "flat16":  # 4,000 records as mpx frames
            cols, heaps = workload.flat16(4000, seed=12)
            stream, ends = O.encode_flat_batch(FLAT16.tags, FLAT16.kinds, cols, [heaps.get(f) for f in range(16)], 4000)
            data = spec_amd.make_frames(stream, ends)
        else:
            data = workload.lz4_data(kind, 300_000)
        f = compress_frame(torch.from_numpy(data.copy()).to(dev), BM).cpu().numpy()
        pay, nb, stored = _payload(f)
        opay = sum(min(len(O.lz4_compress_block(data[k:k + BM])), data[k:k + BM].size) for k in range(0, data.size, BM))
        rc, got, used = O.lz4_frame_read(f, data.size + 16)
        res[kind] = {"bytes": int(data.size), "device_payload": int(pay), "oracle_payload": int(opay),
                     "device_ratio": round(pay / data.size, 4), "oracle_ratio": round(opay / data.size, 4),
                     "stored_blocks": int(stored), "blocks": nb, "ok": bool(rc == 0 and np.array_equal(got, data))}
    res["ok"] = all(v["ok"] for v in res.values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", default="egress")
    ap.add_argument("--out", default=None, help="output directory (default profiles/<run>)")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print("LZ4C " + json.dumps(globals()["step_" + args.step](args.n)), flush=True)
        return 0
    out_dir = args.out or os.path.join(ROOT, "profiles", args.run)
    os.makedirs(out_dir, exist_ok=True)
    result = {"run": args.run, "records": args.n}
    rc = 0
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result[step] = {"error": f"no result within {limit} s"}
            rc = 1
            break
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LZ4C ")), None)
        if r.returncode != 0 or line is None:
            result[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            rc = 1
            break
        result[step] = json.loads(line[5:])
        if not result[step].get("ok"):
            rc = 1
            break
    with open(os.path.join(out_dir, "lz4_compress.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main())

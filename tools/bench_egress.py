"""The send path on the bench's 1M Flat16 records (272 MB framed): spec_frames_write against a
device-to-device copy of the same bytes in the same run.  Writes profiles/<run>/egress.json.

Every GPU step is a child process of its own under a time limit; a step that fails or runs out
of time ends the run (nothing more is started on the GPU).

    python tools/bench_egress.py [--run NAME] [--out DIR] [--n RECORDS]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("frames", 240),)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", default="egress")
    ap.add_argument("--out", default=None, help="output directory (default profiles/<run>)")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print("EGRESS " + json.dumps(globals()["step_" + args.step](args.n)), flush=True)
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
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("EGRESS ")), None)
        if r.returncode != 0 or line is None:
            result[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            rc = 1
            break
        result[step] = json.loads(line[7:])
    with open(os.path.join(out_dir, "egress.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main())

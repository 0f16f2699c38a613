"""Concurrent host callers (include/spec_amd.h, Conventions: the functions may be called from several threads).

Four Python threads call into libspec_amd.so at once (ctypes releases the GIL for the length of a call, so
the C side really runs concurrently), each on its own torch.cuda.Stream with its own batches and output
buffers.  What they share is what the library shares between callers: the cache of schema-specialised
modules (jit_module.cpp find_module, one key asked for by all four), the thread_local lookup rings in front
of it (jit.cpp) and the code-object cache on disk.  The per-device pool of pinned upload slots (capi.hip
spec::pinned_upload, fed by the wide flat encoder, the tree encoder and the wide nested encoder) is NOT
contended here: no thread encodes through it, because several wide flat encodes in flight
aborted the process on the MI355X (tests/test_gpu_streams.py test_wide_decodes_in_flight) and that cause
comes first.  No thread touches the process-wide switches (set_jit,
spec_set_nested_mode).  Every result is compared bit for bit with the CPU oracle's, computed on the main
thread beforehand.
"""
from __future__ import annotations

import functools
import os
import threading
import time
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, Kind, Schema, workload
from spec_amd.tree import TreeDecoder
from tests.gpu_helpers import require_specialised, to_dev
from tests.stream_helpers import (ALL_KINDS, _stop_on_gpu_error, parse_case, tree_collect, tree_columns_out, tree_want,  # noqa: F401
                                  u8)
from tests.tree_helpers import oracle_decode, oracle_encode

pytestmark = pytest.mark.gpu

THREADS, ITERATIONS, N = 4, 20, 500
PRIVATE = ["n8", "n9", "n17p", "n18"]  # workload.shape_sweep_schemas: one per thread (modules built by build())


def slab_columns(widths, n, dev):
    """Columns of n rows carved from one allocation (one copy brings a call's outputs to the host)."""
    slab = torch.zeros(sum(widths) * n + n, dtype=torch.uint8, device=dev)
    cols, p = [], 0
    for w in widths:
        cols.append(slab[p:p + n * w].view(n, w))
        p += n * w
    return slab, cols, slab[p:p + n]


def slab_want(cols, status):
    return np.concatenate([u8(c) for c in cols] + [u8(status)])


@functools.lru_cache(maxsize=None)
def thread_data(k):
    """Thread k's batches and the oracle's answers (host only)."""
    sweep = workload.shape_sweep_schemas()
    d = NS(k=k)
    d.private = sweep[PRIVATE[k]]
    cols, heaps = workload.gen_columns(d.private, N, seed=200 + k, str_len=(0, 20))
    d.p_stream, d.p_ends = O.encode_flat_batch(d.private.tags, d.private.kinds, cols,
                                               [heaps.get(f) for f in range(len(d.private))], N)
    d.p_want = slab_want(*O.decode_flat_batch(d.private.tags, d.private.kinds, d.p_stream, d.p_ends, d.private.widths))
    # Flat16: encoded by the thread, and its bytes decoded with the schema every thread shares
    d.f_cols, d.f_heaps = workload.flat16(N, seed=300 + k)
    d.f_stream, d.f_ends = O.encode_flat_batch(FLAT16.tags, FLAT16.kinds, d.f_cols, [d.f_heaps.get(f) for f in range(16)], N)
    d.f_want = slab_want(*O.decode_flat_batch(FLAT16.tags, FLAT16.kinds, d.f_stream, d.f_ends, FLAT16.widths))
    # more than 64 fields: the chunked decode
    d.wide = Schema([(2 * i + 1 + k, ALL_KINDS[(i + 3 * k) % 15]) for i in range(70)])
    d.w_cols, d.w_heaps = workload.gen_columns(d.wide, N, seed=400 + k, str_len=(0, 10))
    d.w_stream, d.w_ends = O.encode_flat_batch(d.wide.tags, d.wide.kinds, d.w_cols, [d.w_heaps.get(f) for f in range(70)], N)
    d.w_want = slab_want(*O.decode_flat_batch(d.wide.tags, d.wide.kinds, d.w_stream, d.w_ends, d.wide.widths))
    # validation: thread 0 and 2 the batch with deep records, 1 and 3 its reverse
    pc = parse_case("parse_messages", "-")
    d.v_in, d.v_want = (pc.real, pc.want) if k % 2 == 0 else (pc.decoy, pc.want_decoy)
    # a schema tree
    d.tree = spec_amd.pkg1_tree()
    tcols, theaps, _ = workload.tree_batch(d.tree, 200, 500 + k, count=(0, 3))
    d.t_stream, d.t_ends = oracle_encode(d.tree, tcols, theaps, 200)
    rows, want = oracle_decode(d.tree, d.t_stream, d.t_ends)
    d.t = NS(tree=d.tree, rows=rows, want=want)
    return d


class Worker:
    """Thread k's device state (built on the main thread) and its loop."""

    def __init__(self, k, dev):
        d = self.d = thread_data(k)
        self.s = torch.cuda.Stream()
        dv = lambda a: to_dev(a if a.size else np.zeros(1, np.uint8), dev)  # noqa: E731
        self.p_in = (dv(d.p_stream), dv(d.p_ends.view(np.int64)))
        self.f_in = (dv(d.f_stream), dv(d.f_ends.view(np.int64)))
        self.w_in = (dv(d.w_stream), dv(d.w_ends.view(np.int64)))
        self.p_out, self.f_out, self.w_out = (slab_columns(sc.widths, N, dev) for sc in (d.private, FLAT16, d.wide))
        self.e_cols = [dv(c) for c in d.f_cols]
        self.e_heaps = {f: dv(h) for f, h in d.f_heaps.items()}
        self.enc = spec_amd.Encoder(FLAT16, N, dev)
        self.e_out = torch.zeros(d.f_stream.size, dtype=torch.uint8, device=dev)
        self.e_ends = torch.zeros(N, dtype=torch.int64, device=dev)
        self.v_in = (dv(d.v_in["stream"]), dv(d.v_in["ends"]))
        self.td = TreeDecoder(d.tree)
        self.td.reserve(d.t.rows)
        self.t_in = (dv(d.t_stream), dv(d.t_ends.view(np.int64)))
        self.t_g, self.t_cols = tree_columns_out(d.tree, d.t.rows, dev)
        self.t_rows = torch.zeros(len(d.tree.tables), dtype=torch.int64, device=dev)
        self.t_caps = self.td.column_capacity(self.t_cols)
        self.t_want = tree_want(NS(tree=d.tree, want=d.t.want, rows=d.t.rows), False)

    def clear(self):
        with torch.cuda.stream(self.s):
            for t in (self.p_out[0], self.f_out[0], self.w_out[0], self.e_out, self.e_ends, self.t_rows, self.enc.total):
                t.zero_()
            for g in self.t_g:
                g.t.zero_()

    def iteration(self, it):
        d, s = self.d, self.s
        self.clear()
        spec_amd.decode_flat(d.private, *self.p_in, cols=self.p_out[1], status=self.p_out[2], cuda_stream=s)
        spec_amd.decode_flat(FLAT16, *self.f_in, cols=self.f_out[1], status=self.f_out[2], cuda_stream=s)
        spec_amd.decode_flat(d.wide, *self.w_in, cols=self.w_out[1], status=self.w_out[2], cuda_stream=s)
        self.enc.encode_into(self.e_cols, self.e_heaps, self.e_out, self.e_ends, s)
        st, sz = spec_amd.parse_messages(*self.v_in, cuda_stream=s)
        self.td.run(*self.t_in, self.t_cols, self.t_rows, s, self.t_caps)
        s.synchronize()
        where = f"thread {d.k}, iteration {it}: "
        for name, out, want in (("private", self.p_out, d.p_want), ("shared", self.f_out, d.f_want),
                                ("wide", self.w_out, d.w_want)):
            assert np.array_equal(out[0].cpu().numpy(), want), where + f"{name}-schema decode differs from the oracle"
        for name, enc, out, ends, ws, we in (("flat", self.enc, self.e_out, self.e_ends, d.f_stream, d.f_ends),):
            assert int(enc.total.item()) == ws.size, where + f"{name} encode total"
            assert np.array_equal(ends.cpu().numpy(), we.view(np.int64)), where + f"{name} encode ends"
            assert np.array_equal(out.cpu().numpy(), ws), where + f"{name} encode bytes"
        assert np.array_equal(st.cpu().numpy(), d.v_want["status"]), where + "parse status"
        assert np.array_equal(u8(sz.cpu().numpy()), u8(d.v_want["sizes"])), where + "parse sizes"
        got = tree_collect(d.tree, d.t.rows, self.t_g, self.t_rows)
        for name, w in self.t_want.items():
            assert np.array_equal(u8(got[name]), u8(w)), where + f"tree column {name}"

    def loop(self, iterations=ITERATIONS):
        for it in range(iterations):
            self.iteration(it)


def run_threads(targets, timeout):
    """Run the callables on a thread each; a thread that has not finished `timeout` seconds after the start
    fails the test (it is a daemon: it does not keep the process), and the first exception raised in a thread
    is raised again here."""
    errors = [None] * len(targets)

    def wrap(i, fn):
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 (re-raised on the main thread)
            errors[i] = e

    threads = [threading.Thread(target=wrap, args=(i, fn), daemon=True) for i, fn in enumerate(targets)]
    t0 = time.monotonic()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, timeout - (time.monotonic() - t0)))
    hung = [i for i, t in enumerate(threads) if t.is_alive()]
    for e in errors:
        if e is not None:
            raise e
    assert not hung, f"threads {hung} had not finished after {timeout:.0f} s"


def test_four_threads(dev):
    workers = [Worker(k, dev) for k in range(THREADS)]
    torch.cuda.synchronize()
    require_specialised(FLAT16, "Flat16", decode=(workers[0].d.f_stream.size, N), encode=True)
    for w in workers:  # everything works from the main thread first (and every module is loaded)
        w.loop(1)
    t0 = time.monotonic()
    workers[0].loop()
    single = time.monotonic() - t0
    # four loops at once, on hardware and a host library they share: a generous multiple of one loop alone
    run_threads([w.loop for w in workers], timeout=10.0 + 8 * THREADS * single)
    torch.cuda.synchronize()


def test_cold_cache_compiles(dev):
    """Two threads ask for the same never-seen schema at the same moment, two more for one new schema each
    (tags from the process id: no code-object cache holds them): one compile per schema, every caller gets
    the specialised kernels and the oracle's answer.  (The one test here that takes as long as a few hiprtc
    compiles.)"""
    base = 300 + 40 * (os.getpid() % 1500)
    kinds = [Kind.INT32, Kind.STRING, Kind.UINT64, Kind.BIN64, Kind.INT16]
    schemas = [Schema([(base + 7 * j + i, kinds[(i + j) % 5]) for i in range(4)]) for j in range(3)]
    jobs = []
    for t, sc in enumerate([schemas[0], schemas[0], schemas[1], schemas[2]]):
        cols, heaps = workload.gen_columns(sc, N, seed=600 + t, str_len=(0, 20))
        stream, ends = O.encode_flat_batch(sc.tags, sc.kinds, cols, [heaps.get(f) for f in range(len(sc))], N)
        want = slab_want(*O.decode_flat_batch(sc.tags, sc.kinds, stream, ends, sc.widths))
        jobs.append(NS(schema=sc, stream=stream, want=want, s=torch.cuda.Stream(), out=slab_columns(sc.widths, N, dev),
                       d_in=(to_dev(stream, dev), to_dev(ends.view(np.int64), dev))))
    torch.cuda.synchronize()
    start = threading.Barrier(len(jobs))

    def call(j):
        start.wait(30)
        spec_amd.decode_flat(j.schema, *j.d_in, cols=j.out[1], status=j.out[2], cuda_stream=j.s)
        j.s.synchronize()

    run_threads([functools.partial(call, j) for j in jobs], timeout=240.0)
    for t, j in enumerate(jobs):
        require_specialised(j.schema, f"cold schema of thread {t}", decode=(j.stream.size, N))
        assert np.array_equal(j.out[0].cpu().numpy(), j.want), f"thread {t}: decode differs from the oracle"
    # and through the loaded modules once more, all four at once
    for j in jobs:
        j.out[0].zero_()
    torch.cuda.synchronize()
    run_threads([functools.partial(call, j) for j in jobs], timeout=60.0)
    for t, j in enumerate(jobs):
        assert np.array_equal(j.out[0].cpu().numpy(), j.want), f"thread {t}: second decode differs from the oracle"

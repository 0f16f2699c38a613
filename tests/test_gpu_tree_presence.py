"""Schema trees with optional fields on the GPU (SPEC_TREE_FIELD_OPTIONAL, the HASMASK column),
through the generated kernels and the run-time kernels alike, against the three references of
tests/tree_presence_helpers.py (all built on the committed oracle):

  1. T = T'.plain(): every non-HASMASK column of a decode, and the encode at all-ones masks;
  2. the pruned tree: the encode at a uniform mask;
  3. the record walker: the encode at mixed masks, and every HASMASK word of a decode.

The last test is what the feature exists for: decode then encode of a stream whose writers skipped
setters is byte-exact with the presence tree, and is not with the plain tree.
"""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import spec_amd
from oracle import oracle as O
from oracle.tree_oracle import mismatches, oracle_decode, oracle_encode
from spec_amd import Kind, workload
from spec_amd.tree import REL_ONE, ROLE_HASMASK, ROLE_VALUE, TreeDecoder, TreeEncoder
from tests import tree_presence_helpers as H
from tests.tree_presence_helpers import fuzz, root_windows, to_dev

pytestmark = pytest.mark.gpu

CANARY, ECANARY = 0xA5, -0x5A5A5A5A5A5A5A5B
SIZES = {"presence_small": [1, 64, 65, 300, 5000], "pkg1": [1, 64, 65, 300, 5000], "presence_wide": [1, 65, 300]}
MASKS = ["ones", "zeros", "half", "uniform"]
UNIFORM = lambda t, k, f: (k + t) % 3 != 1  # noqa: E731  (the same in every row of every table)


@pytest.fixture(params=["jit", "runtime"])
def kernel(request):
    """The generated tree kernels (hiprtc) and the run-time tree kernels.  spec_encode_tree looks
    its kernels up per call, a TreeDecoder once: every case builds its decoders after this."""
    spec_amd.set_jit(request.param == "jit")
    yield request.param
    spec_amd.set_jit(True)


@pytest.fixture(autouse=True)
def _stop_on_gpu_error():
    """A HIP error left behind by a test ends the session: nothing more is launched after it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU error after a tree presence test: {e}", returncode=3)


# ---- expected results, computed once and shared (never modified) -----------------------------------

@functools.lru_cache(maxsize=None)
def case(name, n, masks, seed=None, **kw):
    """Columns of tree `name` with the masks asked for, and the expected bytes by the reference the
    masks allow: ones -> 1, uniform -> 2, zeros and half -> 3."""
    tree = H.tree_of(name)
    seed = 1000 + n if seed is None else seed
    kw = dict(kw) or dict(count=(0, 3))
    cols, heaps, rows = workload.tree_batch(tree, n, seed=seed, has=0.5 if masks == "half" else 1.0, **kw)
    if masks == "ones":
        stream, ends = oracle_encode(tree.plain(), cols, heaps, n)
    elif masks == "uniform":
        cols = H.set_masks(tree, cols, UNIFORM)
        stream, ends = oracle_encode(H.pruned(tree, UNIFORM), cols, heaps, n)
    else:
        if masks == "zeros":
            cols = H.set_masks(tree, cols, lambda t, k, f: False)
        stream, ends = H.walk_encode(tree, cols, heaps, n)
    return SimpleNamespace(tree=tree, n=n, cols=cols, heaps=heaps, rows=rows, stream=stream, ends=ends)


def gpu_encode(tree, cols, heaps, n, rows, dev, frames=False):
    fn = spec_amd.encode_tree_frames if frames else spec_amd.encode_tree
    s, e = fn(tree, to_dev(cols, dev), to_dev(heaps, dev), n, rows=rows)
    torch.cuda.synchronize()
    return s.cpu().numpy(), e.cpu().numpy().view(np.uint64)


def assert_bytes(got, got_ends, want, want_ends):
    assert np.array_equal(got_ends, want_ends), "ends"
    if not np.array_equal(got, want):
        j = int(np.nonzero(got != want)[0][0]) if got.size == want.size else -1
        raise AssertionError(f"encoded bytes: {got.size} bytes, expected {want.size}, first difference at {j}")


def gpu_decode(tree, stream, ends, dev):
    s = torch.from_numpy(np.ascontiguousarray(stream) if stream.size else np.zeros(1, np.uint8)).to(dev)[: stream.size]
    e = torch.from_numpy(np.ascontiguousarray(ends).view(np.int64)).to(dev)
    out = spec_amd.decode_tree(tree, s, e)
    torch.cuda.synchronize()
    return out.rows, [c.cpu().numpy() for c in out.cols]


def masks_in(tree, got):
    """{table: uint64 [rows, W]} of decoded columns."""
    return {c.table: np.ascontiguousarray(g).view(np.uint64).reshape(-1, c.width // 8)
            for c, g in zip(tree.columns, got) if c.role == ROLE_HASMASK}


def check_decode(tree, stream, ends, dev, want_rows=None):
    """A fresh decoder's decode of (stream, ends) with T': reference 1 for every other column,
    reference 3 for the HASMASK words, the MESSAGE / LIST bits equal to the PRESENT bytes."""
    plain = tree.plain()
    p_rows, p_want = oracle_decode(plain, stream, ends)
    rows, got = gpu_decode(tree, stream, ends, dev)
    assert rows == p_rows and (want_rows is None or rows == want_rows)
    assert mismatches(plain, H.without_hasmask(tree, got), p_want) == []
    want, have = H.walk_masks(tree, stream, ends, rows), masks_in(tree, got)
    assert set(want) == set(have)
    for x in want:
        assert np.array_equal(have[x], want[x]), f"HASMASK of table {x}"
        for k, i in enumerate(H.direct_fields(tree, x)):
            f = tree.fields[i]
            if f.kind in (Kind.MESSAGE, Kind.LIST):
                pres = got[tree.by_name[f"{f.path}?"].index].reshape(-1)
                assert np.array_equal((have[x][:, k // 64] >> np.uint64(k % 64)) & np.uint64(1), pres), f.path
        nd = len(H.direct_fields(tree, x))
        top = have[x][:, nd // 64] >> np.uint64(nd % 64) if nd % 64 else np.zeros(1, np.uint64)
        assert not np.any(top), "bits at or above the field count"
    return rows, got


def cache_files():
    dirs = [os.path.join(os.path.dirname(spec_amd.LIB_PATH), "jit_cache"),
            os.path.join(os.environ.get("XDG_CACHE_HOME", os.path.join(os.path.expanduser("~"), ".cache")), "spec_amd")]
    return {os.path.join(d, f) for d in dirs if os.path.isdir(d) for f in os.listdir(d)}


# ---- the precompiled modules ---------------------------------------------------------------------

def test_precompiled_trees_are_loaded_not_compiled(dev):
    """(first in the file) build() precompiled the three presence trees: their first use adds no
    code object to the cache."""
    spec_amd.set_jit(True)
    before = cache_files()
    assert before, "no code-object cache: run build()"
    for name in SIZES:
        b = case(name, 65, "half")
        s, e = gpu_encode(b.tree, b.cols, b.heaps, b.n, b.rows, dev)
        assert_bytes(s, e, b.stream, b.ends)
        check_decode(b.tree, b.stream, b.ends, dev, b.rows)
    assert cache_files() == before, sorted(cache_files() - before)


# ---- encode and decode over the sizes and masks -----------------------------------------------------

@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("name,n", [(name, n) for name, ns in SIZES.items() for n in ns])
def test_encode_decode(dev, kernel, name, n, masks):
    b = case(name, n, masks)
    if name == "presence_wide":
        assert len(H.direct_fields(b.tree, 0)) > 64  # the run-time group kernel, the over-64 generated writer
    s, e = gpu_encode(b.tree, b.cols, b.heaps, b.n, b.rows, dev)
    assert_bytes(s, e, b.stream, b.ends)
    if masks == "zeros" and name == "presence_wide":  # a row with nothing written is 00 00 50
        st = np.concatenate([[0], b.ends[:-1]]).astype(np.int64)
        for r in np.nonzero(b.cols["sub?"].reshape(-1) == 0)[0]:
            assert bytes(b.stream[st[r]: int(b.ends[r])]) == b"\x00\x00\x50"
    check_decode(b.tree, b.stream, b.ends, dev, b.rows)


def test_big_and_small_tables_alternate_in_a_wave(dev, kernel):
    """Tag 300 present in every other record: IsBigMessage per row, big and small tables side by
    side in one wave, on encode and on decode (a big table leaves the generated fast path)."""
    b = case("presence_small", 300, "ones", seed=31)
    tree = b.tree
    k = [tree.fields[i].tag for i in H.direct_fields(tree, 0)].index(300)
    cols = dict(b.cols)
    m = H.mask_of(cols, tree, 0).copy()
    m[1::2, 0] &= ~(np.uint64(1) << np.uint64(k))
    cols["#hasmask"] = m.view(np.uint8).reshape(-1, 8)
    want, wends = H.walk_encode(tree, cols, b.heaps, b.n)
    types = want[wends.astype(np.int64) - 1]
    assert set(types[0::2]) == {0x51} and set(types[1::2]) == {0x50}, "big (0x51) and small (0x50) tables alternate"
    s, e = gpu_encode(tree, cols, b.heaps, b.n, b.rows, dev)
    assert_bytes(s, e, want, wends)
    check_decode(tree, want, wends, dev, b.rows)


@pytest.mark.parametrize("with_string", [True, False])
def test_row_past_65535_bytes_with_and_without_its_string(dev, kernel, with_string):
    """One record's optional string holds 70,000 bytes: with it the row's data passes 65,535 (a big
    table), without it the same row is small; its neighbours are small either way."""
    b = case("presence_small", 65, "ones", seed=41)
    tree, row = b.tree, 33
    cols, heaps = dict(b.cols), dict(b.heaps)
    big = np.full(70_000, 0x61, np.uint8)
    sp = cols["s"].copy().view(np.uint32).reshape(-1, 2)
    sp[row] = (heaps["s"].size, big.size)
    cols["s"], heaps["s"] = sp.view(np.uint8).reshape(-1, 8), np.concatenate([heaps["s"], big])
    ks = [tree.fields[i].path for i in H.direct_fields(tree, 0)]
    m = H.mask_of(cols, tree, 0).copy()
    m[:, 0] &= ~(np.uint64(1) << np.uint64(ks.index("big")))
    if not with_string:
        m[row, 0] &= ~(np.uint64(1) << np.uint64(ks.index("s")))
    cols["#hasmask"] = m.view(np.uint8).reshape(-1, 8)
    want, wends = H.walk_encode(tree, cols, heaps, b.n)
    assert want[int(wends[row]) - 1] == (0x51 if with_string else 0x50) and want[int(wends[row - 1]) - 1] == 0x50
    s, e = gpu_encode(tree, cols, heaps, b.n, b.rows, dev)
    assert_bytes(s, e, want, wends)
    check_decode(tree, want, wends, dev, b.rows)


@pytest.mark.parametrize("name", ["presence_small", "pkg1", "presence_wide"])
def test_absent_fields_with_garbage_spans_and_canaries(dev, kernel, name):
    """The columns of an absent field are never read: garbage {off, len} spans and values there are
    no error and touch no heap; and the encoder writes only out[0, total) and ends[0, n)."""
    b = case(name, 300, "half")
    tree = b.tree
    rng = np.random.default_rng(5)
    cols = dict(b.cols)
    for t in tree.tables:
        if t.shape != 0 or not any(c.role == ROLE_HASMASK for c in t.columns):
            continue
        m = H.mask_of(cols, tree, t.index)
        for k, i in enumerate(H.direct_fields(tree, t.index)):
            if not tree.fields[i].optional:
                continue
            absent = ((m[:, k // 64] >> np.uint64(k % 64)) & np.uint64(1)) == 0
            for c in t.columns:
                j = c.field
                while j > i:
                    j = tree.fields[j].parent
                if c.role == ROLE_VALUE and j == i:
                    a = cols[c.name].copy()
                    a[absent] = rng.integers(0, 256, (int(absent.sum()), a.shape[1]), dtype=np.uint8)
                    if c.kind in (Kind.STRING, Kind.BYTES):
                        a[absent] = 0xff  # off and len 0xffffffff: far outside any heap
                    cols[c.name] = a
    enc = TreeEncoder(tree, b.rows, dev)
    d_cols, d_heaps = to_dev(cols, dev), to_dev(b.heaps, dev)
    assert int(enc.encode(d_cols, d_heaps, None, None).item()) == b.stream.size
    guard = 256
    out = torch.full((b.stream.size + 2 * guard,), CANARY, dtype=torch.uint8, device=dev)
    ends = torch.full((b.n + 16,), ECANARY, dtype=torch.int64, device=dev)
    assert int(enc.encode(d_cols, d_heaps, out[guard: guard + b.stream.size], ends[8: 8 + b.n]).item()) == b.stream.size
    torch.cuda.synchronize()
    o, e = out.cpu().numpy(), ends.cpu().numpy()
    assert (o[:guard] == CANARY).all() and (o[guard + b.stream.size:] == CANARY).all(), "bytes outside out"
    assert (e[:8] == ECANARY).all() and (e[8 + b.n:] == ECANARY).all(), "entries outside ends"
    assert_bytes(o[guard: guard + b.stream.size], e[8: 8 + b.n].view(np.uint64), b.stream, b.ends)


@pytest.mark.parametrize("name", ["presence_small", "pkg1"])
def test_encode_frames(dev, kernel, name):
    """spec_encode_tree_frames: make_frames of the expected records, ends + 4 (k + 1)."""
    b = case(name, 300, "half")
    frames, fends = gpu_encode(b.tree, b.cols, b.heaps, b.n, b.rows, dev, frames=True)
    assert np.array_equal(fends, b.ends + 4 * np.arange(1, b.n + 1, dtype=np.uint64))
    assert np.array_equal(frames, spec_amd.make_frames(b.stream, b.ends))


def test_record_tiles_past_the_image_with_mixed_masks(dev, kernel):
    """Records of kilobytes: a 64-record tile's output range passes the record-tile writer's LDS
    image (36 KiB), the rest goes straight to HBM; the per-record field mask of the size pass
    includes the optional scalars."""
    b = case("pkg1", 200, "half", seed=77, str_len=(0, 3000))
    starts = np.concatenate([[0], b.ends[:-1]]).astype(np.int64)
    tiles = [int(b.ends[min(b.n, t + 64) - 1]) - int(starts[t]) for t in range(0, b.n, 64)]
    assert max(tiles) > 72 * 1024
    s, e = gpu_encode(b.tree, b.cols, b.heaps, b.n, b.rows, dev)
    assert_bytes(s, e, b.stream, b.ends)
    check_decode(b.tree, b.stream, b.ends, dev, b.rows)


# ---- decode: the kernel paths ----------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["tail_wave0", "tail_wave1", "last_over_slab"])
def test_pkg1_root_pair_over_slab_and_stream_end(dev, where):
    """The construction of tests/test_gpu_tree.py's test of the same name, on the presence tree with mixed masks: a 64-record
    window over the slab (both waves parse it from HBM) among staged windows, and the stream's last
    partial 16-byte chunk in wave 0's or wave 1's share; wave 1's HasField bits reach wave 0 through
    the exchange in every one of them."""
    spec_amd.set_jit(True)
    b = case("pkg1", 1500, "half", seed=77, count=(0, 4))
    tree = b.tree
    e = b.ends.astype(np.int64)
    st = np.concatenate([[0], e[:-1]])
    sz = e - st
    big = int(np.argmax(sz))
    gn = 1 + sum(1 for t in tree.tables if t.index and t.rel == REL_ONE and tree.tables[t.parent].rel != 2)
    extra = 512 * (gn - 1) + 16
    pick = None
    for m in range(600, 1500):
        order = list(range(64)) + [big] * 64 + list(range(128, m))
        if where == "last_over_slab":
            order = list(range(m - 64)) + [big] * 64
        slab, w = root_windows(np.cumsum(sz[order]), extra)
        if not slab:
            continue
        if where == "last_over_slab":
            ok = not w[-1][0] and all(f for f, _ in w[:-1]) and int(np.sum(sz[order])) % 16
        else:
            ok = not w[1][0] and all(f for f, _ in w[:1] + w[2:]) and w[-1][1] == int(where[-1])
        if ok:
            pick = order
            break
    assert pick is not None, "no record count puts the windows where the case needs them"
    stream = np.concatenate([b.stream[st[i]: e[i]] for i in pick])
    ends = np.cumsum(sz[pick]).astype(np.uint64)
    check_decode(tree, stream, ends, dev)


def _record(fields):
    """A record from (tag, kind, value) through the oracle's Writer."""
    w = O.Writer()
    w.message()
    for tag, kind, v in fields:
        w.field(tag, kind, v)
    rec, err = w.end()
    assert err is None
    return rec


def test_rows_the_fast_path_rejects_beside_accepted_ones(dev, kernel):
    """pkg1 records with a foreign tag, an unsorted table and a big table among plain ones in one
    wave: the generated code's fallback writes the same HASMASK words as its fast path."""
    b = case("pkg1", 64, "half", seed=9)
    tree = b.tree
    st = np.concatenate([[0], b.ends[:-1]]).astype(np.int64)
    recs = [bytes(b.stream[st[i]: int(b.ends[i])]) for i in range(b.n)]
    foreign = _record([(1, "bool", True), (11, "int32", 7), (99, "int32", 1), (50, "string", "x")])
    bigtab = _record([(2, "byte", 3), (12, "int64", -5), (300, "int32", 1)])
    unsorted_ = bytearray(_record([(10, "int16", 4), (11, "int32", 5), (12, "int64", 6)]))
    t0 = len(unsorted_) - 3 - 9  # three small entries before rvarint(data), rvarint(table), type
    assert [unsorted_[t0], unsorted_[t0 + 3], unsorted_[t0 + 6]] == [10, 11, 12]
    unsorted_[t0: t0 + 3], unsorted_[t0 + 3: t0 + 6] = unsorted_[t0 + 3: t0 + 6], unsorted_[t0: t0 + 3]
    dup = bytearray(_record([(10, "int16", 4), (11, "int32", 5), (12, "int64", 6)]))
    dup[t0 + 3] = 10  # a duplicate tag
    for at, r in ((3, foreign), (17, bigtab), (30, bytes(unsorted_)), (45, bytes(dup)), (63, foreign)):
        recs[at] = r
    stream = np.frombuffer(b"".join(recs), np.uint8).copy()
    ends = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    rows, got = check_decode(tree, stream, ends, dev)
    root = masks_in(tree, got)[0][:, 0]
    ks = [tree.fields[i].tag for i in H.direct_fields(tree, 0)]
    assert int(root[3]) == sum(1 << ks.index(t) for t in (1, 11, 50))
    assert int(root[17]) == sum(1 << ks.index(t) for t in (2, 12))


def test_run_frames(dev, kernel):
    """spec_tree_decoder_run_frames: the HASMASK words of the framed batch are the unframed ones."""
    b = case("pkg1", 300, "half")
    tree = b.tree
    frames = spec_amd.make_frames(b.stream, b.ends)
    fends = (b.ends + 4 * np.arange(1, b.n + 1, dtype=np.uint64)).view(np.int64)
    d = TreeDecoder(tree)
    fr, fe = torch.from_numpy(frames).to(dev), torch.from_numpy(fends).to(dev)
    assert d.index_frames(fr, fe) == b.rows
    cols = d.alloc(dev)
    got_rows = d.run_frames(fr, fe, cols).cpu().numpy()
    torch.cuda.synchronize()
    assert list(got_rows) == b.rows
    got = [c[: tree.column_rows(tc, b.rows)].cpu().numpy() for c, tc in zip(cols, tree.columns)]
    want, have = H.walk_masks(tree, b.stream, b.ends, b.rows), masks_in(tree, got)
    for x in want:
        assert np.array_equal(have[x], want[x]), x
    p_rows, p_want = oracle_decode(tree.plain(), b.stream, b.ends)
    for c, g, w in zip(tree.plain().columns, H.without_hasmask(tree, got), p_want):
        if not (c.role == ROLE_VALUE and c.kind in (Kind.STRING, Kind.BYTES, Kind.ANY)):  # (spans: frame offsets)
            assert np.array_equal(g, w), c.name


@pytest.mark.parametrize("name", ["presence_small", "pkg1", "presence_wide"])
def test_index_then_decode_without_and_with_only_the_masks(dev, kernel, name):
    """index() writes no column; decode() with the HASMASK columns omitted (NULL) gives the other
    columns unchanged, and with only them requested gives the same words."""
    b = case(name, 300, "half")
    tree = b.tree
    s = torch.from_numpy(b.stream).to(dev)
    e = torch.from_numpy(b.ends.view(np.int64)).to(dev)
    full_rows, full = gpu_decode(tree, b.stream, b.ends, dev)
    d = TreeDecoder(tree)
    assert d.index(s, e) == b.rows == full_rows
    for only_masks in (False, True):
        cols = [c if (tc.role == ROLE_HASMASK) == only_masks else None for c, tc in zip(d.alloc(dev), tree.columns)]
        keep = [c is not None for c in cols]
        for c in cols:
            if c is not None:
                c.fill_(CANARY)
        out = d.decode(cols)
        torch.cuda.synchronize()
        for tc, c, k, w in zip(tree.columns, out.cols, keep, full):
            assert (c is not None) == k
            if c is not None:
                assert np.array_equal(c.cpu().numpy(), w), tc.name


# ---- fuzzed records --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fuzzed(name, seed):
    b = case(name, 2000, "half", seed=200 + seed, count=(0, 5))
    s, e = fuzz(b.stream, b.ends, seed, b.n)
    return b.tree, s, e


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("name", ["presence_small", "pkg1"])
def test_fuzzed_records(dev, name, seed):
    """Mutated and truncated records, decoded by the generated and by the run-time kernels in this
    one test: every other column by reference 1; the root words by oracle.Message(record).has_field,
    zero where the record does not open; a sub-table's words zero where the row's owner has no such
    field or its message does not open; and the two decodes agree on every HASMASK word."""
    tree, s, e = fuzzed(name, seed)
    plain = tree.plain()
    p_rows, p_want = oracle_decode(plain, s, e)
    words = {}
    try:
        for kernel in ("jit", "runtime"):
            spec_amd.set_jit(kernel == "jit")
            rows, got = gpu_decode(tree, s, e, dev)
            assert rows == p_rows, kernel
            assert mismatches(plain, H.without_hasmask(tree, got), p_want) == [], kernel
            have = words[kernel] = masks_in(tree, got)
            want = H.walk_masks(tree, s, e, rows, root_only=True)
            assert np.array_equal(have[0], want[0]), f"root HASMASK ({kernel})"
            status = {t.index: got[next(c.index for c in t.columns if c.name == f"{t.path}#status")].reshape(-1)
                      for t in tree.tables}
            assert not np.any(have[0][(status[0] >= 1) & (status[0] <= 5)]), kernel
            for x, m in have.items():
                if x == 0:
                    continue
                t = tree.tables[x]
                dead = (status[x] >= 1) & (status[x] <= 5)
                if t.rel == REL_ONE:
                    dead |= got[tree.by_name[f"{tree.fields[t.field].path}?"].index].reshape(-1) == 0
                assert not np.any(m[dead]), f"table {x} ({kernel})"
    finally:
        spec_amd.set_jit(True)
    assert set(words["jit"]) == set(words["runtime"]) and len(words["jit"]) >= 2
    for x in words["jit"]:
        assert np.array_equal(words["jit"][x], words["runtime"][x]), f"jit and run-time kernels differ on table {x}"


# ---- the round trip ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["presence_small", "pkg1", "presence_wide"])
def test_round_trip_is_byte_exact_only_with_presence(dev, kernel, name):
    """Records whose writers skipped setters: GPU decode with T' then GPU encode with T' from the
    decoded columns (string and any heaps: the stream) gives the original bytes; the same through
    the plain tree T does not, the absent fields come back as written zeros."""
    b = case(name, 300, "half")
    s = torch.from_numpy(b.stream).to(dev)
    e = torch.from_numpy(b.ends.view(np.int64)).to(dev)
    outs = {}
    for which, tree in (("presence", b.tree), ("plain", b.tree.plain())):
        # (the test trees' plain forms have no precompiled module: they take the run-time kernels)
        spec_amd.set_jit(kernel == "jit" and (which == "presence" or name == "pkg1"))
        dec = spec_amd.decode_tree(tree, s, e)
        assert dec.rows == b.rows
        cols = {c.name: dec.cols[c.index] for c in tree.columns}
        heaps = {c.name: s for c in tree.span_columns()}
        out, ends = spec_amd.encode_tree(tree, cols, heaps, b.n, rows=dec.rows)
        torch.cuda.synchronize()
        outs[which] = (out.cpu().numpy(), ends.cpu().numpy().view(np.uint64))
    assert_bytes(*outs["presence"], b.stream, b.ends)
    assert not np.array_equal(outs["plain"][0], b.stream)
    assert outs["plain"][0].size > b.stream.size

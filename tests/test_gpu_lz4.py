"""GPU LZ4 decompression (spec_lz4_decompress + spec_lz4_pack) against the oracle (oracle/lz4.c):
every block of oracle-written frames decompressed on the device equals the content; corrupt
blocks get the oracle's verdict; short and long literals, near / far / overlapping matches and
sequences too long for the batch window are all exercised; and the whole compressed receive path (LZ4 frame -> blocks -> device
decompress -> device frame index -> in-place decode) equals the oracle decode.

The block kernel is also run on blocks made sequence by sequence (tests/lz4_blocks.py), where the
test and not a compressor chooses the sequences: each family puts them at one of the kernel's
edges (ring, chunk, window, batch, solo), and the expected bytes are built with the block.
spec_lz4_pack runs over more blocks than one scan chunk, and the content checksum at unaligned
data pointers."""
from __future__ import annotations

import numpy as np
import pytest

import spec_amd
from oracle import oracle as O
from spec_amd import FLAT16, workload
from spec_amd.lz4 import decompress, frame_blocks
from tests import lz4_blocks as B
from tests.gpu_helpers import to_dev

pytestmark = pytest.mark.gpu

# The block kernel's constants (spec_amd/csrc/lz4_device.hip:31-32: the compressed ring, its
# chunk and look-ahead, the output window, the longest batched sequence, the sequences of a
# batch) and the 256 positions of its speculative next-token window.  The block families of
# tests/lz4_blocks.py are derived from them and must be revisited when they change.
CR, CHUNK, LOOK, WIN, SOLO, BATCH, SPEC = 16384, 2048, 4096, 8192, 4096, 64, 256
assert dict(CR=CR, CHUNK=CHUNK, LOOK=LOOK, WIN=WIN, SOLO=SOLO, BATCH=BATCH, SPEC=SPEC) == B.K


def gpu_content(dev, f):
    blocks, used, bmax, rc = frame_blocks(f)
    assert rc == 0
    out, sizes, status = decompress(to_dev(f, dev), blocks, bmax)
    return out.cpu().numpy(), status.cpu().numpy()


def _chunks(rng, n, lit, rep):
    """random runs of `lit` bytes, each followed by `rep` bytes copied from earlier output"""
    out = bytearray()
    while len(out) < n:
        out += rng.integers(0, 256, lit, dtype=np.uint8).tobytes()
        src = int(rng.integers(0, max(1, len(out) - rep)))
        out += out[src:src + rep]
    return np.frombuffer(bytes(out[:n]), np.uint8)


@pytest.mark.parametrize("kind", ["text", "random", "mixed", "zeros", "period3", "period200", "records", "chunks",
                                  "longlit"])
def test_frames_round_trip(dev, kind):
    rng = np.random.default_rng(hash(kind) % 1000)
    n = 700000
    data = {
        "text": np.frombuffer((b"spec message field table trailer " * 30000)[:n], np.uint8),
        "random": rng.integers(0, 256, n, dtype=np.uint8),
        "mixed": np.concatenate([rng.integers(0, 6, n // 2, dtype=np.uint8), rng.integers(0, 256, n - n // 2,
                                                                                           dtype=np.uint8)]),
        "zeros": np.zeros(n, np.uint8),          # one match per block far longer than the ring
        "period3": np.frombuffer((b"abc" * n)[:n], np.uint8),
        "period200": np.tile(rng.integers(0, 256, 200, dtype=np.uint8), n // 200 + 1)[:n],
        # many short sequences, near and far matches, batch windows filling up
        "records": np.tile(np.frombuffer(b"".join(bytes([7, i % 13, 0, 0]) + rng.integers(0, 256, 9, dtype=np.uint8)
                                                  .tobytes() for i in range(64)), np.uint8), n // 832 + 1)[:n],
        "chunks": _chunks(rng, n, 300, 700),  # literals > 16 bytes, matches reaching back up to a block
        "longlit": _chunks(rng, n, 9000, 3000),  # literals longer than the ring look-ahead: alone, HBM to HBM
    }[kind]
    for flushes in ([n], [1, 4000, 300001, n]):
        f = O.lz4_frame_write(data, flushes, 256 << 10)
        got, st = gpu_content(dev, f)
        assert not st.any()
        assert np.array_equal(got, data), kind


def test_block_sizes(dev):
    rng = np.random.default_rng(4)
    for bmax in (64 << 10, 1 << 20):
        data = rng.integers(0, 10, 3_000_000, dtype=np.uint8)
        f = O.lz4_frame_write(data, None, bmax)
        got, st = gpu_content(dev, f)
        assert np.array_equal(got, data)


def test_corrupt_blocks(dev):
    """Hand-made blocks: the device status equals the oracle's verdict block by block."""
    import torch

    good = O.lz4_compress_block(b"hello hello hello hello hello!")
    cases = [good, b"\x50hello", b"", bytes([0x10]) + b"a" + bytes([0, 0]), bytes([0x10]) + b"a" + bytes([2, 0]),
             bytes([0x11]) + b"a", bytes([0x50]) + b"abc", bytes([0xF0]), bytes([0x1F]) + b"x" + bytes([1, 0, 10]),
             bytes([0x0F, 1, 0])]
    src = b"".join(cases)
    blocks = np.zeros(len(cases), spec_amd.lz4.BLOCK_DTYPE)
    off = 0
    for i, c in enumerate(cases):
        blocks[i] = (off, len(c), 0)
        off += len(c)
    d = to_dev(np.frombuffer(src + b"\0\0\0\0", np.uint8), dev)[: len(src)]
    L = spec_amd.lib()
    import ctypes as C
    nb, slot = len(cases), 1024
    d_blocks = to_dev(blocks.view(np.uint8), dev)
    slots = torch.zeros(nb * slot, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(nb, dtype=torch.int32, device=dev)
    status = torch.zeros(nb, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.spec_lz4_decompress(p(d), len(src), p(d_blocks), nb, p(slots), slot, p(sizes), p(status), None) == 0
    torch.cuda.synchronize()
    st, sz, sl = status.cpu().numpy(), sizes.cpu().numpy().view(np.uint32), slots.cpu().numpy()
    for i, c in enumerate(cases):
        want = O.lz4_decompress_block(c, slot)
        assert bool(st[i]) == (want is None), (i, c)
        if want is not None:
            assert sz[i] == len(want) and sl[i * slot:i * slot + len(want)].tobytes() == want, i


def test_compressed_receive_path(dev):
    """mpx with compression: Flat16 records -> frames -> one LZ4 frame (flushed per ~500 frames)
    -> host block walk -> device decompress -> device frame index -> in-place decode."""
    import torch

    n = 50_000
    cols, heaps = workload.flat16(n, seed=12)
    stream, ends = O.encode_flat_batch(FLAT16.tags, FLAT16.kinds, cols, [heaps.get(f) for f in range(16)], n)
    frames = spec_amd.make_frames(stream, ends)
    fe = spec_amd.frames_index(frames, n)[0]
    flushes = list(fe[499::500]) + [frames.size]
    comp = O.lz4_frame_write(frames, flushes, 256 << 10, close=False)
    blocks, used, bmax, rc = frame_blocks(comp)
    assert rc == 0 and used == comp.size
    plain, sizes, status = decompress(to_dev(comp, dev), blocks, bmax)
    assert plain.numel() == frames.size
    fends, consumed, st = spec_amd.frames_index_device(plain, n)
    assert st == 0 and consumed == frames.size and fends.numel() == n
    got = spec_amd.decode_frames(FLAT16, plain, fends)
    want_cols, want_status = O.decode_flat_batch(FLAT16.tags, FLAT16.kinds, stream, ends, FLAT16.widths, nthreads=4)
    torch.cuda.synchronize()
    assert np.array_equal(got.status.cpu().numpy(), want_status)
    for f in range(16):
        if FLAT16.kinds[f] in (spec_amd.Kind.STRING, spec_amd.Kind.BYTES):
            continue  # spans point into the framed buffer, not the compact stream
        assert np.array_equal(got.cols[f].cpu().numpy(), want_cols[f]), f


@pytest.mark.parametrize("chunks", [[0], [5], [16], [17, 3, 40], [1000, 1, 15, 16, 4096, 77777], [300_000]])
def test_content_checksum_device(dev, chunks):
    """spec_lz4_content_update / _digest: xxHash32 streamed over any split of the data (empty,
    partial stripes carried between calls, long runs), equal to the oracle's xxh32."""
    import torch

    from spec_amd.lz4 import ContentChecksum

    rng = np.random.default_rng(sum(chunks))
    data = rng.integers(0, 256, sum(chunks), dtype=np.uint8)
    d = torch.from_numpy(data).to(dev) if data.size else torch.zeros(0, dtype=torch.uint8, device=dev)
    cc = ContentChecksum(dev)
    p = 0
    for c in chunks:
        cc.update(d[p: p + c])
        p += c
    assert cc.digest() == O.xxh32(data)


def test_content_checksum_receive_path(dev):
    """A compressed connection's frame end: the blocks decompressed on the device, the content
    checksum computed on the device over the decompressed bytes equals the one the frame stores
    (frame_blocks reports it), and a corrupted stored checksum is detected."""
    import torch

    from spec_amd.lz4 import ContentChecksum, Lz4State

    n = 20_000
    cols, heaps = workload.flat16(n, seed=8)
    stream, ends = O.encode_flat_batch(FLAT16.tags, FLAT16.kinds, cols, [heaps.get(f) for f in range(16)], n)
    fr = spec_amd.make_frames(stream, ends)
    comp = O.lz4_frame_write(fr, None, 256 << 10)
    st = Lz4State()
    blocks, used, bmax, rc = frame_blocks(comp, st)
    assert rc == 0 and (st.flags & 4)
    out, _, _ = decompress(torch.from_numpy(comp).to(dev), blocks, bmax)
    cc = ContentChecksum(dev)
    cc.update(out)
    assert cc.digest() == st.content_checksum == O.xxh32(fr)
    bad = comp.copy()
    bad[-1] ^= 0x40  # the stored checksum's last byte
    st2 = Lz4State()
    frame_blocks(bad, st2)
    assert (st2.flags & 4) and st2.content_checksum != cc.digest()


# ---- the block kernel against constructed sequences (tests/lz4_blocks.py): the expected bytes
# are the synthesizer's, built with the block; every comparison is bit-exact ----
@pytest.mark.parametrize("ending", ["lit", "match"])
def test_blocks_single_sequence_grid(dev, ending):
    """One sequence at every (literal length, match length, offset) of the grid — the per-lane
    and wave-wide literal copies, every length-extension boundary, periodic / exact / disjoint
    matches — ending on 5 literals and ending on the match."""
    B.run_and_check(dev, B.grid(ending))


def test_blocks_solo_boundary(dev):
    B.run_and_check(dev, B.solo())


def test_blocks_batch_and_window_edges(dev):
    B.run_and_check(dev, B.batch_edges())


def test_blocks_far_near_straddle(dev):
    B.run_and_check(dev, B.straddle())


def test_blocks_ring_and_chunk_phases(dev):
    cases = B.random_chains()
    big = sum(len(c.block) > 3 * CR for c in cases)
    assert len(cases) == 200 and big >= 50, big  # the ring wraps several times in at least 50 blocks
    B.run_and_check(dev, cases)
    B.run_and_check(dev, B.ring_sweep())


def test_blocks_length_codes_and_degenerate(dev):
    B.run_and_check(dev, B.boundary_codes())


@pytest.mark.parametrize("S", [6000, 16400])
def test_blocks_capacity(dev, S):
    """A block of exactly slot bytes fits, one of slot + 1 is rejected (as the oracle says),
    whatever the last sequence is; the neighbouring slots, filled to their last byte, come back
    byte-exact: nothing wrote past a slot."""
    cases = B.capacity(S)
    for c in cases:
        assert O.lz4_decompress_block(c.block, S) == c.content, c.label
    assert sum(c.content is None for c in cases) == 4 and all(len(c.content) == S for c in cases if c.content)
    st, sz, sl = B.run_blocks(dev, [c.block for c in cases], S)
    B.check(cases, st, sz, sl, S)


def test_blocks_placement(dev):
    """The grid again with the source ending exactly at the last block's last byte (the
    kernel's bytewise dword tail), blocks packed without padding: src_off on every residue."""
    for ending in ("lit", "match"):
        ls = B.launches(B.grid(ending))
        for slot, group in ls:
            _, table = B.block_table([c.block for c in group])
            assert set(int(o) % 4 for o in table["src_off"]) == {0, 1, 2, 3}, (slot, len(group))
        for slot, group in ls:
            st, sz, sl = B.run_blocks(dev, [c.block for c in group], slot, exact_src=True)
            B.check(group, st, sz, sl, slot)


def test_blocks_malformed_verdict_parity(dev):
    """Truncated and mutated blocks on the fast, careful and alone paths: the device status is
    the oracle's verdict block by block; where the oracle accepts a mutated block, the size and
    the bytes match too."""
    cases = B.malformed()
    assert len(cases) <= 3000
    for slot, group in B.launches(cases):
        want = B.expect(group, slot, O.lz4_decompress_block)
        st, sz, sl = B.run_blocks(dev, [c.block for c in group], slot)
        B.check(want, st, sz, sl, slot)


# ---- spec_lz4_pack ----
def test_pack_many_blocks(dev):
    """2,500 stored blocks (more than two of the scan's 1024-block chunks, a ragged last one) of
    0..9 bytes and a few of 100..300, contiguous in the source so the packed offsets take every
    alignment: the packed bytes, *total and the offsets workspace; out_cap one byte short and a
    corrupt block leave `out` untouched and report the size / all-ones."""
    import ctypes as C

    import torch

    rng = np.random.default_rng(17)
    nb, slot = 2500, 304
    lens = [i % 10 for i in range(nb)]
    for i, n in ((7, 100), (500, 300), (1023, 101), (1024, 299), (1025, 157), (2047, 256), (2048, 123), (2499, 211)):
        lens[i] = n
    blocks = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    want = np.frombuffer(b"".join(blocks), np.uint8)
    scan = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    L = spec_amd.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def pack(sizes, slots, out_cap):
        d_sizes, d_slots = to_dev(sizes.view(np.int32), dev), to_dev(slots, dev)
        out = torch.full((want.size + 64,), 0xC3, dtype=torch.uint8, device=dev)
        wsb = L.spec_lz4_pack_workspace_size(nb)
        assert wsb >= (nb + 1) * 8
        ws = torch.zeros((wsb + 7) // 8, dtype=torch.int64, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        assert L.spec_lz4_pack(p(d_slots), slot, p(d_sizes), nb, p(out), out_cap, p(total), p(ws), wsb, None) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy(), int(total.item()) & (2 ** 64 - 1), ws.cpu().numpy().view(np.uint64)

    st, sz, sl = B.run_blocks(dev, blocks, slot, stored=1)
    assert not st.any() and np.array_equal(sz, np.array(lens, np.uint32))
    out, total, ws = pack(sz, sl, want.size)
    assert total == want.size
    assert np.array_equal(ws[:nb + 1], scan)
    assert np.array_equal(out[:want.size], want) and (out[want.size:] == 0xC3).all()
    # one byte short: the size is still reported, nothing is written
    out, total, _ = pack(sz, sl, want.size - 1)
    assert total == want.size and (out == 0xC3).all()
    # one corrupt block (a match nibble and no offset) among them: status 1, *total all-ones
    stored = np.ones(nb, np.uint32)
    stored[1500] = 0
    blocks[1500] = b"\x11a"
    st, sz, sl = B.run_blocks(dev, blocks, slot, stored=stored)
    assert st[1500] == 1 and sz[1500] == 0xFFFFFFFF and st.sum() == 1
    out, total, _ = pack(sz, sl, want.size)
    assert total == 2 ** 64 - 1 and (out == 0xC3).all()


# ---- the content checksum at unaligned data pointers ----
def _at_offset(dev, piece, k):
    """`piece` copied to byte offset k of an allocation of its own -> the device view"""
    import torch

    buf = torch.zeros(len(piece) + 8, dtype=torch.uint8, device=dev)
    view = buf[k:k + len(piece)]
    if len(piece):
        view.copy_(torch.from_numpy(np.frombuffer(piece, np.uint8).copy()))
    assert buf.data_ptr() % 16 == 0 and (len(piece) == 0 or view.data_ptr() % 4 == k % 4)
    return view


def _fresh(cc):
    cc.state.zero_()
    return cc


CONTENT_NS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97)


def test_content_checksum_unaligned(dev):
    """The funnel-shifted stripe loop (sh = 1, 2, 3) of the content kernel at every stripe count
    around its 32-deep pipeline's entry, steady state and drain, fresh and after carried bytes."""
    from spec_amd.lz4 import ContentChecksum

    rng = np.random.default_rng(23)
    cc = ContentChecksum(dev)
    seen = set()
    for k in (1, 2, 3):
        for ns in CONTENT_NS:
            for carried in (0, 7, 14):
                head = 16 - carried if carried else 0  # bytes that complete the carried stripe
                n = head + 16 * ns + 5
                data = rng.integers(0, 256, carried + n, dtype=np.uint8).tobytes()
                _fresh(cc)
                if carried:
                    cc.update(_at_offset(dev, data[:carried], 0))
                cc.update(_at_offset(dev, data[carried:], k))
                seen.add(((k + head) & 3, (n - head) // 16))  # the kernel's sh and ns
                assert cc.digest() == O.xxh32(data), (k, ns, carried)
    assert seen >= {(sh, ns) for sh in (1, 2, 3) for ns in CONTENT_NS}, sorted(seen)
    # one long update at offset 3
    data = rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    _fresh(cc).update(_at_offset(dev, data, 3))
    assert cc.digest() == O.xxh32(data)


def test_content_checksum_two_piece_splits(dev):
    """Every split (a, b), a and b in 0..33, the second piece at a misaligned pointer."""
    from spec_amd.lz4 import ContentChecksum

    rng = np.random.default_rng(29)
    data = rng.integers(0, 256, 66, dtype=np.uint8).tobytes()
    firsts = {a: _at_offset(dev, data[:a], 0) for a in range(34)}
    cc = ContentChecksum(dev)
    for a in range(34):
        for b in range(34):
            k = 1 + (a + b) % 3
            second = _at_offset(dev, data[a:a + b], k)
            _fresh(cc).update(firsts[a])
            cc.update(second)
            assert cc.digest() == O.xxh32(data[:a + b]), (a, b, k)


def test_content_checksum_two_frames(dev):
    """Two checksummed frames (a skippable frame between them) in one buffer: each call of
    frame_blocks ends with a frame; its blocks decompressed on the device and hashed by a fresh
    ContentChecksum give that call's state.content_checksum."""
    from spec_amd.lz4 import ContentChecksum, Lz4State

    rng = np.random.default_rng(31)
    data = rng.integers(0, 6, 500_000, dtype=np.uint8)
    cut = 300_007
    f1 = O.lz4_frame_write(data[:cut], [77, cut], 64 << 10)
    f2 = O.lz4_frame_write(data[cut:], None, 256 << 10)
    skip = np.frombuffer(b"\x5f\x2a\x4d\x18" + (3).to_bytes(4, "little") + b"xyz", np.uint8)
    buf = np.concatenate([f1, skip, f2])
    st, pos, parts = Lz4State(), 0, []
    while pos < buf.size:
        assert len(parts) < 2
        piece = buf[pos:]
        blocks, used, bmax, rc = frame_blocks(piece, st)
        assert rc == 0 and used > 0 and (st.flags & 4)
        out, _, status = decompress(to_dev(piece, dev), blocks, bmax)
        assert not status.cpu().numpy().any()
        cc = ContentChecksum(dev)
        cc.update(out)
        assert cc.digest() == st.content_checksum == O.xxh32(out.cpu().numpy())
        parts.append(out.cpu().numpy())
        pos += used
    assert pos == buf.size and len(parts) == 2
    assert np.array_equal(parts[0], data[:cut]) and np.array_equal(parts[1], data[cut:])

"""The LZ4 oracle (oracle/lz4.c: mpx's compression, pierrec/lz4/v4 restated from the published
formats).  pierrec is absent, so the exact compressed bytes are parity-unpinned; what is pinned
here: xxHash32 against the xxhash module and a table of its digests, hand-made blocks
(literal-only, overlapping matches, the error classes of pierrec's decodeBlock), the block decoder
against constructed sequences (tests/lz4_blocks.py, the families the device kernel is tested
with), and round trips of the compressor/decompressor and of the frame writer/reader (header
checksum, block/content checksums, stored blocks, flushes)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import lz4_blocks as B


def test_xxh32_known_answers():
    # XXH32 reference values (xxHash specification test vectors)
    assert O.xxh32(b"") == 0x02CC5D05
    assert O.xxh32(b"", 1) == 0x0B2CB792


def test_hand_made_blocks():
    # literal-only block: token 0x50, "hello"
    assert O.lz4_decompress_block(b"\x50hello", 100) == b"hello"
    # "ab" then a match of 6 at offset 2 (overlapping copy repeats the pattern), then 1 literal
    blk = bytes([0x22]) + b"ab" + bytes([2, 0]) + bytes([0x10]) + b"z"
    assert O.lz4_decompress_block(blk, 100) == b"ab" + b"abababab"[:6] + b"z"
    # run-length: 1 literal, offset 1, match 4 + 15 + 10 = 29
    blk = bytes([0x1F]) + b"x" + bytes([1, 0, 10])
    assert O.lz4_decompress_block(blk, 100) == b"x" * 30
    # long literal run: 15 + 255 + 5 = 275 bytes
    lit = bytes(range(256)) + bytes(19)
    blk = bytes([0xF0, 255, 5]) + lit
    assert O.lz4_decompress_block(blk, 1000) == lit
    # error classes: empty, offset 0, offset beyond the output start, a match nibble with no
    # offset, literal overrun, output overrun
    assert O.lz4_decompress_block(b"", 10) is None
    assert O.lz4_decompress_block(bytes([0x10]) + b"a" + bytes([0, 0]), 10) is None
    assert O.lz4_decompress_block(bytes([0x10]) + b"a" + bytes([2, 0]), 10) is None
    assert O.lz4_decompress_block(bytes([0x11]) + b"a", 10) is None
    assert O.lz4_decompress_block(bytes([0x50]) + b"abc", 10) is None
    assert O.lz4_decompress_block(b"\x50hello", 4) is None


def test_block_round_trips():
    rng = np.random.default_rng(3)
    for data in [b"", b"a", b"abcd" * 1000, rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
                 (b"spec message " * 50 + rng.integers(0, 4, 300, dtype=np.uint8).tobytes()) * 40]:
        c = O.lz4_compress_block(data)
        assert O.lz4_decompress_block(c, len(data)) == data
    # compressible data shrinks
    assert len(O.lz4_compress_block(b"abcd" * 1000)) < 200


def test_frame_round_trips():
    rng = np.random.default_rng(5)
    data = np.concatenate([rng.integers(0, 8, 300000, dtype=np.uint8),
                           rng.integers(0, 256, 100000, dtype=np.uint8)])
    for bcs in (False, True):
        for flushes in ([data.size], [1000, 70000, 262144 + 5, data.size]):
            f = O.lz4_frame_write(data, flushes, 256 << 10, content_checksum=True, block_checksum=bcs)
            assert f[:4].tobytes() == b"\x04\x22\x4d\x18"
            rc, out, used = O.lz4_frame_read(f, data.size + 10)
            assert rc == 0 and used == f.size and np.array_equal(out, data)
    # header checksum, content checksum, corrupt block
    f = O.lz4_frame_write(data, None, 64 << 10)
    g = f.copy()
    g[6] ^= 1
    assert O.lz4_frame_read(g, data.size)[0] == -2
    g = f.copy()
    g[-1] ^= 1
    assert O.lz4_frame_read(g, data.size)[0] == -6
    # an unclosed frame (a live connection): every complete block, the partial one left
    f = O.lz4_frame_write(data, [200000, data.size], 64 << 10, close=False)
    rc, out, used = O.lz4_frame_read(f[:-100], data.size)
    assert rc == 0 and used < f.size - 100 and np.array_equal(out, data[:out.size]) and out.size % 1 == 0


# ---- xxHash32 pinned: against the xxhash module where it is installed, and by a table of its
# digests (generated from the module, xxhash 3.8.1) where it is not ----
def _xxh_input(n):
    return bytes((131 * i + 7) & 255 for i in range(n))


# (length, seed, xxhash.xxh32(_xxh_input(length), seed).intdigest())
XXH32_TABLE = [
    (0, 0x00000000, 0x02CC5D05), (1, 0x00000000, 0x002E0D32), (15, 0x00000000, 0x57055FE6),
    (16, 0x00000000, 0x64287C90), (17, 0x00000000, 0x1C63FDC5), (17, 0x00000001, 0x30AB243B),
    (17, 0xFFFFFFFF, 0xDE37D5BE), (31, 0x9E3779B1, 0x6782F4D6), (32, 0x00000000, 0x1E1BFF83),
    (33, 0x9E3779B1, 0x66B35A99), (4095, 0x00000000, 0xFB01CCEA), (4096, 0x00000000, 0xE4D29CA7),
    (4096, 0x00000001, 0x2E6DCC1D), (4096, 0xFFFFFFFF, 0x60C5846D), (4097, 0x9E3779B1, 0x4C16FDD3),
    (100000, 0x00000000, 0x54C4C799),
]


def test_xxh32_table():
    for n, seed, want in XXH32_TABLE:
        assert O.xxh32(_xxh_input(n), seed) == want, (n, hex(seed))


def test_xxh32_against_module():
    xxhash = pytest.importorskip("xxhash")
    lengths = sorted(set(range(301)) | {16 * k + d for k in (32, 64, 256) for d in range(-2, 3)} | {100_000})
    rng = np.random.default_rng(9)
    data = rng.integers(0, 256, max(lengths), dtype=np.uint8).tobytes()
    for seed in (0, 1, 0x9E3779B1, 0xFFFFFFFF):
        for n in lengths:
            assert O.xxh32(data[:n], seed) == xxhash.xxh32(data[:n], seed=seed).intdigest(), (n, hex(seed))
    for n, seed, want in XXH32_TABLE:  # the table is the module's
        assert xxhash.xxh32(_xxh_input(n), seed=seed).intdigest() == want, (n, hex(seed))


# ---- the block decoders against constructed sequences (tests/lz4_blocks.py): every family the
# device kernel is tested with goes through oracle/lz4.c and the Python restatement of the format;
# both must give the content the synthesizer built ----
def _agree(cases):
    for c in cases:
        slot = B.slot_for(c.need)
        for cap in (slot, len(c.content)) if c.content is not None else (slot,):
            got_o, got_p = O.lz4_decompress_block(c.block, cap), B.decode(c.block, cap)
            assert got_o == c.content, f"oracle, cap {cap}: {c.label}"
            assert got_p == c.content, f"lz4_blocks.decode, cap {cap}: {c.label}"
        if c.content:  # one byte short of the content: both reject
            cap = len(c.content) - 1
            assert O.lz4_decompress_block(c.block, cap) is None, f"oracle accepts cap {cap}: {c.label}"
            assert B.decode(c.block, cap) is None, f"lz4_blocks.decode accepts cap {cap}: {c.label}"


@pytest.mark.parametrize("family", ["grid-lit", "grid-match", "solo", "batch_edges", "straddle", "random_chains",
                                    "ring_sweep", "boundary_codes", "capacity"])
def test_synth_families_agree(family):
    cases = {"grid-lit": lambda: B.grid("lit"), "grid-match": lambda: B.grid("match"), "solo": B.solo,
             "batch_edges": B.batch_edges, "straddle": B.straddle, "random_chains": B.random_chains,
             "ring_sweep": B.ring_sweep, "boundary_codes": B.boundary_codes,
             "capacity": lambda: B.capacity(6000) + B.capacity(16400)}[family]()
    if family == "capacity":  # the S + 1 blocks are valid blocks that do not fit their slot
        for c in cases:
            want = c.content
            assert O.lz4_decompress_block(c.block, c.need) == want and B.decode(c.block, c.need) == want, c.label
            if want is None:
                assert len(B.decode(c.block, c.need + 1)) == c.need + 1 == len(O.lz4_decompress_block(c.block,
                                                                                                       c.need + 1))
        return
    _agree(cases)


def test_synth_family_sizes():
    """The conditions the families must meet on their inputs (asserted again before the GPU runs)."""
    assert len(B.grid("lit")) == len(B.grid("match")) == 19 * 17 * 21
    big = sum(len(c.block) > 3 * B.CR for c in B.random_chains())
    assert len(B.random_chains()) == 200 and big >= 50, big
    assert sum(c.label.endswith("end=match") for c in B.random_chains()) >= 66
    assert len(B.malformed()) <= 3000
    for fam in (B.grid("lit"), B.grid("match"), B.solo(), B.batch_edges(), B.straddle(), B.random_chains(),
                B.ring_sweep(), B.boundary_codes(), B.malformed()):
        for slot, group in B.launches(fam):
            assert len(group) <= 10_000 and len(group) * slot <= 64 << 20


def test_length_code_is_unique():
    """noncanonical=True spells out the 0xFF..FF 00 form at lengths of 15 + 255 k; the format
    reads extension bytes until one is not 255, so those are the bytes of the plain encoding too."""
    for ll in (15, 270, 525, 100):
        for ml in (19, 274, 529, 100):
            a = B.synth([(300, 1, 4), (ll, 300, ml)], ll, np.random.default_rng(1), noncanonical=True)
            b = B.synth([(300, 1, 4), (ll, 300, ml)], ll, np.random.default_rng(1))
            assert a == b
    blk, out = B.synth([(270, 270, 274)], 15, np.random.default_rng(1), noncanonical=True)
    assert blk[:3] == b"\xff\xff\x00" and blk[273:278] == bytes([0x0E, 0x01, 0xFF, 0x00, 0xF0]) and blk[278] == 0
    assert len(out) == 270 + 274 + 15


def test_malformed_verdicts_agree():
    """Every malformed block: the oracle and the Python decoder give the same verdict and bytes."""
    cases = B.malformed()
    rejected = 0
    for c in cases:
        slot = B.slot_for(c.need)
        a, b = O.lz4_decompress_block(c.block, slot), B.decode(c.block, slot)
        assert a == b, c.label
        rejected += a is None
    assert rejected > len(cases) // 2 and rejected < len(cases)  # both verdicts occur


def test_check_helper_can_fail():
    """The comparison the device tests make, fed a wrong 'device' result: one byte flipped in one
    slot, one status flipped, one size off by one — each fails and names the block's family."""
    cases = B.straddle()[:40] + [B.Case("made-up rejected block ll=1 off=2 ml=4", b"\x10a\x02\x00", None, 16)]
    slot = B.slot_for(max(c.need for c in cases))
    status = np.array([c.content is None for c in cases], np.uint8)
    sizes = np.array([0xFFFFFFFF if c.content is None else len(c.content) for c in cases], np.uint32)
    slots = np.full(len(cases) * slot, 0xA5, np.uint8)
    for i, c in enumerate(cases):
        if c.content is not None:
            slots[i * slot:i * slot + len(c.content)] = np.frombuffer(c.content, np.uint8)
    B.check(cases, status, sizes, slots, slot)  # the right answer passes
    bad = slots.copy()
    bad[17 * slot + len(cases[17].content) - 1] ^= 1
    with pytest.raises(AssertionError, match=r"block 17 .*straddle first-batch=\w+ first_op=\d+ ll=\d+ off=\d+ "
                                             r"ml=\d+ .*end=.*byte \d+"):
        B.check(cases, status, sizes, bad, slot)
    for i in (5, len(cases) - 1):  # an accepted block rejected, a rejected block accepted
        bad = status.copy()
        bad[i] ^= 1
        with pytest.raises(AssertionError, match=rf"block {i} .*ll=\d+ off=\d+ ml=\d+"):
            B.check(cases, bad, sizes, slots, slot)
    bad = sizes.copy()
    bad[9] += 1
    with pytest.raises(AssertionError, match=r"block 9 .*ll=\d+ off=\d+ ml=\d+.*size"):
        B.check(cases, status, bad, slots, slot)
    bad = sizes.copy()
    bad[-1] = 5  # a rejected block must also report the all-ones size
    with pytest.raises(AssertionError, match="made-up rejected block"):
        B.check(cases, status, bad, slots, slot)

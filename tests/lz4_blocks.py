"""LZ4 blocks made sequence by sequence, for tests of the block decoders (oracle/lz4.c and the
device kernel, spec_amd/csrc/lz4_device.hip).

`synth` writes a block from a list of (literal length, offset, match length) and builds the
content it must decompress to as it goes, so the expected output exists by construction and not
from any decoder.  `decode` is a plain restatement of the block format with the error classes of
pierrec's decodeBlock: a third opinion next to the oracle's C decoder.  `run_blocks` hands blocks
to spec_lz4_decompress through the C ABI; `check` compares what came back with the expectation
and names the failing block's family parameters.  The family builders below put sequences at the
device kernel's edges (its constants are mirrored in K); the CPU tests run them through both host
decoders, the GPU tests through the kernel.

Nothing here needs a GPU or the oracle; only `run_blocks` and `block_table` import spec_amd
(torch + libspec_amd.so), inside themselves."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

# The device kernel's constants (spec_amd/csrc/lz4_device.hip:31-32, and the 256-position
# speculative window of its fast chain).  The families below are derived from them: revisit the
# families when they change.
K = dict(CR=16384, CHUNK=2048, LOOK=4096, WIN=8192, SOLO=4096, BATCH=64, SPEC=256)
CR, CHUNK, LOOK, WIN, SOLO, BATCH, SPEC = (K[k] for k in ("CR", "CHUNK", "LOOK", "WIN", "SOLO", "BATCH", "SPEC"))

MIN_MATCH = 4


class Case(NamedTuple):
    label: str              # the family parameters, for a failure message
    block: bytes
    content: bytes | None   # what the block decompresses to; None: the decoder must reject it
    need: int               # output capacity the case wants (the launch's slot is >= need)


# ---------------------------------------------------------------------------------------------
# synthesizer
# ---------------------------------------------------------------------------------------------
def _length_code(out: bytearray, length: int, noncanonical: bool):
    """the extension bytes of a length whose nibble is 15 (length >= 15)"""
    rest = length - 15
    if noncanonical and rest % 255 == 0:
        # the explicit 0xFF..FF 00 form: a zero byte closes the run of 255s.  The format reads
        # extension bytes until one is not 255, so this is also what the loop below emits: the
        # length code has exactly one representation, and the option only states it outright.
        out += b"\xff" * (rest // 255) + b"\x00"
        return
    while rest >= 255:
        out.append(255)
        rest -= 255
    out.append(rest)


def synth_marks(seqs, tail, rng, *, noncanonical=False):
    """synth, plus for every sequence (token position, offset position, output size before its
    match) — what the malformed family mutates."""
    blk, out, marks = bytearray(), bytearray(), []
    for ll, off, ml in seqs:
        assert ll >= 0 and ml >= MIN_MATCH and 1 <= off <= 65535, (ll, off, ml)
        tpos = len(blk)
        blk.append((min(ll, 15) << 4) | min(ml - MIN_MATCH, 15))
        if ll >= 15:
            _length_code(blk, ll, noncanonical)
        lit = rng.integers(0, 256, ll, dtype=np.uint8).tobytes()
        blk += lit
        out += lit
        assert off <= len(out), f"offset {off} reaches before the output ({len(out)} bytes)"
        marks.append((tpos, len(blk), len(out)))
        blk += off.to_bytes(2, "little")
        if ml - MIN_MATCH >= 15:
            _length_code(blk, ml - MIN_MATCH, noncanonical)
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:  # an overlapping copy repeats the last `off` bytes
            pat = bytes(out[start:])
            out += (pat * (ml // off + 1))[:ml]
    if tail is not None:
        marks.append((len(blk), None, len(out)))
        blk.append(min(tail, 15) << 4)
        if tail >= 15:
            _length_code(blk, tail, noncanonical)
        lit = rng.integers(0, 256, tail, dtype=np.uint8).tobytes()
        blk += lit
        out += lit
    return bytes(blk), bytes(out), marks


def synth(seqs, tail, rng, *, noncanonical=False):
    """seqs: [(literal_len, offset, match_len)]; tail: the final literal count, or None for a
    block that ends on a match -> (block_bytes, content_bytes)."""
    blk, out, _ = synth_marks(seqs, tail, rng, noncanonical=noncanonical)
    return blk, out


# ---------------------------------------------------------------------------------------------
# independent decoder
# ---------------------------------------------------------------------------------------------
def decode(block: bytes, cap: int):
    """The LZ4 block format, decoded into at most cap bytes -> bytes, or None for a block that
    pierrec's decodeBlock rejects (empty input, a length extension or an offset cut off by the
    block's end, literals past the block's end, offset 0 or reaching before the output, output
    past cap)."""
    n = len(block)
    if n == 0:
        return None
    out = bytearray()
    si = 0
    while si < n:
        token = block[si]
        si += 1
        ll = token >> 4
        if ll == 15:
            while True:
                if si >= n:
                    return None
                v = block[si]
                si += 1
                ll += v
                if v != 255:
                    break
        if ll:
            if si + ll > n or len(out) + ll > cap:
                return None
            out += block[si:si + ll]
            si += ll
        ml = token & 15
        if si == n and ml == 0:
            break  # the last sequence: literals only
        if si + 2 > n:
            return None
        off = block[si] | (block[si + 1] << 8)
        si += 2
        if off == 0:
            return None
        ml += MIN_MATCH
        if ml == 19:
            while True:
                if si >= n:
                    return None
                v = block[si]
                si += 1
                ml += v
                if v != 255:
                    break
        if off > len(out) or len(out) + ml > cap:
            return None
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:
            pat = bytes(out[start:])
            out += (pat * (ml // off + 1))[:ml]
    return bytes(out)


# ---------------------------------------------------------------------------------------------
# the device, through the C ABI
# ---------------------------------------------------------------------------------------------
SLOT_CLASSES = (256, 1024, 4096, 16384, 32768, 81920, 262144)


def slot_for(need: int) -> int:
    """the smallest slot class (each a multiple of 16) that holds `need` bytes"""
    for s in SLOT_CLASSES:
        if need <= s:
            return s
    raise ValueError(f"no slot class for {need} bytes")


def block_table(blocks):
    """blocks packed back to back, no padding between them -> (source bytes, block table);
    src_off takes whatever residue mod 4 the sizes give."""
    from spec_amd.lz4 import BLOCK_DTYPE

    table = np.zeros(len(blocks), BLOCK_DTYPE)
    off = 0
    for i, b in enumerate(blocks):
        table[i] = (off, len(b), 0)
        off += len(b)
    return b"".join(blocks), table


def run_blocks(dev, blocks, slot, *, exact_src=False, stored=None):
    """spec_lz4_decompress over `blocks` (packed by block_table into one device buffer), every
    block into its own slot of `slot` bytes -> (status, sizes, slots) as numpy.  exact_src: the
    source ends with the last block's last byte (the kernel's bytewise dword tail); otherwise 8
    bytes of padding follow.  stored: optional per-block flags (1: stored uncompressed)."""
    import ctypes as C

    import torch

    import spec_amd

    assert slot % 16 == 0 and len(blocks) > 0
    src, table = block_table(blocks)
    if stored is not None:
        table["stored"] = stored
    if not exact_src:
        src += bytes(8)
    src_len = len(src)
    d_src = torch.from_numpy(np.frombuffer(src + bytes(16), np.uint8).copy()).to(dev)[:src_len]
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    nb = len(blocks)
    slots = torch.full((nb * slot,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(nb, dtype=torch.int32, device=dev)
    status = torch.full((nb,), 7, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = spec_amd.lib().spec_lz4_decompress(p(d_src), src_len, p(d_table), nb, p(slots), slot, p(sizes), p(status),
                                            None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return status.cpu().numpy(), sizes.cpu().numpy().view(np.uint32), slots.cpu().numpy()


def launches(cases, *, max_blocks=10_000, max_bytes=64 << 20):
    """cases grouped into launches: by slot class (slot_for(need)), each launch at most
    max_blocks blocks and max_bytes of slots -> [(slot, [case])], order kept within a class."""
    by_slot = {}
    for c in cases:
        by_slot.setdefault(slot_for(c.need), []).append(c)
    out = []
    for slot in sorted(by_slot):
        per = max(1, min(max_blocks, max_bytes // slot))
        group = by_slot[slot]
        out += [(slot, group[i:i + per]) for i in range(0, len(group), per)]
    return out


def check(cases, status, sizes, slots, slot):
    """The comparison every device test makes: block i of the launch against cases[i] — status 0,
    the content's size and the content's bytes in its slot, or status 1 and an all-ones size for
    a block that must be rejected.  A mismatch raises with the case's label."""
    assert len(status) == len(sizes) == len(cases) and len(slots) == len(cases) * slot
    for i, c in enumerate(cases):
        where = f"block {i} of the launch (slot {slot}, {len(c.block)} compressed bytes) [{c.label}]"
        if c.content is None:
            if status[i] != 1 or sizes[i] != 0xFFFFFFFF:
                raise AssertionError(f"{where}: must be rejected, got status {status[i]} size {sizes[i]}")
            continue
        if status[i] != 0:
            raise AssertionError(f"{where}: status {status[i]}, want 0 ({len(c.content)} bytes)")
        if sizes[i] != len(c.content):
            raise AssertionError(f"{where}: size {sizes[i]}, want {len(c.content)}")
        got = slots[i * slot:i * slot + len(c.content)]
        want = np.frombuffer(c.content, np.uint8)
        if not np.array_equal(got, want):
            j = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"{where}: byte {j} of {len(c.content)} is {got[j]:#04x}, want {want[j]:#04x} "
                                 f"({int((got != want).sum())} bytes differ)")


def run_and_check(dev, cases, *, exact_src=False):
    """every case through the device, launch by launch -> [(slot, [case])] as launched"""
    ls = launches(cases)
    for slot, group in ls:
        st, sz, sl = run_blocks(dev, [c.block for c in group], slot, exact_src=exact_src)
        check(group, st, sz, sl, slot)
    return ls


# ---------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------
def _case(label, seqs, tail, rng, *, noncanonical=False, need=None):
    blk, out = synth(seqs, tail, rng, noncanonical=noncanonical)
    end = "match" if tail is None else f"lit{tail}"
    return Case(f"{label} end={end}", blk, out, len(out) if need is None else need)


def _filler(need, kind):
    """sequences that put at least `need` bytes of output before the sequence under test ->
    (seqs, name).  kind 0: one literal run (alone when it is long); kind 1: a chain of batched
    sequences with near and far matches."""
    if need <= 0:
        return [], "none"
    if kind == 0:
        return [(max(1, need - 4), 1, 4)], f"lit:{max(1, need - 4)}"
    seqs, have = [], 0
    while have < need:
        seqs.append((100, 50 if have < 2000 else 1900, 900))
        have += 1000
    return seqs, f"chain:{len(seqs)}"


GRID_LL = (0, 1, 5, 6, 14, 15, 16, 17, 63, 64, 65, 269, 270, 271, 524, 525, 4095, 4096, 4097)
GRID_ML = (4, 5, 18, 19, 20, 63, 64, 65, 273, 274, 275, 4092, 4096, 4097, 8191, 8192, 8193)
GRID_OFF = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 255, 256, 4095, 4096, 8191, 8192, 8193, 65535)


@functools.lru_cache(maxsize=None)
def grid(ending):
    """One sequence at every (ll, ml, off) of the grid, after a filler where the offset reaches
    before the sequence's own literals.  ending: 'lit' (5 trailing literals) or 'match'."""
    rng = np.random.default_rng(11 if ending == "lit" else 12)
    tail = 5 if ending == "lit" else None
    cases = []
    for ll in GRID_LL:
        for ml in GRID_ML:
            for off in GRID_OFF:
                pre, name = _filler(off - ll, (ll + ml + off) & 1)
                cases.append(_case(f"grid ll={ll} off={off} ml={ml} prefix={name}", pre + [(ll, off, ml)], tail, rng))
    return cases


@functools.lru_cache(maxsize=None)
def solo():
    """Sequences at the SOLO boundary (ll + ml of 4095 / 4096 / 4097: batched or alone), alone
    sequences reading their own literals or repeating, a batched match that reads what an alone
    sequence stored, an alone last literal run, literals that end past the ring's look-ahead
    behind other sequences, and a literal run longer than the ring."""
    rng = np.random.default_rng(21)
    cases = []
    seed = (16, 8, 8)
    for tail in (5, None):
        for total in (SOLO - 1, SOLO, SOLO + 1):
            for ll, ml in ((total - 4, 4), (total - 5, 5), (0, total), (1, total - 1), (total // 2, total - total // 2)):
                for off in (1, 13, 24):
                    cases.append(_case(f"solo-boundary ll={ll} off={off} ml={ml} prefix=seed(16,8,8)",
                                       [seed, (ll, off, ml)], tail, rng))
        # off <= ll: the match source lies in the sequence's own literals; off < ml: periodic
        for ll, off, ml in ((3000, 2000, 2000), (3000, 3000, 1500), (5000, 1, 4), (100, 7, 5000), (4200, 64, 65),
                            (2, 2, 9000), (0, 24, 4200), (6000, 5999, 6000)):
            cases.append(_case(f"solo-self ll={ll} off={off} ml={ml} prefix=seed(16,8,8)", [seed, (ll, off, ml)],
                               tail, rng))
        # a batched far match reads bytes the parser wave stored
        for ll, off, ml in ((2, 3000, 20), (0, 5004, 100), (5, 17, 40), (0, 1, 70), (3, 4999, 4000)):
            cases.append(_case(f"after-solo ll={ll} off={off} ml={ml} prefix=solo(5000,1,4)",
                               [(5000, 1, 4), (ll, off, ml)], tail, rng))
            cases.append(_case(f"after-solo ll={ll} off={off} ml={ml} prefix=seed+solo(0,8,5000)",
                               [seed, (0, 8, 5000), (ll, off, ml)], tail, rng))
        # literals of 4050..4096 and a 4-byte match, batched behind other sequences
        for ll in range(4050, 4097):
            for k in (1, 5):
                cases.append(_case(f"look-ahead ll={ll} off=2 ml=4 prefix={k}x(3,1,5) then (2,9,6)",
                                   [(3, 1, 5)] * k + [(ll, 2, 4), (2, 9, 6)], tail, rng))
        # longer than the ring
        cases.append(_case("long-literal ll=20000 off=5 ml=40 prefix=(4,1,4) then (3,100,10)",
                           [(4, 1, 4), (20000, 5, 40), (3, 100, 10)], tail, rng))
        cases.append(_case("long-literal ll=40000 off=39999 ml=300 prefix=none", [(40000, 39999, 300)], tail, rng))
    # an alone sequence as the last, literal-only one
    for t in (SOLO - 4, SOLO - 3, SOLO + 1, 5000, 20000):
        cases.append(_case(f"solo-last prefix=(4,1,8) tail={t}", [(4, 1, 8)], t, rng))
        cases.append(_case(f"solo-last prefix=none tail={t}", [], t, rng))
        cases.append(_case(f"solo-last prefix=70x(0,3,4) tail={t}", [(4, 1, 8)] + [(0, 3, 4)] * 70, t, rng))
    return cases


def _shift(p, kind):
    """a prefix after which the next batch starts at a chosen phase -> (seqs, output bytes).
    'solo': one literal run that runs alone; 'count': 64 sequences, a full batch by count."""
    if kind == "solo":
        return [(SOLO + 1 + p, 1, 4)], SOLO + 5 + p
    return [(p + 1, 1, 4)] + [(0, 3, 4)] * (BATCH - 1), p + 1 + 4 * BATCH


@functools.lru_cache(maxsize=None)
def batch_edges():
    """Chains of minimal sequences around the batch's 64-sequence limit, and chains of equal
    sequences whose output ends within 17 bytes below to 1 byte above WIN measured from the
    batch's first byte — so that, whatever the phase of the batch start (wb = op & ~15), the
    chain ends at, one before and one after the window's end.  The batch start is shifted by a
    literal prefix of 0..17 bytes."""
    rng = np.random.default_rng(31)
    cases = []
    i = 0
    for count in (63, 64, 65, 127, 128, 129):
        for p in range(18):
            for off in (1, 3, 4):
                i += 1
                cases.append(_case(f"min-chain count={count} seed-literals={p + 1} ll=0 off={off} ml=4",
                                   [(p + 1, 1, 4)] + [(0, off, 4)] * count, 5 if i & 1 else None, rng))
    shapes = {"32x(16,100,240)": [(16, 100, 240)] * 31,          # the fast chain
              "60x(8,24,128)": [(8, 24, 128)] * 60,              # periodic matches
              "13x(40,250,560)": [(40, 250, 560)] * 13}          # lengths of the careful path
    for kind in ("solo", "count"):
        for p in range(18):
            pre, base = _shift(p, kind)
            for name, body in shapes.items():
                got = sum(ll + ml for ll, _, ml in body)
                for total in range(WIN - 17, WIN + 2):
                    i += 1
                    last = (total - got - 4, 9, 4)  # the sequence that reaches `total`
                    assert last[0] >= 0
                    cases.append(_case(f"window-chain shape={name} total={total} batch-start={base} ({kind} prefix "
                                       f"{p}) last=(ll={last[0]},off=9,ml=4) then (3,50,9)",
                                       pre + body + [last, (3, 50, 9)], 5 if i & 1 else None, rng))
    return cases


@functools.lru_cache(maxsize=None)
def straddle():
    """Two batches: the first fills the window (to within 4 bytes of its end, or 64 sequences), the
    second holds one match whose source is swept across the second batch's first byte: ending 2,
    1, 0 bytes before it (far), crossing it by 1 and 2 bytes (straddling), starting at it
    (near); non-overlapping (off > ml) and periodic (off < ml); ml below and above 64 and not a
    multiple of 16."""
    rng = np.random.default_rng(41)
    cases = []
    i = 0
    for fill, p in [("window", r) for r in range(5)] + [("count", p) for p in range(16)]:
        if fill == "window":  # WIN - p bytes, p < 5: no further sequence of the sweep fits
            first = [(16, 1, WIN - p - 31 * 256 - 16)] + [(16, 100, 240)] * 31
        else:                 # 64 sequences: first_op takes every phase
            first = [(p + 8, 1, 100)] + [(8, 16, 119)] * (BATCH - 1)
        f_op = sum(ll + ml for ll, _, ml in first)
        for ml in (5, 37, 64, 150):
            sweep = []
            for d in (-2, -1, 0, 1, 2):  # source end - first_op, off > ml
                ll2 = 10
                sweep.append((ll2, ll2 + ml - d, ml, f"src-end={d:+d}"))
            sweep.append((ml + 5, ml + 5, ml, "src-start=+0"))
            for off in sorted({3, ml - 1}):  # periodic: the source ends at the match
                for ll2 in (0, 1, 2):
                    sweep.append((ll2, off, ml, f"src-end={ll2:+d} periodic"))
                sweep.append((off, off, ml, "src-start=+0 periodic"))
            for ll2, off, mlen, what in sweep:
                i += 1
                cases.append(_case(f"straddle first-batch={fill} first_op={f_op} ll={ll2} off={off} ml={mlen} "
                                   f"{what}", first + [(ll2, off, mlen)], 5 if i & 1 else None, rng))
    return cases


_EDGE_LEN = (0, 1, 4, 5, 14, 15, 16, 17, 18, 19, 20, 63, 64, 65, 269, 270, 271, 273, 274, 275, 524, 525, 2048, 4095,
             4096, 4097)
_EDGE_OFF = (1, 2, 3, 4, 8, 16, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def random_chains():
    """200 random chains (lengths and offsets from the edge values and uniform draws, up to 400
    sequences or 250 KB of output, every third block ending on a match): tokens, extension bytes
    and offsets on every phase of the 2 KiB chunk, the 16 KiB ring wrapped several times."""
    cases = []
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        seqs, have = [], 0
        for _ in range(400):
            ll = int(rng.choice(_EDGE_LEN)) if rng.random() < 0.5 else int(rng.integers(0, 3001))
            ml = int(rng.choice(_EDGE_LEN)) if rng.random() < 0.5 else int(rng.integers(0, 3001))
            ml = max(ml, MIN_MATCH)
            if have + ll == 0:
                ll = 1
            off = int(rng.choice(_EDGE_OFF)) if rng.random() < 0.5 else int(rng.integers(1, 65536))
            off = min(off, have + ll)
            if have + ll + ml > 250_000:
                break
            seqs.append((ll, off, ml))
            have += ll + ml
        tail = None if seed % 3 == 2 else int(rng.integers(0, 40))
        cases.append(_case(f"random-chain seed={seed} sequences={len(seqs)}", seqs, tail, rng, need=262144))
    return cases


def _reach(pos, kind):
    """sequences whose compressed bytes end exactly at block position `pos` -> seqs.  'solo':
    one literal run; 'chain': batched sequences of 100 compressed bytes each."""
    def clen(ll):  # compressed bytes of (ll, off, 4)
        return 1 + (0 if ll < 15 else 1 + (ll - 15) // 255) + ll + 2
    if kind == "chain":
        k = pos // 100 - 2
        seqs = [(96, 1 if j == 0 else 90, 4) for j in range(k)]
        rest = pos - 100 * k  # 200..299: two more sequences
        for a in range(60, 130):
            for b in range(60, 230):
                if clen(a) + clen(b) == rest:
                    return seqs + [(a, 50, 4), (b, 50, 4)]
    for a in (1, 2, 3, 20):
        for ll in range(max(0, pos - 80 - a), pos):
            if clen(a) + clen(ll) == pos:
                return [(a, 1, 4), (ll, 1, 4)]
    raise AssertionError(f"no prefix ends at {pos}")


@functools.lru_cache(maxsize=None)
def ring_sweep():
    """A fixed header group — a token with a 255-extension literal length (277), 277 literals, an
    offset, a 255-extension match length (277) — placed so that its token, and then its offset,
    sits at every compressed position within 10 bytes of the first chunk boundary and of the
    ring's size."""
    rng = np.random.default_rng(51)
    group = (277, 300, 277)  # token, 0xFF, 0x07, literals, offset, 0xFF, 0x03
    cases = []
    i = 0
    for boundary in (CHUNK, CR):
        for what, back in (("token", 0), ("offset", 3 + 277)):
            for d in range(-10, 11):
                for kind in ("solo", "chain"):
                    i += 1
                    pos = boundary + d - back
                    pre = _reach(pos, kind)
                    blk, _, marks = synth_marks(pre + [group], 5, np.random.default_rng(0))
                    tpos, opos, _ = marks[len(pre)]
                    assert (tpos if what == "token" else opos) == boundary + d
                    cases.append(_case(f"ring-sweep {what}-at={boundary}{d:+d} prefix={kind} group=(277,300,277) "
                                       f"then (2,5,6)", pre + [group, (2, 5, 6)], 5 if i & 1 else None, rng))
    return cases


@functools.lru_cache(maxsize=None)
def boundary_codes():
    """The length-extension boundary points (a length of exactly 15 + 255 k, whose code ends in a
    zero byte) written with noncanonical=True and without, and degenerate blocks."""
    rng = np.random.default_rng(61)
    cases = []
    for nc in (True, False):
        for ll in (15, 270, 525, 780, 14, 16):
            for ml in (19, 274, 529, 784, 18, 20):
                for tail in (5, 15, 270, None):
                    pre, name = _filler(300 - ll, 1)
                    blk, out = synth(pre + [(ll, 300, ml)], tail, rng, noncanonical=nc)
                    end = "match" if tail is None else f"lit{tail}"
                    cases.append(Case(f"length-code noncanonical={nc} ll={ll} off=300 ml={ml} prefix={name} "
                                      f"end={end}", blk, out, len(out)))
    cases.append(Case("degenerate block=00 (valid, nothing out)", b"\x00", b"", 16))
    cases.append(Case("degenerate block=10 'a'", b"\x10a", b"a", 16))
    for n in range(1, 21):
        blk, out = synth([], n, rng)
        cases.append(Case(f"degenerate literal-only tail={n}", blk, out, 16))
    cases.append(Case("degenerate one token and one match (offset 1 before any output)", b"\x00\x01\x00", None, 16))
    cases.append(Case("degenerate one literal, offset 1, match 4", b"\x10a\x01\x00", b"aaaaa", 16))
    return cases


def capacity(S):
    """For every kind of ending, a block of exactly S bytes (fits slot S) and one of S + 1 (must
    be rejected), each between valid neighbours that fill their slots to the last byte ->
    cases for ONE launch with slot = S, in launch order."""
    assert S % 16 == 0 and S >= 6000
    rng = np.random.default_rng(71 + S)
    body = [(40, 20, 60)] * 8  # 800 bytes, batched
    have = 800

    def ending(kind, total):
        rest = total - have
        if kind == "short literal in a batch":
            return body + [(rest - 5 - 40, 700, 40)], 5
        if kind == "match in a batch":
            return body + [(7, 700, rest - 7)], None
        if kind == "solo literal":
            return body + [(rest - 5000 - 30, 700, 30)], 5000
        if kind == "solo match":
            return body + [(3, 700, rest - 3)], None
        raise ValueError(kind)

    def full(j):
        seqs, tail = ending(("short literal in a batch", "match in a batch", "solo literal", "solo match")[j % 4], S)
        return _case(f"capacity neighbour filling slot={S}", seqs, tail, rng, need=S)

    cases, j = [full(0)], 1
    for kind in ("short literal in a batch", "match in a batch", "solo literal", "solo match"):
        for over in (0, 1):
            # rest of a batched ending stays <= SOLO, of a solo ending > SOLO
            if kind.endswith("batch"):
                pad = [(1000, 1, 2000)] * max(0, -(-(S - have - 3900) // 3000))
            else:
                pad = []
            seqs, tail = ending(kind, S + over - sum(ll + ml for ll, _, ml in pad))
            blk, out = synth(pad + seqs, tail, rng)
            assert len(out) == S + over
            cases.append(Case(f"capacity ending='{kind}' content={S + over} slot={S} last-seq={seqs[-1]} tail={tail}",
                              blk, None if over else out, S))
            cases.append(full(j))
            j += 1
    return cases


def malformed_bases():
    """~30 valid blocks that between them take the fast chain, the careful path and the alone
    path -> [(label, seqs, tail)]"""
    bases = []
    for tail in (5, None):
        bases += [
            ("fast short", [(3, 1, 5), (2, 4, 6), (0, 3, 4), (7, 9, 12)], tail),
            ("fast 20 minimal", [(4, 1, 4)] + [(0, 3, 4)] * 20, tail),
            ("fast one-byte extensions", [(20, 5, 30), (100, 40, 200), (16, 90, 19)], tail),
            ("careful 255-extensions", [(300, 100, 300), (270, 7, 274), (525, 600, 20)], tail),
            ("careful then fast", [(600, 1, 4), (3, 2, 5), (0, 1, 4), (280, 280, 280)], tail),
            ("solo literal", [(4, 1, 4), (4200, 5, 40), (3, 100, 10)], tail),
            ("solo match", [(16, 8, 8), (0, 24, 4200), (2, 1, 5)], tail),
            ("solo boundary 4096/4097", [(16, 8, 8), (4092, 13, 4), (4093, 13, 4)], tail),
            ("two batches", [(16, 1, 240)] + [(16, 100, 240)] * 33, tail),
            ("65 minimal (two batches by count)", [(4, 1, 4)] + [(0, 3, 4)] * 65, tail),
            ("look-ahead literals", [(3, 1, 5), (4090, 2, 4), (2, 9, 6)], tail),
            ("past the first chunk", [(97, 1, 4)] + [(97, 90, 4)] * 24 + [(277, 300, 277)], tail),
        ]
    bases += [
        ("literal only 4", [], 4), ("literal only 300", [], 300), ("literal only alone 5000", [], 5000),
        ("one match", [(1, 1, 4)], None), ("one match then nothing", [(1, 1, 4)], 0),
        ("long ring literal", [(18000, 17000, 300), (2, 5, 6)], 5),
    ]
    return bases


@functools.lru_cache(maxsize=None)
def malformed():
    """Blocks derived from malformed_bases(): proper prefixes (all of a block up to 64 bytes, 64
    evenly spaced of a longer one), and for the first, middle and last sequence: the offset set
    to 0, the offset set to di + 1, the literal-length nibble raised so that the literals
    overrun the block, and the final token given a match nibble.  `content` is left None here:
    the expected verdict (and bytes, where a mutated block is still valid) comes from a host
    decoder at the launch's slot size — see expect()."""
    rng = np.random.default_rng(81)
    cases = []
    for name, seqs, tail in malformed_bases():
        blk, out, marks = synth_marks(seqs, tail, rng)
        need = max(len(out), 16)
        end = "match" if tail is None else f"lit{tail}"
        base = f"malformed base='{name}' ({len(seqs)} sequences, end={end}, {len(blk)} bytes)"
        cuts = range(len(blk)) if len(blk) <= 64 else sorted({(len(blk) * j) // 64 for j in range(64)})
        for cut in cuts:
            cases.append(Case(f"{base} prefix of {cut} bytes", blk[:cut], None, need))
        with_match = [m for m in marks if m[1] is not None]
        picks = {0, len(with_match) // 2, len(with_match) - 1} if with_match else set()
        for k in sorted(picks):
            tpos, opos, di = with_match[k]
            ll, off, ml = seqs[k]
            b = bytearray(blk)
            b[opos:opos + 2] = b"\x00\x00"
            cases.append(Case(f"{base} sequence {k} (ll={ll},off={off},ml={ml}) offset=0", bytes(b), None, need))
            if di + 1 <= 65535:
                b = bytearray(blk)
                b[opos:opos + 2] = (di + 1).to_bytes(2, "little")
                cases.append(Case(f"{base} sequence {k} (ll={ll},off={off},ml={ml}) offset=di+1={di + 1}", bytes(b),
                                  None, need))
            # the literal-length nibble raised: 15 reads the next byte(s) as an extension
            b = bytearray(blk)
            b[tpos] |= 0xF0
            cases.append(Case(f"{base} sequence {k} (ll={ll},off={off},ml={ml}) literal nibble=15", bytes(b), None,
                              need))
            if ll < 14:
                b = bytearray(blk)
                b[tpos] = (b[tpos] & 0x0F) | ((ll + 1) << 4)
                cases.append(Case(f"{base} sequence {k} (ll={ll},off={off},ml={ml}) literal nibble+1", bytes(b),
                                  None, need))
        if tail is not None:  # the final token given a match nibble
            tpos = marks[-1][0]
            for nib in (1, 15):
                b = bytearray(blk)
                b[tpos] |= nib
                cases.append(Case(f"{base} final token match nibble={nib}", bytes(b), None, need))
    return cases


def expect(cases, slot, decoder):
    """cases with `content` set to decoder(block, slot) (None: rejected)"""
    return [c._replace(content=decoder(c.block, slot)) for c in cases]

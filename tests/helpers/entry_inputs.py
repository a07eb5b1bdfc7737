"""TEST INFRASTRUCTURE -- archives whose seek-table ENTRIES are chains of Zstandard frames and skippable frames, for the tests of
zk_refine_entries (tests/test_refine_entries.py on the CPU, tests/test_gpu_refine_entries.py on the device), and what refining them must
give.  Everything is deterministic, small and assembled from pieces; nothing here touches the product.

Pieces: Zstandard frames of 0 .. 64 KiB of content from the oracle's encoder (zko.frame_encode), from libzstd as zeekstd drives it
(encode_seekable_frames: no Frame_Content_Size, so the sequence walk must size them) and in one shot (encode_oneshot_frames: with it), with
and without checksums, from the frame generator (zstd_gen.generate: every header form, several blocks), and empty frames; skippable frames
with magic nibbles 0, 5, 0xE, 0xF and 0, 1, 7, 8, 100 bytes of content.

The EXPECTED refined table is not the product's: `split` is a pure-Python entry walk (frame header, block hops, skippable sizes) and the
sizes are what libzstd 1.5.7 hands out for each piece (decode_stream_verdict)."""
import collections
import functools
import random
import struct

import numpy as np

from helpers import zstd_gen
from oracle import libzstd_ref as Z
from oracle import zko

JUDGE = "1.5.7" if Z.load("1.5.7") is not None else "system"
ZSTD_MAGIC = 0xFD2FB528
SKIP_NIBBLES = (0, 5, 0xE, 0xF)
SKIP_SIZES = (0, 1, 7, 8, 100)

Piece = collections.namedtuple("Piece", "comp data")        # one frame and what it decodes to (b"" for a skippable frame)
# c / d: the entries' prefix sums (d None: nobody knows the sizes); pieces: per entry the list of Piece it was built from (None where the
# entry was damaged afterwards)
Archive = collections.namedtuple("Archive", "name comp c d pieces")
# what refining gives: the refined prefix sums, the input entry of every refined entry, the set of bad input entries, and -- for entries
# that are whole frames to `split` -- whether libzstd refuses one of them (bad_deep) or the structure alone decides (bad - bad_deep).
# lax: entries libzstd decodes although one of their frames is not valid Zstandard (format_refuses): libzstd is laxer than the format in
# places (judge_damaged, oracle/libzstd_ref.py), so a decoder may refuse them as well -- the one case where two verdicts are right
Refined = collections.namedtuple("Refined", "c d entry_of bad bad_deep lax")


# ---------------------------------------------------------------------------------------------- pieces
def skippable(nibble, n, seed=0):
    body = bytes((seed * 31 + i * 7 + nibble) & 0xFF for i in range(n))
    return Piece(struct.pack("<II", 0x184D2A50 | nibble, n) + body, b"")


@functools.lru_cache(maxsize=None)
def skips():
    return [skippable(nb, n, k) for k, (nb, n) in enumerate((nb, n) for nb in SKIP_NIBBLES for n in SKIP_SIZES)]


def _cut(comp, sizes, data):
    out, cp, dp = [], 0, 0
    for cs, ds in sizes:
        out.append(Piece(comp[cp:cp + cs], data[dp:dp + ds]))
        cp += cs; dp += ds
    assert cp == len(comp) and dp == len(data)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """the Zstandard frames every archive is assembled from, each checked against libzstd once"""
    out = []
    for i, n in enumerate((100, 333, 1000, 4097, 20000, 65536)):
        data = zko.gen_text(n, 900 + i) if i % 2 == 0 else zko.gen_chunks(n, 40 + i)
        out.append(Piece(zko.frame_encode(data, 1 + (i % 2), bool(i & 1)), data))
    for cks in (False, True):
        data = zko.gen_text(100000, 77 + cks)
        out += _cut(*Z.encode_seekable_frames(data, 17000, 1 + 2 * cks, cks, which=JUDGE), data)
        data = zko.gen_chunks(40000 if cks else 1400, 5 + cks)
        out += _cut(*Z.encode_oneshot_frames(data, 9000 if cks else 140, 3, cks, which=JUDGE), data)
        out += _cut(*Z.encode_seekable_frames(b"", 1000, 1, cks, which=JUDGE), b"")
    out.append(Piece(zko.frame_encode(b"", 1, False), b""))
    out.append(Piece(zko.frame_encode(b"", 1, True), b""))
    for seed in range(870000, 870040):
        f, data, _ = zstd_gen.generate(seed, zko.xxh64)
        out.append(Piece(f, data))
    for p in out:
        assert Z.decode_stream(p.comp, len(p.data), which=JUDGE) == p.data
    assert any(len(p.data) == 0 for p in out) and any(len(p.data) == 65536 for p in out)
    return out


def _archive(name, entries, sized=True):
    comp = b"".join(p.comp for e in entries for p in e)
    c = np.zeros(len(entries) + 1, np.uint64)
    d = np.zeros(len(entries) + 1, np.uint64)
    c[1:] = np.cumsum([sum(len(p.comp) for p in e) for e in entries])
    d[1:] = np.cumsum([sum(len(p.data) for p in e) for e in entries])
    return Archive(name, comp, c, d if sized else None, tuple(tuple(e) for e in entries))


def plain_bytes(a):
    return b"".join(p.data for e in a.pieces for p in e)


def head(a, n):
    """the archive of a's first n entries"""
    return Archive("%s[:%d]" % (a.name, n), a.comp[:int(a.c[n])], a.c[:n + 1].copy(), None if a.d is None else a.d[:n + 1].copy(), a.pieces[:n])


# ---------------------------------------------------------------------------------------------- archives
@functools.lru_cache(maxsize=None)
def identity():
    return _archive("identity", [[p] for p in pool()])


@functools.lru_cache(maxsize=None)
def coarse():
    """70 entries of 1 .. 40 frames, a skippable frame now and then: more than 1024 refined entries"""
    rng, P, S = random.Random(4242), pool(), skips()
    small = [p for p in P if len(p.comp) < 3000]
    counts = [1, 40, 2, 39] + [rng.randint(1, 40) for _ in range(66)]
    entries = []
    for k in counts:
        e = []
        for _ in range(k):
            r = rng.random()
            e.append(rng.choice(S) if r < 0.08 else rng.choice(P) if r < 0.2 else rng.choice(small))
        entries.append(e)
    a = _archive("coarse", entries)
    assert len(entries) == 70 and sum(counts) > 1024
    return a


@functools.lru_cache(maxsize=None)
def skip_entries():
    """skippable frames as entries of their own; first, in the middle and last inside an entry; two adjacent"""
    P, S = pool(), skips()
    entries = [[s] for s in S]
    entries += [[S[3], P[0], P[7]], [P[1], S[9], P[2]], [P[8], P[3], S[14]], [P[4], S[0], S[19], P[9]], [S[5], S[6]], [P[5]], [S[12]], [P[20], S[1]]]
    empty = [p for p in P if not p.data]                     # empty Zstandard frames (one block each), with and without a checksum
    assert len(empty) >= 4
    entries += [[empty[0]], [empty[1], S[8], empty[2]], [S[10], empty[3]]]
    return _archive("skips", entries)


@functools.lru_cache(maxsize=None)
def pzstd():
    """a 12-byte skippable frame (the size of the frame behind it) in front of every frame, as pzstd writes them"""
    entries = [[Piece(struct.pack("<III", 0x184D2A50, 4, len(p.comp)), b""), p] for p in pool()[:40]]
    return _archive("pzstd", entries)


@functools.lru_cache(maxsize=None)
def plain():
    """300 frames as ONE entry without sizes: a plain multi-frame stream"""
    rng, P = random.Random(99), pool()
    small = [p for p in P if len(p.comp) < 3000]
    return _archive("plain", [[rng.choice(small) if i % 10 else rng.choice(P) for i in range(300)]], sized=False)


GOOD = (identity, coarse, skip_entries, pzstd, plain)
FLIP_SEED = 20250                                           # fixed on the CPU: tests/test_refine_entries.py asserts what it must give
FLIP_ENTRIES = 600


@functools.lru_cache(maxsize=None)
def damaged():
    """600 entries of three frames, one to three flipped bits in the MIDDLE frame of about 150 of them; behind them entries with a truncated
    last frame, 1 .. 3 and 4 or more junk bytes behind the frames, a skippable size field that runs past the entry, and an entry whose size
    disagrees with the sum of its frames.  -> (Archive, {entry: what was done to it})"""
    rng, P, S = random.Random(FLIP_SEED), pool(), skips()
    small = [p for p in P if 20 < len(p.comp) < 1500]
    entries = [[rng.choice(small), rng.choice(small), rng.choice(small)] for _ in range(FLIP_ENTRIES)]
    junk = lambda n: Piece(bytes(rng.randrange(1, 256) for _ in range(n)), b"")
    cut = P[2].comp[:len(P[2].comp) - 5]
    specials = [("truncated", [P[0], Piece(cut, P[2].data)]),
                ("junk1", [P[1], junk(1)]), ("junk2", [P[1], P[0], junk(2)]), ("junk3", [P[3], junk(3)]),
                ("junk4", [P[0], junk(4)]), ("junk9", [P[1], junk(9)]), ("junk40", [P[0], P[1], junk(40)]),
                ("skip_past", [P[0], Piece(struct.pack("<II", 0x184D2A55, 50) + b"x" * 20, b"")]),
                ("skip_short", [P[0], Piece(struct.pack("<I", 0x184D2A5E) + b"\1\0", b"")]),
                ("size_wrong", [P[1], P[0]]), ("good", [P[0], S[2], P[1]])]
    what = {}
    for name, e in specials:
        what[len(entries)] = name
        entries.append(e)
    a = _archive("damaged", entries)
    comp = bytearray(a.comp)
    d = a.d.copy()
    for e in sorted(rng.sample(range(FLIP_ENTRIES), 150)):
        lo = int(a.c[e]) + len(entries[e][0].comp)
        hi = lo + len(entries[e][1].comp)
        for _ in range(rng.randint(1, 3)):
            comp[rng.randrange(lo, hi)] ^= 1 << rng.randrange(8)
        what[e] = "flip"
    k = next(i for i, n in what.items() if n == "size_wrong")
    d[k + 1:] += np.uint64(1)
    return Archive("damaged", bytes(comp), a.c, d, a.pieces), what


# ---------------------------------------------------------------------------------------------- the expected result
def split(comp, begin, end):
    """The entry walk in plain Python -> (first bytes of the pieces, why it stopped).  A whole number of frames: stop is None and the
    pieces are the frames; otherwise the last piece is whatever begins where the walk could not go on."""
    starts, p = [], begin
    while True:
        starts.append(p)
        left = end - p
        if left < 4:
            return starts, "fewer than 4 bytes"
        magic = int.from_bytes(comp[p:p + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if left < 8:
                return starts, "skippable header cut"
            q = 8 + int.from_bytes(comp[p + 4:p + 8], "little")
        elif magic == ZSTD_MAGIC:
            if left < 6:
                return starts, "frame header cut"
            fhd = comp[p + 4]
            single, did, fcs = (fhd >> 5) & 1, fhd & 3, fhd >> 6
            q = 5 + (0 if single else 1) + (4 if did == 3 else did) + (single if fcs == 0 else 1 << fcs)
            while True:
                if q + 3 > left:
                    return starts, "block header cut"
                bh = int.from_bytes(comp[p + q:p + q + 3], "little")
                if (bh >> 1) & 3 == 3:
                    return starts, "reserved block type"
                q += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
                if q > left:
                    return starts, "block cut"
                if bh & 1:
                    break
            if fhd & 4:
                q += 4
        else:
            return starts, "no magic"
        if q > left:
            return starts, "frame runs past the entry"
        p += q
        if p == end:
            return starts, None


_VERDICTS = {}


def libzstd_verdict(piece):
    """decode_stream_verdict of libzstd 1.5.7 on these bytes, cached: (bytes handed out, "end" / "more" / the error)"""
    piece = bytes(piece)
    if piece not in _VERDICTS:
        _VERDICTS[piece] = Z.decode_stream_verdict(piece, which=JUDGE)
    return _VERDICTS[piece]


_FORMAT = {}


def format_refuses(piece):
    """the oracle's restatement of the format (zko.frame_decode) does not take these bytes as one whole Zstandard frame"""
    piece = bytes(piece)
    if piece not in _FORMAT:
        try:
            _, used = zko.frame_decode(piece, (1 << 20), True)
            _FORMAT[piece] = used != len(piece)
        except zko.OracleError:
            _FORMAT[piece] = True
    return _FORMAT[piece]


def entry_verdict(a, e):
    """libzstd on the whole entry -> its bytes if it decodes the entry to its end (and to the entry's size, where the table states one), else None"""
    out, state = libzstd_verdict(a.comp[int(a.c[e]):int(a.c[e + 1])])
    if state != "end" or (a.d is not None and len(out) != int(a.d[e + 1] - a.d[e])):
        return None
    return out


def refined(a):
    """what zk_refine_entries must return for archive a"""
    c_ref, d_ref, entry_of, bad, deep, lax = [], [], [], set(), set(), set()
    dpos = int(a.d[0]) if a.d is not None else 0
    for e in range(len(a.c) - 1):
        cb, ce = int(a.c[e]), int(a.c[e + 1])
        starts, stop = split(a.comp, cb, ce)
        sizes = []
        if stop is None:
            for s, t in zip(starts, starts[1:] + [ce]):
                out, state = libzstd_verdict(a.comp[s:t])
                if state != "end":
                    deep.add(e)
                    break
                sizes.append(len(out))
        want = int(a.d[e + 1] - a.d[e]) if a.d is not None else None
        if stop is not None or e in deep or (want is not None and sum(sizes) != want):
            bad.add(e)
            c_ref.append(cb); d_ref.append(dpos); entry_of.append(e)
            dpos += want or 0
            continue
        for s, t, n in zip(starts, starts[1:] + [ce], sizes):
            c_ref.append(s); d_ref.append(dpos); entry_of.append(e)
            dpos += n
            if int.from_bytes(a.comp[s:s + 4], "little") == ZSTD_MAGIC and format_refuses(a.comp[s:t]):
                lax.add(e)
    c_ref.append(int(a.c[-1])); d_ref.append(dpos)
    return Refined(np.array(c_ref, np.uint64), np.array(d_ref, np.uint64), np.array(entry_of, np.uint32), bad, deep, lax)

"""Named, deterministic inputs that drive the ENCODER's entropy stage (zk_k_enc_fse_build / zk_k_enc_entropy / zk_k_enc_sizes /
zk_k_enc_assemble and their CPU twin oracle/zstd_oracle_enc.c) to the edges of the format: every literals header form, the Huffman
length limit, the ends of the literal alphabet, RLE and empty literals inside a compressed block, more than 4096 sequences in a
block, the per-frame table thresholds, a defining block that is not a frame's first.

An entry is (name, data, frame_size, level, features).  `features` is the set of facts that must hold for the frames an encoder
makes of it; every fact is a string that `reached()` reads back from the frames themselves with a block walker (`walk_frame`,
RFC 8878 3.1.1.2 / 3.1.1.3), so a test can ask "did what you wrote go down the path this input is here for" of the twin's
frames and of the GPU's alike.  Seeds and lengths were tuned with the twin until the facts held and are frozen here;
tests/test_encode_edges.py is the guard that notices when a change to the matcher moves an input off its path.

The facts (b = one block, f = one frame):
  block=raw|rle|comp                       a block of that type exists
  lit=raw|rle|huf/sf=S/nlit=N              a compressed block's literals section: type, Size_Format, Regenerated_Size
  .../nseq=0                               the same for a block without sequences
  lit=raw/hdr=H/nlit=N                     raw literals inside a compressed block, H header bytes
  lit=huf/sf=3/nlit>=16384                 the 5-byte Huffman header is in use
  tree=B                                   Huffman tree description byte
  huf_symbols=K                            symbols with a code
  fFbK/huf_depth=D                         longest code of frame F's block K
  lit=rle/nseq>0, comp/nlit=0, nseq>4096   what they say
  frame_nseq=N                             sequences of a frame
  modes=all_00                             every block with sequences of a frame says Predefined_Mode
  def=0xXX@K                               first block of a frame whose modes byte is not a Repeat/Predefined form: byte and index
  after_def=repeat                         every later block with sequences of that frame says Repeat_Mode where the defining one says
                                           FSE_Compressed_Mode (0xA8 -> 0xFC), and there is such a block
  def_late                                 the same with 0xA8 at an index > 0
  fFbK/raw|rle|lit=raw|lit=rle|lit=huf     what frame F's block K is: a raw or RLE block, or a compressed one with such literals
  logs=a/b/c                               accuracy logs of the three descriptions in the defining block
  modes_mixed_0_2                          a defining modes byte that mixes Predefined_Mode and FSE_Compressed_Mode

`table_stays_predefined` (a frame with >= 256 sequences in which one of LL / OF / ML has a single code, so that zke_fse_normalize
returns false and that table alone stays predefined) is documented at its builder below.
"""
import collections
import functools

import numpy as np

from oracle import zko

Entry = collections.namedtuple("Entry", "name data frame_size level features")


# ---------------------------------------------------------------------------------------------- the block walker
def _fse_ncount_len(b, at):
    """-> (accuracy log, bytes) of the FSE table description at b[at:] (RFC 8878 4.1.1)"""
    v = int.from_bytes(b[at:at + 96], "little")
    al = (v & 15) + 5
    pos, remaining, sym = 4, (1 << al) + 1, 0
    while remaining > 1 and sym < 256:
        nb = remaining.bit_length()                     # bits of the largest value, remaining
        low = (1 << nb) - 1 - remaining                 # values below it are written with one bit less
        x = (v >> pos) & ((1 << (nb - 1)) - 1)
        if x < low:
            pos += nb - 1
        else:
            x = (v >> pos) & ((1 << nb) - 1)
            if x >= (1 << (nb - 1)):
                x -= low
            pos += nb
        prob = x - 1
        remaining -= abs(prob) if prob else 0
        sym += 1
        if prob == 0:
            while True:
                rep = (v >> pos) & 3
                pos += 2
                sym += rep
                if rep != 3:
                    break
    return al, (pos + 7) // 8


def _huf_tree(b, at):
    """direct-weight tree description at b[at:] -> (description byte, symbols with a code, longest code)"""
    hb = b[at]
    assert hb >= 128, "the encoder writes direct weights only"
    n = hb - 127
    ws = []
    for i in range(n):
        x = b[at + 1 + i // 2]
        ws.append(x >> 4 if i % 2 == 0 else x & 15)
    total = sum(1 << (w - 1) for w in ws if w)
    maxbits = total.bit_length()                        # the implied last weight completes a power of two
    rest = (1 << maxbits) - total
    assert rest & (rest - 1) == 0 and rest > 0
    ws.append(rest.bit_length())
    used = [w for w in ws if w]
    return hb, len(used), maxbits + 1 - min(used)


def walk_frame(f):
    """The blocks of ONE frame as dicts: type ('raw' | 'rle' | 'comp'), size (Block_Size), and for a compressed block lit
    ('raw' | 'rle' | 'huf'), sf (Size_Format), lit_hdr (header bytes), nlit, lit_csize, tree / huf_symbols / huf_depth (Huffman),
    nseq, modes (None without sequences), logs (the accuracy logs of the descriptions the block carries, None per table without)."""
    f = bytes(f)
    assert f[:4] == b"\x28\xb5\x2f\xfd"
    fhd = f[4]
    single, fcs = (fhd >> 5) & 1, fhd >> 6
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fcs]
    out = []
    while True:
        h = int.from_bytes(f[p:p + 3], "little")
        p += 3
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        assert btype != 3
        blk = {"type": ("raw", "rle", "comp")[btype], "size": bsize}
        if btype == 2:
            b = f[p:p + bsize]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            assert lt != 3, "no treeless literals from this encoder"
            v = int.from_bytes(b[:5], "little")
            if lt < 2:
                hdr = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                nlit = v >> 3 & 0x1F if hdr == 1 else v >> 4 & 0xFFF if hdr == 2 else v >> 4 & 0xFFFFF
                csz = 1 if lt == 1 else nlit
            else:
                hdr = 3 if sf < 2 else 4 if sf == 2 else 5
                bits = 10 if hdr == 3 else 14 if hdr == 4 else 18
                nlit, csz = v >> 4 & ((1 << bits) - 1), v >> (4 + bits) & ((1 << bits) - 1)
                blk["tree"], blk["huf_symbols"], blk["huf_depth"] = _huf_tree(b, hdr)
            blk.update(lit=("raw", "rle", "huf")[lt], sf=sf, lit_hdr=hdr, nlit=nlit, lit_csize=csz)
            q = hdr + csz
            nseq = b[q]
            if nseq < 128:
                q += 1
            elif nseq < 255:
                nseq = ((nseq - 128) << 8) + b[q + 1]; q += 2
            else:
                nseq = b[q + 1] + (b[q + 2] << 8) + 0x7F00; q += 3
            blk["nseq"], blk["modes"], blk["logs"] = nseq, None, None
            if nseq:
                m = blk["modes"] = b[q]
                q += 1
                logs = []
                for t in range(3):
                    mode = (m >> (6 - 2 * t)) & 3
                    if mode == 2:
                        al, n = _fse_ncount_len(b, q)
                        logs.append(al); q += n
                    else:
                        assert mode != 1, "no RLE tables from this encoder"
                        logs.append(None)
                blk["logs"] = tuple(logs)
            assert q <= bsize
        p += 1 if btype == 1 else bsize
        out.append(blk)
        if last:
            break
    assert p + (4 if fhd & 4 else 0) == len(f), "the walk ends with the frame"
    return out


def reached(frames):
    """The set of facts (module docstring) that hold for these frames (each one frame's bytes)."""
    facts = set()
    for fi, f in enumerate(frames):
        blocks = walk_frame(f)
        withseq = [(k, b) for k, b in enumerate(blocks) if b["type"] == "comp" and b["nseq"]]
        for k, b in enumerate(blocks):
            facts.add("block=" + b["type"])
            facts.add(f"f{fi}b{k}/" + (b["type"] if b["type"] != "comp" else "lit=" + b["lit"]))
            if b["type"] != "comp":
                continue
            s = f"lit={b['lit']}/sf={b['sf']}/nlit={b['nlit']}"
            facts.add(s)
            if b["nseq"] == 0:
                facts.add(s + "/nseq=0")
            if b["lit"] == "raw":
                facts.add(f"lit=raw/hdr={b['lit_hdr']}/nlit={b['nlit']}")
            if b["lit"] == "huf":
                if b["sf"] == 3 and b["nlit"] >= 16384:
                    facts.add("lit=huf/sf=3/nlit>=16384")
                facts.add(f"tree={b['tree']}")
                facts.add(f"huf_symbols={b['huf_symbols']}")
                facts.add(f"f{fi}b{k}/huf_depth={b['huf_depth']}")
            if b["lit"] == "rle" and b["nseq"] > 0:
                facts.add("lit=rle/nseq>0")
            if b["nlit"] == 0:
                facts.add("comp/nlit=0")
            if b["nseq"] > 4096:
                facts.add("nseq>4096")
        facts.add(f"frame_nseq={sum(b['nseq'] for _, b in withseq)}")
        if withseq and all(b["modes"] == 0 for _, b in withseq):
            facts.add("modes=all_00")
        for i, (k, b) in enumerate(withseq):
            m = b["modes"]
            if any((m >> s) & 3 == 2 for s in (2, 4, 6)):
                facts.add(f"def=0x{m:02X}@{k}")
                facts.add("logs=" + "/".join("-" if a is None else str(a) for a in b["logs"]))
                fields = {(m >> s) & 3 for s in (2, 4, 6)}
                if fields == {0, 2}:
                    facts.add("modes_mixed_0_2")
                rep = m | m >> 1 & 0x54                                  # 2 -> 3 in every field
                if len(withseq) > i + 1 and all(x["modes"] == rep for _, x in withseq[i + 1:]):
                    facts.add("after_def=repeat")
                    if k > 0 and m == 0xA8:
                        facts.add("def_late")
                break
    return facts


def split_frames(comp, frames):
    """(payload, [(c_size, d_size)]) as encode_frames returns it -> the frames' bytes"""
    out, pos = [], 0
    for c, _ in frames:
        out.append(comp[pos:pos + c]); pos += c
    return out


def twin_frames(e, checksum=True):
    """the entry's frames as the CPU twin encodes them"""
    return [zko.frame_encode(e.data[o:o + e.frame_size], e.level, checksum) for o in range(0, max(len(e.data), 1), e.frame_size)]


def huffman_depth(counts):
    """depth of the unrestricted two-queue Huffman tree over the counts > 0 (what zke_huf_lengths builds before it looks at the limit)"""
    leaves = collections.deque(sorted(c for c in counts if c))
    inner = collections.deque()                                          # (weight, depth below)
    if len(leaves) < 2:
        return 0
    leaves = collections.deque((c, 0) for c in leaves)
    while len(leaves) + len(inner) > 1:
        two = []
        for _ in range(2):
            two.append(leaves.popleft() if leaves and (not inner or leaves[0][0] <= inner[0][0]) else inner.popleft())
        inner.append((two[0][0] + two[1][0], max(two[0][1], two[1][1]) + 1))
    return inner[0][1]


# ---------------------------------------------------------------------------------------------- generators
def skewed(n, nsym, seed, base=0, power=1.0, shift=0.0):
    """n i.i.d. bytes over nsym symbols from `base` on, p proportional to 1 / (rank + shift) ** power"""
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(1, nsym + 1) + shift) ** power
    return (rng.choice(nsym, n, p=p / p.sum()) + base).astype(np.uint8).tobytes()


def once_used(seps, seed, vocab_bytes, avoid=(), shuffle=False, tok=7, stride=None, back=None):
    """A vocabulary of random bytes, then a stream of len(seps) x (separator byte + a token of `tok` vocabulary bytes), every token
    used ONCE: a token's only earlier occurrence is the vocabulary's, where another byte stands in front of and behind it, so the
    matcher takes every token as one match of exactly `tok` bytes and leaves exactly the separators as literals -- the block's
    literals are `seps`, byte for byte.  `avoid`: byte values the vocabulary does not contain (the separators').
    Tokens are taken `stride` bytes apart from `back` bytes before the stream on (default: the vocabulary's start, back to back),
    or in a random order (shuffle)."""
    rng = np.random.default_rng(seed)
    ok = np.array([v for v in range(256) if v not in set(avoid)], np.uint8)
    voc = ok[rng.integers(0, len(ok), vocab_bytes)]
    n = len(seps)
    stride = stride or tok
    first = vocab_bytes - back if back else 0
    at = first + stride * np.arange(n)
    assert at[-1] + tok <= vocab_bytes
    if shuffle:
        at = rng.permutation(at)
    stream = np.empty((n, 1 + tok), np.uint8)
    stream[:, 0] = np.frombuffer(bytes(seps), np.uint8)
    stream[:, 1:] = voc[at[:, None] + np.arange(tok)[None, :]]
    return voc.tobytes(), stream.tobytes()


# ---------------------------------------------------------------------------------------------- the inputs
MIB = 1 << 20
_B = {}


def _entry(name):
    def deco(fn):
        _B[name] = fn
        return fn
    return deco


def _e(name, data, level, features, frame_size=None):
    return Entry(name, bytes(data), frame_size or max(len(data), 1), level, frozenset(features))


@_entry("lit_huf_5byte")
def _():
    # 90 printable symbols, p ~ 1 / rank, no matches to speak of: ~32 000 literals per 32 KiB block, four streams of ~5 KiB
    return _e("lit_huf_5byte", skewed(MIB, 90, 1, base=33), 1, {"lit=huf/sf=3/nlit>=16384"})


def _tail(extra):
    # 128 symbols, mildly skewed: no sequence in the whole frame; 16 blocks of 32 KiB and a last one of `extra` bytes
    sf = 2 if extra < 16384 else 3
    return _e(f"lit_huf_edges/tail{extra}", skewed((512 << 10) + extra, 128, 1, shift=20.0), 1,
              {f"lit=huf/sf={sf}/nlit={extra}/nseq=0", "lit=huf/sf=3/nlit>=16384"})


for _x in (16383, 16384, 16385):
    _B[f"lit_huf_edges/tail{_x}"] = functools.partial(_tail, _x)

SWEEP_SIZES = list(range(56, 201)) + [1022, 1023, 1024, 1025, 1026]


def _sweep_facts(n):
    # Without sequences raw literals cost a header more than a raw block, so below the gate (64 literals) the block itself goes out
    # raw; from 64 on Huffman wins on these 16 symbols (tree 9 bytes + jump table 6): 3-byte header below 1024 literals, 4 from there.
    return {"block=raw"} if n < 64 else {f"lit=huf/sf={1 if n < 1024 else 2}/nlit={n}/nseq=0"}


def huf_edge_sweep(many=False):
    """lit_huf_edges, the small frames: match-free bytes over 16 symbols, as ONE frame of n bytes for every n of SWEEP_SIZES --
    or (many) as 40 frames of n bytes each, so that the blocks of one entropy workgroup belong to 16 different frames."""
    if many:
        src = skewed(40 * 1026, 16, 6, shift=4.0)
        return [_e(f"lit_huf_edges/40x{n}", src[:40 * n], 1, _sweep_facts(n), frame_size=n) for n in SWEEP_SIZES]
    src = skewed(4096, 16, 5, shift=4.0)
    return [_e(f"lit_huf_edges/n={n}", src[:n], 1, _sweep_facts(n)) for n in SWEEP_SIZES]


def _replay(head, total):
    return (head + head * (total // len(head) + 1))[:total]


# lit_raw_edges: R random bytes, then the same bytes again and again.  The first match starts where the matcher finds it (even
# positions, tiles of 256), so R was searched with the twin until the block's literal count came out as wanted.
@_entry("lit_raw_edges/nlit=31")
def _():
    return _e("lit_raw_edges/nlit=31", _replay(zko.gen_random(31, 7), 4096), 1, {"lit=raw/hdr=1/nlit=31"})


@_entry("lit_raw_edges/nlit=32")
def _():
    return _e("lit_raw_edges/nlit=32", _replay(zko.gen_random(32, 7), 4096), 1, {"lit=raw/hdr=2/nlit=32"})


@_entry("lit_raw_edges/nlit=4095")
def _():
    # two runs of literals: 3000 random bytes, 300 of them again, 1095 more, then the replay (block 0 of 16 blocks of 8 KiB)
    rnd = zko.gen_random(8192, 7)
    d = rnd[:3000] + rnd[:300] + rnd[3000:4095]
    return _e("lit_raw_edges/nlit=4095", d + (rnd[:4095] * 50)[:131072 - len(d)], 1, {"lit=raw/hdr=2/nlit=4095"})


@_entry("lit_raw_edges/nlit=4096")
def _():
    # 4091 random bytes: the tile's last five positions hold no match, the first one starts at 4096
    return _e("lit_raw_edges/nlit=4096", _replay(zko.gen_random(4091, 7), 131072), 1, {"lit=raw/hdr=3/nlit=4096"})


# the Huffman gate (nlit >= 64) inside a compressed block: 63 / 64 literals over 16 symbols, then their replay
@_entry("lit_raw_edges/gate63")
def _():
    return _e("lit_raw_edges/gate63", _replay(skewed(63, 16, 7, shift=4.0), 4096), 1, {"lit=raw/hdr=2/nlit=63"})


@_entry("lit_raw_edges/gate64")
def _():
    return _e("lit_raw_edges/gate64", _replay(skewed(64, 16, 7, shift=4.0), 4096), 1, {"lit=huf/sf=1/nlit=64"})


@_entry("huf_depth_limit")
def _():
    # min(geometric(0.3) - 1, 40) + 40: block histograms like 9791, 6874, 4782, ..., 4, 3, 1, 0, 1 -- the unrestricted tree is 13 deep
    rng = np.random.default_rng(1)
    d = (np.minimum(rng.geometric(0.3, MIB) - 1, 40) + 40).astype(np.uint8).tobytes()
    lits = zko.enc_match_debug(d, 1)[1][1]
    depth = huffman_depth(np.bincount(np.frombuffer(lits, np.uint8), minlength=256))
    assert depth >= 12, depth                            # block 1 needs the count halving of zke_huf_lengths ...
    return _e("huf_depth_limit", d, 1, {"f0b1/huf_depth=11"})      # ... and comes out at the limit


@_entry("alphabet_extremes/two_symbols")
def _():
    rng = np.random.default_rng(3)
    return _e("alphabet_extremes/two_symbols", (rng.integers(0, 2, 70000) * 127).astype(np.uint8).tobytes(), 1, {"huf_symbols=2", "tree=254"})


@_entry("alphabet_extremes/zero_and_127")
def _():
    rng = np.random.default_rng(3)
    p = np.ones(128); p[0] = 30; p[127] = 20
    return _e("alphabet_extremes/zero_and_127", rng.choice(128, 70000, p=p / p.sum()).astype(np.uint8).tobytes(), 1, {"tree=254", "huf_symbols=128"})


def _maxsym(top):
    # the same bytes but for one symbol's value (30-odd of it in every 4 KiB block): 127 keeps the block under the Huffman gate, 128 does not
    c = np.frombuffer(skewed(70000, 100, 4, shift=10.0), np.uint8).copy()
    c[c == 50] = top
    return c.tobytes()


@_entry("alphabet_extremes/maxsym127")
def _():
    return _e("alphabet_extremes/maxsym127", _maxsym(127), 1, {"tree=254", "lit=huf/sf=2/nlit=4096/nseq=0", "f0b0/lit=huf", "f0b1/lit=huf"})


@_entry("alphabet_extremes/maxsym128")
def _():
    return _e("alphabet_extremes/maxsym128", _maxsym(128), 1, {"f0b0/raw", "f0b1/raw"})


@_entry("alphabet_extremes/adjacent_1_4000")
def _():
    # i.i.d. over two adjacent symbols, one in 4000: to the matcher these are byte runs -- all-'A' blocks go out as RLE blocks, the
    # others as a handful of raw literals between offset-1 matches.  (Two symbols under one Huffman code: two_symbols above.)
    rng = np.random.default_rng(3)
    d = np.full(70000, 65, np.uint8); d[rng.integers(0, 70000, 70000 // 4000)] = 66
    return _e("alphabet_extremes/adjacent_1_4000", d.tobytes(), 1, {"block=rle", "lit=raw/hdr=1/nlit=2"})


def _separators(level):
    # 32 KiB of text, then 1500 x (a 40-byte slice of it + 0x7f): a block whose only literals are separators
    src = zko.gen_text(32768, 5)
    rng = np.random.default_rng(3)
    d = src + b"".join(src[o:o + 40] + b"\x7f" for o in rng.integers(0, 32768 - 40, 1500))
    return _e(f"lit_rle/level{level}", d, level, {"lit=rle/nseq>0"})


for _x in (1, 3):
    _B[f"lit_rle/level{_x}"] = functools.partial(_separators, _x)


def _tokens(tok, seed=2):
    rng = np.random.default_rng(seed)
    toks = rng.integers(33, 127, (512, tok)).astype(np.uint8)
    return toks.tobytes() + toks[rng.integers(0, 512, MIB // tok)].tobytes()


@_entry("lit_none")
def _():
    # 512 random printable 8-byte tokens, then a MiB of them drawn at random: blocks of ~4080 sequences and 0, 1, 2, ... literals
    return _e("lit_none", _tokens(8), 3, {"comp/nlit=0", "lit=rle/nseq>0"})


def _over4096(level):
    return _e(f"seq_over_4096/level{level}", _tokens(6), level, {"nseq>4096", "logs=9/8/9"})


for _x in (1, 3):
    _B[f"seq_over_4096/level{_x}"] = functools.partial(_over4096, _x)


# frame_seq_thresholds: prefixes of one text, found by bisection with the twin (the count moves by one every few bytes: no value is skipped)
def _threshold(nseq, n, facts):
    return _e(f"frame_seq_thresholds/{nseq}", zko.gen_text(300000, 9)[:n], 1, {f"frame_nseq={nseq}"} | facts)


_B["frame_seq_thresholds/255"] = functools.partial(_threshold, 255, 6184, {"modes=all_00"})
_B["frame_seq_thresholds/256"] = functools.partial(_threshold, 256, 6212, {"def=0xA8@0", "logs=6/6/6", "after_def=repeat"})
_B["frame_seq_thresholds/16383"] = functools.partial(_threshold, 16383, 184594, {"def=0xA8@0", "logs=6/6/6", "after_def=repeat"})
_B["frame_seq_thresholds/16384"] = functools.partial(_threshold, 16384, 184604, {"def=0xA8@0", "logs=9/8/9", "after_def=repeat"})


def _late(kind, level):
    d = {"raw_raw": lambda: zko.gen_random(70000, 3) + zko.gen_text(600000, 4),
         "rle": lambda: bytes(40000) + zko.gen_text(600000, 4),
         "zero_mid": lambda: zko.gen_text(32768 * 5, 4) + bytes(32768) + zko.gen_text(600000 - 32768 * 6, 5)}[kind]()
    facts = {"raw_raw": {"def=0xA8@2", "def_late", "block=raw"}, "rle": {"def=0xA8@1", "def_late", "block=rle"},
             "zero_mid": {"def=0xA8@0", "after_def=repeat", "block=rle"}}[kind]
    return _e(f"def_block_late/{kind}/level{level}", d, level, facts)


for _k in ("raw_raw", "rle", "zero_mid"):
    for _x in (1, 3):
        _B[f"def_block_late/{_k}/level{_x}"] = functools.partial(_late, _k, _x)


def _predefined(level):
    """table_stays_predefined.  Tried with the twin: fixed records (4 random bytes + 16 constant ones: the tiles' ends cut the matches, LL, OF
    and ML all keep several codes -> 0xA8); a vocabulary as a raw first block + random slices of it (every later block has literals at
    the slices' starts -> 0xA8).  What works: 16 KiB of random bytes without 'A', then 2048 x ('A' + seven of those bytes), every 7-byte
    token used once, in random order.  Every match the matcher finds is one token, exactly 7 bytes (the byte in front of and behind it
    differs at its source), so ML has ONE code, zke_fse_normalize returns false for it and the frame's tables are LL own, OF own, ML
    predefined: modes byte 0xA0 in the defining block, 0xF0 behind it."""
    voc, stream = once_used(bytes([65]) * 2048, 1, 16384, avoid=(65,), shuffle=True)
    return _e(f"table_stays_predefined/level{level}", voc + stream, level, {"def=0xA0@4", "modes_mixed_0_2", "after_def=repeat", "logs=6/6/-"})


for _x in (1, 3):
    _B[f"table_stays_predefined/level{_x}"] = functools.partial(_predefined, _x)

NAMES = list(_B)


@functools.lru_cache(maxsize=None)
def get(name):
    e = _B[name]()
    assert e.name == name
    return e

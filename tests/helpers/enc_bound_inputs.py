"""Named, deterministic inputs that stress the SIZE of what the encoder writes, not its ratio: the cases in which a frame comes closest to
zk_compress_bound() and a block to the format's Block_Maximum_Size.  tests/helpers/enc_inputs.py drives the entropy stage to the format's
edges; this file is about the encoder's memory-safety contract (zk_compress_bound, dst_cap) and is used by tests/test_encode_bound.py (the
CPU twin, no GPU) and tests/test_gpu_encode_bound.py (what the kernels write, and where).

An entry is enc_inputs.Entry: (name, data, frame_size, level, features).  The facts are read back from the frames with
enc_inputs.walk_frame; `reached()` here adds, to the facts of enc_inputs.reached():
  frames=K                 the number of frames
  all_raw                  every block of every frame is a raw block
  raw_exact                every frame is exactly d + 6 + 3 * n_blocks (+ 4 with a checksum) bytes: header, block headers, the input
  def_outgrows=+N          in some frame the defining block (the first one that carries table descriptions) has a Block_Size N bytes ABOVE
                           the bytes it regenerates: zk_k_enc_entropy keeps a block compressed when its Repeat_Mode form is smaller than
                           the block (total < bsz), zk_k_enc_sizes then adds the frame's descriptions to the first such block
  def_grows_by<=N          the frames have defining blocks and none outgrows its input by more than N (N = 0: none outgrows at all)
Seeds and counts were tuned with the twin (oracle/zstd_oracle_enc.c) until the facts held and are frozen here; tests/test_encode_bound.py
is the guard that notices when the matcher moves an input off its path.

The groups:
  all_raw/fs=F             random bytes, 2 F + 1 of them: two whole frames and one of 1 byte, at every frame size where the block count or
                           the block size changes (1 KiB window floor, 4 KiB blocks, 16 blocks per frame, 32 KiB blocks from 512 KiB on, one
                           matcher segment plus a byte).  Nothing compresses: the frame is the input plus every header.
  near_raw/fs=F/lL/CxN     random bytes with C planted matches of N bytes per frame (1 .. 2000 of 5, 6 or 8 bytes): blocks that hover around the
                           "compressed is smaller" decision, frames on both sides of the 256-sequence threshold for tables of their own.
  near_raw/tie/fs=4096/l1  three frames with one 9-byte match in 4096 random bytes each: every block's compressed form is EXACTLY as large as the block, which then goes
                           out raw (the mode decision is total < bsz; see the builder).
  def_outgrows/fs=F/lL     random bytes, per frame ONE planted 10-byte match in a block and 300 planted 40-byte matches (frames of 8192 bytes:
                           330 of 6 bytes, every 12 bytes) in the blocks behind it: the frame has its own tables (>= 256 sequences), the block
                           with the lone match is compressed by one to three bytes and pays for all three descriptions: Block_Size 20 to 51
                           bytes above what it regenerates.  At level 3 the matcher finds nothing in a frame's first 4096 positions, so
                           there the lone match sits in block 1 behind a raw block 0 -- which leaves no level-3 variant for frames of 8192.
  def_outgrows/single/...  the same question for a single-block frame (frame_size in 2049..4096, >= 256 sequences), where the window is the
                           block and Block_Size <= Block_Maximum_Size is at stake.  IT COULD NOT BE MADE TO OUTGROW: 256 sequences in at
                           most 4096 bytes are matches of >= 5 bytes that cost about 2.25 bytes each as a sequence (an 11-bit offset, three
                           short codes), so the block's Repeat_Mode form ends up hundreds of bytes below its input and the descriptions
                           (at most 108 bytes at accuracy log 6) do not make that up.  Searched with the twin at level 1 (level 3 finds
                           nothing in such a frame): frame sizes 2049, 2304, 2560, 2816, 3072, 3500, 4096; matches of 5, 6, 7 bytes every
                           7..14 bytes from anywhere earlier in the frame (the costliest offsets); 40 seeds each.  The defining block
                           never came closer than 741 bytes BELOW its regenerated size; that variant (3072 bytes, 277 matches of 5 bytes
                           every 10, 256 sequences in its tightest frame) is kept, with the fact def_grows_by<=0.
  many_tiny/64, /1         2500 frames of 64 bytes / of 1 byte: frame overhead is the dominant share of the output, and zk_k_scan64 carries
                           across its 1024-entry rounds.
  empty                    n = 0: one empty frame.

THE `ovf` BRANCH OF ZkeBitsL (a block's sequence bitstream that does not fit bsz bytes, nor bsz + 64 of scratch) IS NOT REACHED by any
input here.  Tried with the twin, which shares the matcher: a 2 MiB frame at levels 3 and 9 that begins with 64 KiB of random bytes and goes
on as text (so that the frame's tables give their short codes to text's sequences), in which one 32 KiB block 1.6 MiB in consists of
snippets of the random region -- 5..8, 6, 7..8, 8, 16 or 16..20 bytes long, 0..3 random bytes between them.  Of the ~4000 short snippets the
matcher took 400..700 (the dense far tables hold one candidate per hash slot and segment, want ZKE_DENSE_MIN = 6 bytes and a margin over
the ring's candidate); the 16-byte ones cost a sequence of ~4 bytes each.  The block's whole sequence section was 1.5 to 2.6 KiB of its
32 KiB in every variant; the block stayed compressed with raw literals.  For the stream to outgrow the block every sequence would have to
cost more than the bytes it regenerates, and the matcher's minimum lengths (4 at a repeat or 1 offset, 5 or 6 elsewhere, 16 for the sampled
far table and for anything in a prefix) against a worst case of 9 + 8 + 9 code bits and 21 offset bits leave no room for that in an input
we could construct.  The branch stays untested rather than reached through a back door into the kernel.
"""
import functools

import numpy as np

from helpers import enc_inputs as E
from oracle import zko

Entry = E.Entry
twin_frames = E.twin_frames
split_frames = E.split_frames


# ---------------------------------------------------------------------------------------------- what the frames say
def block_max(d):
    """the encoder's block size for a frame of d bytes without a prefix (zke_block_max / block_max_of in the twin): the window (>= 1 KiB) up
    to 4 KiB, then at least 16 blocks per frame, at most 32 KiB"""
    wlog = 10
    while (1 << wlog) < d and wlog < 17:
        wlog += 1
    t = 32768
    while t > 4096 and t * 16 > d:
        t >>= 1
    return min(t, 1 << wlog)


def window_size(f):
    """Window_Size a frame declares (RFC 8878 3.1.1.1.2; Frame_Content_Size for a Single_Segment frame)"""
    f = bytes(f)
    fhd = f[4]
    if (fhd >> 5) & 1:
        n = (1, 2, 4, 8)[fhd >> 6]
        v = int.from_bytes(f[5 + (0, 1, 2, 4)[fhd & 3]:][:n], "little")
        return v + 256 if n == 2 else v
    exp, mant = f[5] >> 3, f[5] & 7
    return (1 << (10 + exp)) + ((1 << (10 + exp)) >> 3) * mant


def frame_lengths(e):
    """decompressed bytes of each frame of the entry"""
    n = len(e.data)
    return [min(e.frame_size, n - o) for o in range(0, max(n, 1), e.frame_size)]


def defining_growth(f, d):
    """Block_Size minus regenerated bytes of the frame's defining block (None: the frame has none).  Blocks regenerate block_max(d) bytes
    each, the last one the rest."""
    blocks = E.walk_frame(f)
    bm = block_max(d)
    assert len(blocks) == max(1, -(-d // bm)), (len(blocks), d, bm)
    for k, b in enumerate(blocks):
        if b["type"] == "comp" and b["nseq"] and any((b["modes"] >> s) & 3 == 2 for s in (2, 4, 6)):
            return b["size"] - min(bm, d - k * bm)
    return None


def reached(frames, e):
    """the facts (module docstring, and enc_inputs.reached) that hold for these frames of entry e"""
    facts = set(E.reached(frames))
    ds = frame_lengths(e)
    assert len(ds) == len(frames)
    facts.add(f"frames={len(frames)}")
    walks = [E.walk_frame(f) for f in frames]
    if all(b["type"] == "raw" for w in walks for b in w):
        facts.add("all_raw")
    if all(len(f) == d + 6 + 3 * len(w) + (4 if f[4] & 4 else 0) for f, d, w in zip(frames, ds, walks)):
        facts.add("raw_exact")
    grows = [g for g in (defining_growth(f, d) for f, d in zip(frames, ds)) if g is not None]
    for g in grows:
        if g > 0:
            facts.add(f"def_outgrows=+{g}")
    if grows:
        facts.add(f"def_grows_by<={max(0, max(grows))}")
    return facts


# ---------------------------------------------------------------------------------------------- generators
def planted(n, seed, plants, reach=50000):
    """n random bytes; then, in the order given, for (count, length, lo, hi, floor) of `plants`: `count` copies of `length` bytes, each to a
    random place in [lo, hi) from a random place up to `reach` bytes in front of it, but not in front of `floor` (a frame's start); with a
    seventh value `stride` the places are lo, lo + stride, ... instead of random ones.  Copies
    are laid down front to back, so a source is final when it is read."""
    rng = np.random.default_rng(seed)
    buf = np.frombuffer(zko.gen_random(n, seed), np.uint8).copy()
    for count, length, lo, hi, floor, *stride in plants:
        hi = min(hi, n)
        lo = max(lo, floor + length)
        if hi - length <= lo:
            continue
        at = lo + stride[0] * np.arange(count) if stride else np.sort(rng.integers(lo, hi - length, count))
        for dst in at[at + length <= hi]:
            src = int(rng.integers(max(floor, dst - reach), dst - length + 1))
            buf[dst:dst + length] = buf[src:src + length].copy()
    return buf.tobytes()


_B = {}


def _e(name, data, frame_size, level, features):
    return Entry(name, bytes(data), frame_size, level, frozenset(features))


# ---- all_raw
ALL_RAW_SIZES = (1, 2, 63, 64, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537,
                 131071, 131072, 131073, 262145, 524287, 524288, 524289)


def _all_raw(fs, level):
    return _e(f"all_raw/fs={fs}", zko.gen_random(2 * fs + 1, 1000 + fs % 997), fs, level, {"all_raw", "raw_exact", "frames=3"})


for _i, _fs in enumerate(ALL_RAW_SIZES):
    _B[f"all_raw/fs={_fs}"] = functools.partial(_all_raw, _fs, 1 if _i % 2 == 0 else 3)


# ---- near_raw: (frame_size, level, planted matches per frame, their length) -> facts, frozen from the twin
NEAR_RAW = {
    (1025, 1, 1, 5): {"all_raw", "raw_exact"},
    (1025, 3, 2, 6): {"all_raw", "raw_exact"},
    (4096, 1, 2, 8): {"block=comp", "frame_nseq=2", "modes=all_00"},
    (4097, 1, 50, 6): {"block=comp", "block=raw", "frame_nseq=44", "modes=all_00"},
    (4097, 3, 260, 5): {"all_raw", "raw_exact"},                   # level 3 finds nothing in a frame's first 4096 positions
    (8193, 1, 260, 6): {"block=comp", "block=raw", "frame_nseq=204", "modes=all_00"},
    (8193, 3, 600, 8): {"block=comp", "block=raw", "frame_nseq=99", "modes=all_00"},
    (65536, 1, 260, 5): {"block=comp", "block=raw", "frame_nseq=100", "modes=all_00"},
    (65536, 3, 600, 6): {"block=raw", "def=0xA8@1", "frame_nseq=258", "def_outgrows=+4"},
    (65536, 1, 2000, 8): {"def=0xA8@0", "frame_nseq=1188", "def_grows_by<=0"},
    (131073, 3, 2000, 5): {"block=raw", "def=0xA8@0", "def=0xA8@1", "def_outgrows=+11"},
    (131073, 1, 600, 8): {"block=raw", "def=0xA8@0", "frame_nseq=343", "def_grows_by<=0"},
}


def _near_raw(fs, level, count, length, seed, facts):
    """two frames of fs bytes and one of a third of that, `count` planted matches in each"""
    n = 2 * fs + fs // 3
    return _e(f"near_raw/fs={fs}/l{level}/{count}x{length}", planted(n, seed, [(count, length, f * fs, (f + 1) * fs, f * fs) for f in range(3)]), fs, level,
              facts | {"frames=3"})


for (_fs, _l, _c, _n), _f in NEAR_RAW.items():
    _B[f"near_raw/fs={_fs}/l{_l}/{_c}x{_n}"] = functools.partial(_near_raw, _fs, _l, _c, _n, 7, _f)


# ---- near_raw/tie: the "compressed is smaller" decision at equality.  One 9-byte match in 4096 random bytes: 2 bytes of literals header, 4087
# literals, the sequence count, the modes byte and a 5-byte bitstream are 4096 bytes -- total == bsz, and the block goes out raw (total < bsz
# keeps it compressed).  An encoder that decides with <= writes a compressed block here: the facts fail, and so does the byte comparison.
def _tie(fs, level):
    n = 2 * fs + 4096
    plants = [(1, 9, b0 + 64, b0 + 4000, b0) for b0 in range(0, n, 4096)]
    return _e(f"near_raw/tie/fs={fs}/l{level}", planted(n, 3, plants, reach=3000), fs, level, {"all_raw", "raw_exact", "frames=3"})


for _fs, _l in ((4096, 1),):
    _B[f"near_raw/tie/fs={_fs}/l{_l}"] = functools.partial(_tie, _fs, _l)


# ---- def_outgrows
def _def_outgrows(fs, level, seed, facts, n=65536 * 2, first=10, count=300, length=40, stride=None, blk=0):
    """per frame of fs bytes: one `first`-byte match in block `blk`, `count` matches of `length` bytes behind that block"""
    nf = -(-n // fs)
    bm = block_max(fs)
    plants = []
    for f in range(nf):
        b0 = f * fs + blk * bm
        plants += [(1, first, b0 + 64, b0 + bm - 64, b0), (count, length, b0 + bm + 64, (f + 1) * fs, f * fs) + ((stride,) if stride else ())]
    return _e(f"def_outgrows/fs={fs}/l{level}", planted(n, seed, plants, reach=bm - 128), fs, level, facts)


def _single(fs, level, seed, facts, count, length, stride, reach=4096):
    """three single-block frames of fs bytes with `count` matches of `length` bytes every `stride` bytes from byte 256 on"""
    plants = [(count, length, f * fs + 256, (f + 1) * fs, f * fs, stride) for f in range(3)]
    return _e(f"def_outgrows/single/fs={fs}/l{level}", planted(3 * fs, seed, plants, reach=reach), fs, level, facts)


# A 10-byte match is the shortest that keeps its block compressed (by one to three bytes).  Level 3 finds no match in a frame's first 4096
# positions (its table is looked up before the step's own positions enter it), so there the lone match sits in block 1 and block 0 is raw;
# with frames of 8192 bytes that leaves no block for the other 255 sequences: no level-3 variant at that size.
_B["def_outgrows/fs=8192/l1"] = functools.partial(_def_outgrows, 8192, 1, 1, {"def=0xA8@0", "def_outgrows=+22", "frames=3"}, n=2 * 8192 + 4096, count=330,
                                                  length=6, stride=12)
_B["def_outgrows/fs=65536/l1"] = functools.partial(_def_outgrows, 65536, 1, 1, {"def=0xA8@0", "def_outgrows=+50", "frames=2"})
_B["def_outgrows/fs=65536/l3"] = functools.partial(_def_outgrows, 65536, 3, 1, {"def=0xA8@1", "def_outgrows=+49", "frames=2"}, blk=1)
_B["def_outgrows/fs=100000/l1"] = functools.partial(_def_outgrows, 100000, 1, 2, {"def=0xA8@0", "def_outgrows=+51", "frames=3"}, n=250000)
_B["def_outgrows/fs=100000/l3"] = functools.partial(_def_outgrows, 100000, 3, 1, {"def=0xA8@1", "def_outgrows=+50", "frames=3"}, n=250000, blk=1)
_B["def_outgrows/single/fs=3072/l1"] = functools.partial(_single, 3072, 1, 22, {"def=0xA8@0", "frame_nseq=256", "def_grows_by<=0", "frames=3"}, 277, 5, 10)
DEF_OUTGROWS_MAX = 51           # the largest N above


# ---- many_tiny, empty
def _many_tiny(fs):
    # text at 64 bytes per frame (at the Huffman gate: some frames come out compressed, most raw), random bytes at 1
    data = zko.gen_text(2500 * 64, 11) if fs == 64 else zko.gen_random(2500, 11)
    return _e(f"many_tiny/{fs}", data, fs, 1, {"frames=2500"} | ({"all_raw", "raw_exact"} if fs == 1 else set()))


_B["many_tiny/64"] = functools.partial(_many_tiny, 64)
_B["many_tiny/1"] = functools.partial(_many_tiny, 1)
_B["empty"] = lambda: _e("empty", b"", 4096, 1, {"frames=1", "all_raw"})

NAMES = list(_B)


@functools.lru_cache(maxsize=None)
def get(name):
    e = _B[name]()
    assert e.name == name
    return e

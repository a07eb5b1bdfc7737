"""Named, deterministic inputs that drive the encoder's FAR-HISTORY kernels (zeekstd_amd/csrc/zk_enc_far.h: zk_k_enc_dense_part,
zk_k_enc_dense_cand, zk_k_enc_ldm_build, zk_k_enc_ldm_build_frames, zk_k_enc_stage_hist) to their edges.  tests/helpers/enc_inputs.py drives
the entropy stage, enc_bound_inputs.py the output bound; this file is about what the matcher is handed from beyond its ring.

An entry is (name, data, frame_size, levels, slices, facts).  `slices` are the values of ZK_CHOICE_ENC_DENSE_SLICE_KIB's byte count the input
also runs under (0 = one slice).  `facts(refs, level)` asserts what makes the input a test of its edge; refs is enc_far_sim.reference(): per frame
the twin's (sampled table, (d, l, bk) per position, dense on) -- READ FROM THE TWIN (oracle/zstd_oracle_enc.c), never from the kernels, so an
input that misses its edge fails in tests/test_sim_enc_far.py before any kernel is asked.  Random filler keeps nearer copies out of the way.

  window_edge          four 200-byte blocks recur at distances ZKE_WINDOW - 1, ZKE_WINDOW, + 1, + 2: entries at exactly the two larger ones
  frame_start/zeros|bytes   X + filler + X: the second X's first four positions find frame positions 0..3 with catch-up 0..3 -- the bytes in
                       front of the second X are zeros (which agree with the zeros the kernel assumes in front of the frame: only the clip
                       `bk < e` keeps the catch-up from running past the frame's first byte) or random
  frame_tail/rR, /zeros/rR  a far copy that runs to the frame's last byte, frame sizes = R mod 4, two frames per call; /zeros: the copy's
                       source is followed by zero bytes, which "agree" with the zeros the kernel reads behind the frame.  Entries up to
                       frame size - 8 and none later
  seams/tT             (fact: the exact counts of entries served by `first` and by `last`, frozen from the twin per table size) one frame of 2 * ZKE_SEGMENT + T bytes; blocks that recur from the own segment only, from the segment before only
                       (one at distance ZKE_WINDOW across the seam: not found; one at ZKE_WINDOW + 1: found), from both in one slot, from
                       two segments back only (T = 4099: not found); the frame's last 8 bytes are a far copy (T = 8: the third segment's one entry)
  crowded/text         B + B, B = 106 496 bytes of gen_text.  The twin gives the fullest 8192-position chunk 7552 entries at level 3 and
                       7626 at level 9 (words recur inside B: a slot's first occurrence is often another word's, and six bytes do not agree) -- with B of
                       102 400, 106 496, 110 000 and 114 688 bytes, seeds 1..12 and both table sizes never more than 7674: text cannot fill a chunk
                       beyond 8000.  This input's fact is "> 7500"; the next one carries "> 8000"
  crowded/periodic     60 periods of 2048 random bytes: every position beyond the window has an entry; a chunk with more than 8000 entries,
                       the case of "a chunk's list lives where its entries will be: at most as many candidates as positions"
  crowded/records      20 000 records of a constant 5-byte head + 11 random bytes, two segments: one slot takes its minimum and maximum
                       from thousands of lanes
  runs                 far copies of a block that holds byte runs of 3, 4 and 5 and `aaaab`, copies placed at a tile, a chunk and a segment
                       start: no entry at a position whose four bytes are one byte, entries on both sides of it
  launch/KxF           K frames of F bytes (60 000: one segment each, 7 | 8 | 9 | 16 | 24 of them; 2 * ZKE_SEGMENT: 4 | 8): the candidate
                       kernel's XCD remap is live at 8, 16 and 24 workgroups; also cut into slices of one and of three frames
  launch/last=T        two frames of 60 000 bytes and a last one of T = 1 | 7 | 8 | 30 000 bytes, dense on for the call; T = 30 000 also in slices of
                       60 000 and 90 000 bytes: the engine cuts whole frames while they fit, [0] [1] [2] and [0] [1, 2], not a fixed count per slice
  ldm_frames/...       frames of 300 003 + 70 001, 300 003 + 57 281, 70 001 + 57 281 bytes (a call has one frame size and a last frame): each
                       frame's own zke_ldm_log inside the common stride
  PREFIXES             for zk_k_enc_ldm_build: lengths = 0..3 mod 4, ZKE_WINDOW + 1, and one whose last selected position is n - ZKE_LDM_MIN
"""
import collections
import functools

import numpy as np

from helpers import enc_far_sim as S
from oracle import zko

Entry = collections.namedtuple("Entry", "name data frame_size levels slices facts")
W, SEG = S.WINDOW, S.SEGMENT
_B = {}


def _rand(n, seed):
    return bytearray(zko.gen_random(n, seed))


def _entries(dlb, lo, hi):
    return int((dlb[lo:hi, 0] > 0).sum())


# ---- window_edge
def _window_edge():
    buf = _rand(61000, 101)
    dist = (W - 1, W, W + 1, W + 2)
    at = [1000 + 300 * i for i in range(4)]
    for a, d in zip(at, dist):
        buf[a + d:a + d + 200] = buf[a:a + 200]

    def facts(refs, level):
        dlb = refs[0][1]
        for a, d in zip(at, dist):
            got = dlb[a + d:a + d + 195]
            if d > W:
                assert int((got[:, 0] == d).sum()) >= 185 and int(((got[:, 0] != d) & (got[:, 0] != 0)).sum()) == 0, (d, got[:, 0].tolist())
            else:
                assert not got[:, 0].any(), d
    return Entry("window_edge", bytes(buf), 1 << 21, (3,), (0,), facts)


_B["window_edge"] = _window_edge


# ---- frame_start
def _frame_start(zeros):
    x = _rand(300, 111)
    filler = _rand(W + 120, 112)
    if zeros:
        filler[-8:] = bytes(8)
    else:
        filler[-4:] = b"\x01\x02\x03\x04"
    data = bytes(x + filler + x)
    p0 = len(x) + len(filler)

    def facts(refs, level):
        dlb = refs[0][1]
        assert dlb[p0:p0 + 4].tolist() == [[p0, 16, k] for k in range(4)], dlb[p0:p0 + 4].tolist()
    return Entry("frame_start/" + ("zeros" if zeros else "bytes"), data, 1 << 21, (3,), (0,), facts)


_B["frame_start/zeros"] = functools.partial(_frame_start, True)
_B["frame_start/bytes"] = functools.partial(_frame_start, False)


# ---- frame_tail
def _frame_tail(r, zeros):
    fs = 58000 + r
    frames = []
    for f in range(2):
        buf = _rand(fs, 120 + 4 * f + r)
        if zeros:
            buf[600:616] = bytes(16)
        buf[fs - 100:fs] = buf[500:600]
        frames.append(buf)

    def facts(refs, level):
        for ref in refs:
            dlb = ref[1]
            assert dlb[fs - 8].tolist() == [fs - 600, 8, 4] and not dlb[fs - 7:, 0].any(), dlb[fs - 10:].tolist()
            assert dlb[fs - 20].tolist() == [fs - 600, 16, 4]
    return Entry(f"frame_tail/{'zeros/' if zeros else ''}r{r}", bytes(frames[0] + frames[1]), fs, (3,), (0,), facts)


for _r in range(4):
    _B[f"frame_tail/r{_r}"] = functools.partial(_frame_tail, _r, False)
    _B[f"frame_tail/zeros/r{_r}"] = functools.partial(_frame_tail, _r, True)


# ---- seams
def _seams(t, levels, counts):
    fs = 2 * SEG + t
    buf = _rand(fs, 130 + t % 97)
    cp = lambda dst, src, n=200: buf.__setitem__(slice(dst, dst + n), buf[src:src + n])
    a_src, a_dst = SEG + 1000, SEG + 1000 + W + 500             # A: from the own segment only (first)
    cp(a_dst, a_src)
    b1_src = SEG - 700; b1_dst = b1_src + W                        # B1: across the seam at exactly ZKE_WINDOW: not found
    cp(b1_dst, b1_src)
    b2_src = SEG - 300; b2_dst = b2_src + W + 1                  # B2: ... at ZKE_WINDOW + 1: found (last)
    cp(b2_dst, b2_src)
    c_src, c_mid, c_dst = SEG - W - 400, SEG + 100, SEG + 100 + W + 300   # C: both tables hold the slot: c_mid is served by last, c_dst by first
    cp(c_mid, c_src); cp(c_dst, c_src)
    f_src = 2 * SEG - W - 8                                       # F: the frame's last 8 bytes, from the segment before
    buf[fs - 8:fs] = buf[f_src:f_src + 8]
    d_src, d_dst, e_src, e_dst = 2000, 2 * SEG + 100, 2 * SEG - W - 400, 2 * SEG + 2000
    if t == 4099:
        cp(d_dst, d_src)                                         # D: two segments back only: not found
        cp(e_dst, e_src)                                         # E: the third segment finds the second

    def facts(refs, level):
        dlb = refs[0][1]
        first, last = S.served_by(dlb)
        assert (first, last) == counts[18 if level >= 9 else 17], (first, last)      # (frozen from the twin: entries out of the own segment, out of the one before)
        # (a source in the segment before is the slot's LAST position there: the 57 000+ positions behind it take the slot from about a third of its bytes)
        full = lambda at, d, least=185: int((dlb[at:at + 195, 0] == d).sum()) >= least
        assert full(a_dst, a_dst - a_src) and full(c_dst, c_dst - c_mid) and first >= 360, first
        assert full(b2_dst, W + 1) and full(c_mid, c_mid - c_src, 100), last
        assert not dlb[b1_dst:b1_dst + 195, 0].any()
        third = _entries(dlb, 2 * SEG, fs)
        if t < 8:
            assert third == 0 and last >= 280
        elif t == 8:
            assert third == 1 and dlb[2 * SEG, :2].tolist() == [2 * SEG - f_src, 8]
        else:
            assert not dlb[d_dst:d_dst + 195, 0].any() and full(e_dst, e_dst - e_src, 100) and last >= 380
    return Entry(f"seams/t{t}", bytes(buf), 1 << 21, levels, (0,), facts)


_B["seams/t5"] = functools.partial(_seams, 5, (3,), {17: (389, 322)})
_B["seams/t7"] = functools.partial(_seams, 7, (3,), {17: (390, 326)})
_B["seams/t8"] = functools.partial(_seams, 8, (3,), {17: (388, 329)})
_B["seams/t4099"] = functools.partial(_seams, 4099, (0, 3, 6, 9, 19), {17: (387, 451), 18: (389, 518)})


# ---- crowded
def _fullest(dlb):
    return max(_entries(dlb, c, c + 8192) for c in range(0, len(dlb), 8192))


def _crowded_text():
    b = zko.gen_text(13 * 8192, 5)

    def facts(refs, level):
        assert _fullest(refs[0][1]) > 7500, _fullest(refs[0][1])
    return Entry("crowded/text", b + b, 1 << 21, (0, 3, 6, 9, 19), (0,), facts)


def _crowded_periodic():
    def facts(refs, level):
        assert _fullest(refs[0][1]) > 8000, _fullest(refs[0][1])
    return Entry("crowded/periodic", bytes(_rand(2048, 141)) * 60, 1 << 21, (0, 3, 6, 9, 19), (0,), facts)


def _crowded_records():
    rnd = zko.gen_random(11 * 20000, 142)
    data = b"".join(b"HEAD:" + rnd[11 * i:11 * i + 11] for i in range(20000))

    def facts(refs, level):
        h = S.hash5(data, 17)
        assert int((h == h[0]).sum()) >= 19999                  # one slot, every record's first position
    return Entry("crowded/records", data, 1 << 21, (3, 9), (0,), facts)


_B["crowded/text"] = _crowded_text
_B["crowded/periodic"] = _crowded_periodic
_B["crowded/records"] = _crowded_records


# ---- runs
def _runs():
    r = _rand(400, 151)
    blk = bytearray(b"aaaab") + r[:20] + b"xxx" + r[20:27] + b"yyyy" + r[27:36] + b"zzzzz" + r[36:41] + b"aaaab" + r[41:51] + b"aaaabaaaab" + r[51:90] + \
        b"\0\0\0\0" + r[90:130] + b"qqqqqq" + r[130:160]
    n = len(blk)
    buf = _rand(SEG + 70000, 152)
    src = 1024
    # a chunk start, a tile start, runs across a chunk start, the last content of the first segment, the second segment's start, runs across a chunk start there
    dsts = [8192 * 9, 4096 * 19 + 256, 8192 * 20 - 7, SEG - W - 600, SEG, SEG + 8192 * 8 - 3]
    buf[src:src + n] = blk
    for d in dsts:
        buf[d:d + n] = blk
    buf[dsts[3] + n:SEG] = bytes(SEG - dsts[3] - n)         # zeros: byte runs enter no table, so the copy in front of them is every slot's last position
    run = S.is_run(bytes(buf))

    def facts(refs, level):
        dlb = refs[0][1]
        assert not dlb[:len(run), 0][run].any()
        for d in dsts:
            rr = np.nonzero(run[d:d + n - 16])[0]
            assert len(rr) >= 9, len(rr)
            assert not dlb[d, 0]                                    # the copy begins with `aaaa`
            for q in rr[rr > 0]:                                    # entries on both sides of every run
                lo, hi = q, q
                while run[d + lo]:
                    lo -= 1
                while run[d + hi]:
                    hi += 1
                assert dlb[d + lo, 0] and dlb[d + hi, 0], (d, int(q))
    return Entry("runs", bytes(buf), 1 << 21, (3, 9), (0,), facts)


_B["runs"] = _runs


# ---- launch shapes
def _launch(k, fs, last=0):
    n = k * fs + last
    buf = _rand(n, 160 + k + last % 89)
    for f in range(k):
        o = f * fs
        for g in range(0, fs - 59500 + 1, SEG):
            buf[o + g + 57500:o + g + 59500] = buf[o + g:o + g + 2000]      # a far copy in every segment

    def facts(refs, level):
        assert len(refs) == k + (1 if last else 0)
        for ref in refs[:k]:
            assert ref[2] and _entries(ref[1], 0, fs) >= 1900 * (fs // SEG if fs >= SEG else 1)
        if last:
            assert refs[k][1] is None if last <= W else refs[k][2]
    name = f"launch/last={last}" if last else f"launch/{k}x{fs}"
    # (last=30000 under slices of 60 000 and 90 000 bytes: frames [0] [1] [2] and [0] [1, 2] -- the short last frame joins the slice before it)
    slices = (0, fs, 3 * fs) if not last else (0, 60000, 90000) if last == 30000 else (0,)
    return Entry(name, bytes(buf), fs, (3,), slices, facts)


for _k in (7, 8, 9, 16, 24):
    _B[f"launch/{_k}x60000"] = functools.partial(_launch, _k, 60000)
for _k in (4, 8):
    _B[f"launch/{_k}x{2 * SEG}"] = functools.partial(_launch, _k, 2 * SEG)
for _t in (1, 7, 8, 30000):
    _B[f"launch/last={_t}"] = functools.partial(_launch, 2, 60000, _t)

NAMES = list(_B)
# (name, level, slice bytes) of what tests/sim/enc_far_san.cpp runs under the sanitizers
SAN_SHAPES = [("frame_start/zeros", 3, 0), ("frame_start/bytes", 3, 0)] + [(f"frame_tail/r{r}", 3, 0) for r in range(4)] + \
    [("frame_tail/zeros/r1", 3, 0), ("seams/t5", 3, 0), ("crowded/text", 3, 0), ("crowded/periodic", 9, 0), ("launch/16x60000", 3, 3 * 60000)] + \
    [(f"launch/last={t}", 3, 0) for t in (1, 7, 8)] + \
    [("launch/last=30000", 3, 90000)]   # (a source that ends 1, 7 and 8 bytes into its last frame: nothing is read behind it; a slice of a frame and a half)


@functools.lru_cache(maxsize=None)
def get(name):
    e = _B[name]()
    assert e.name == name
    return e


# ---- sampled tables
def ldm_frames_inputs():
    """(name, data, frame_size): two frames with a zke_ldm_log of their own each"""
    text = zko.gen_text(300003 + 70001, 171)
    return [("ldm_frames/300003+70001", text, 300003), ("ldm_frames/300003+57281", text[:300003 + 57281], 300003),
            ("ldm_frames/70001+57281", text[200000:200000 + 70001 + 57281], 70001)]


@functools.lru_cache(maxsize=None)
def prefixes():
    """{name: prefix bytes} for the prefix table; `last_selected`: the longest prefix of the text below 70 000 bytes whose position n - ZKE_LDM_MIN
    is in the twin's table"""
    text = zko.gen_text(70016, 181)
    out = {f"mod4={r}": text[:66000 + r] for r in range(4)}
    out["window+1"] = text[:W + 1]
    for n in range(70000, 69000, -1):
        if (zko.enc_ldm_prefix_debug(text[:n]) == n - S.LDM_MIN).any():
            out["last_selected"] = text[:n]
            break
    return out

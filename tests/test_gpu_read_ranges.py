"""zk_read_ranges_dev / zk_read_ranges / Engine.read_ranges: batched byte-range reads of an archive, checked against slices of the
archive's input.  The destination is poisoned before every call and compared as a whole: the ranges' bytes, and the poison everywhere
else -- between padded destinations and behind the last one."""
import numpy as np
import pytest

from conftest import GOLDENS
from oracle import zko

pytestmark = pytest.mark.gpu

POISON = 0xA5
TAIL = 257
OUT_OF_RANGE = -1001
DST_TOO_SMALL = -70


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev_u64(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64)).to(dev)


class Arc:
    """An archive in HBM + its input on the host."""

    def __init__(self, name, comp, c, d, data):
        torch, dev = _torch()
        self.name = name
        self.comp = bytes(comp)
        self.c, self.d = np.asarray(c, np.uint64), np.asarray(d, np.uint64)
        self.n = len(self.c) - 1
        self.data = np.frombuffer(bytes(data), np.uint8)
        self.total = int(self.d[-1])
        assert self.total == len(self.data)
        self.d_comp = torch.from_numpy(np.frombuffer(self.comp + b"\0" * 64, np.uint8).copy()).to(dev)
        self.d_c, self.d_d = _dev_u64(self.c), _dev_u64(self.d)


def golden_arc(g):
    c, d = g.offsets()
    return Arc(g.name, g.comp, c, d, g.input())


_MADE = {}


def made_arc(engine, kind):
    """archives made here: 256 frames of 64 KiB and 8 frames of 2 MiB of the generator's text, checksums on; and one written by libzstd"""
    if kind not in _MADE:
        if kind == "t64k":
            data, fs = zko.gen_chunks(256 * 65536 - 1234, 0x7E57), 65536
        elif kind == "t2m":
            data, fs = zko.gen_chunks(8 * 0x200000 - 77, 0x7E58), 0x200000
        elif kind == "ref_l3":
            from oracle import libzstd_ref as Z
            assert Z.load("system") is not None, "the reference-made archive needs the box's libzstd"
            data = zko.gen_chunks(40 * 65536 + 999, 0x7E59)
            comp, frames = Z.encode_seekable_frames(data, 65536, 3, True)
        if kind != "ref_l3":
            comp, frames = engine.encode_frames(data, fs, 1, True)
        c = np.zeros(len(frames) + 1, np.uint64); c[1:] = np.cumsum([f[0] for f in frames])
        d = np.zeros(len(frames) + 1, np.uint64); d[1:] = np.cumsum([f[1] for f in frames])
        _MADE[kind] = Arc(kind, comp, c, d, data)
    return _MADE[kind]


def make_ranges(arc, seed, nrand=300):
    rng = np.random.default_rng(seed)
    total = arc.total
    r = []
    for k in range(nrand):
        off = int(rng.integers(0, total + 1))
        top = (300, 5000, 70000, 400000)[k % 4]
        r.append((off, min(int(rng.integers(0, top + 1)), total - off)))
    r.append((0, total))                                                    # the whole archive as one range
    if arc.n <= 64:                                                         # single bytes on both sides of every frame boundary, and across it
        for b in arc.d.tolist():
            if b > 0:
                r.append((b - 1, 1))
            if b < total:
                r.append((b, 1))
            if 0 < b < total:
                r.append((b - 1, 2))
    r += [(0, 0), (total, 0), (total // 2, 0)]                              # zero-length
    r += [r[3], r[3], r[7]]                                                 # repeats
    x = total // 3
    r += [(x, min(1000, total - x)), (min(x + 500, total), min(1000, total - min(x + 500, total)))]     # overlapping
    order = rng.permutation(len(r))
    return [r[i] for i in order]


def destinations(ranges, mode, seed=1):
    """packed: None; padded: every destination on a 64-byte multiple with odd gaps in front; ragged: odd starts"""
    if mode == "packed":
        offs, at = [], 0
        for _, n in ranges:
            offs.append(at); at += n
        return None, offs, at
    rng = np.random.default_rng(seed)
    offs, at = [], 0
    for _, n in ranges:
        at += int(rng.integers(0, 40)) * 2 + 1                               # an odd gap
        if mode == "padded":
            at = (at + 63) & ~63
        offs.append(at); at += n
    return offs, offs, at


def read(engine, arc, ranges, mode="packed", verify=True, dst_cap=None, dst_offs=None, end=None):
    """one zk_read_ranges_dev call over a poisoned destination -> (rc, status array, the destination as a numpy array, offsets used).
    dst_offs / end: destinations of the caller's own making and where the last one ends (instead of `mode`)"""
    torch, dev = _torch()
    if end is None:
        given, offs, end = destinations(ranges, mode)
    else:
        given, offs = dst_offs, dst_offs
    cap = end if dst_cap is None else dst_cap
    d_dst = torch.full((max(cap, end) + TAIL,), POISON, dtype=torch.uint8, device=dev)
    d_st = torch.full((max(len(ranges), 1),), -12345, dtype=torch.int32, device=dev)
    d_o = _dev_u64([o for o, _ in ranges] or [0])
    d_l = _dev_u64([n for _, n in ranges] or [0])
    d_do = _dev_u64(given) if given is not None else None
    rc = engine.read_ranges_dev(arc.d_comp, len(arc.comp), arc.d_c, arc.d_d, arc.n, d_o, d_l, d_do, len(ranges), d_dst, cap, verify, d_st)
    torch.cuda.synchronize()
    return rc, d_st.cpu().numpy()[:len(ranges)], d_dst.cpu().numpy(), offs


def expected(arc, ranges, offs, size, skip=()):
    want = np.full(size, POISON, np.uint8)
    for i, ((o, n), at) in enumerate(zip(ranges, offs)):
        if i not in skip:
            want[at:at + n] = arc.data[o:o + n]
    return want


def check(engine, arc, ranges, mode, **kw):
    rc, st, got, offs = read(engine, arc, ranges, mode, **kw)
    assert rc == 0 and not st.any(), (arc.name, mode, rc, np.nonzero(st)[0][:8])
    want = expected(arc, ranges, offs, len(got))
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        i = max([k for k, at in enumerate(offs) if at <= bad], key=lambda k: offs[k], default=None)
        pytest.fail(f"{arc.name}, {mode}: first wrong byte at {bad} of the destination (range {i}: {ranges[i] if i is not None else None} at {offs[i] if i is not None else None})")
    return got


NONEMPTY = [g for g in GOLDENS if any(f[1] for f in g.frames)]


# ---- 1. every golden archive
@pytest.mark.parametrize("g", NONEMPTY, ids=[g.name for g in NONEMPTY])
@pytest.mark.parametrize("mode", ["packed", "padded", "ragged"])
def test_ranges_of_every_golden(engine, g, mode):
    arc = golden_arc(g)
    check(engine, arc, make_ranges(arc, 0xA11 + len(g.name)), mode)


@pytest.mark.parametrize("mode", ["packed", "padded"])
def test_ranges_of_made_archives(engine, mode):
    """many frames, long copies (the chunked path of the copy kernel) and empty frames in the table"""
    for kind in ("t64k", "t2m"):
        arc = made_arc(engine, kind)
        ranges = make_ranges(arc, 0xB22)
        ranges += [(arc.total - 3000000, 3000000), (65536 * 3 + 5, 65536 * 9 + 1)]
        check(engine, arc, ranges, mode)
    # the same 64 KiB archive with empty frames in front, in the middle and at the end of its table
    a = made_arc(engine, "t64k")
    empty = b"\x28\xb5\x2f\xfd\x00\x58\x01\x00\x00"            # an empty zstd frame: magic, descriptor, window, one empty raw last block
    pieces, sizes = [], []
    for f in range(a.n):
        if f in (0, 100, 101):
            pieces += [empty, empty]; sizes += [(len(empty), 0)] * 2
        pieces.append(a.comp[int(a.c[f]):int(a.c[f + 1])]); sizes.append((int(a.c[f + 1] - a.c[f]), int(a.d[f + 1] - a.d[f])))
    pieces += [empty, empty]; sizes += [(len(empty), 0)] * 2
    c = np.zeros(len(sizes) + 1, np.uint64); c[1:] = np.cumsum([s[0] for s in sizes])
    d = np.zeros(len(sizes) + 1, np.uint64); d[1:] = np.cumsum([s[1] for s in sizes])
    arc = Arc("t64k_with_empties", b"".join(pieces), c, d, a.data.tobytes())
    ranges = make_ranges(arc, 0xB23, 200) + [(int(b) - 1, 2) for b in d[1:-1].tolist() if 0 < b < arc.total]
    check(engine, arc, ranges, mode)
    assert engine.ranges_frames_decoded() == a.n                # the whole archive is among the ranges: every non-empty frame once, no empty one


# ---- 2. host pointers
@pytest.mark.parametrize("name", ["text_l1_64k", "text_100B_frames", "mixed", "oneshot_text_l3", "one_byte"])
def test_host_pointer_form(engine, name):
    import zeekstd_amd as zk
    g = next(x for x in GOLDENS if x.name == name)
    arc = golden_arc(g)
    ranges = make_ranges(arc, 0xC33, 120)
    offs = np.array([o for o, _ in ranges], np.uint64)
    lens = np.array([n for _, n in ranges], np.uint64)
    comp = g.comp + b"\0" * 8
    # Engine.read_ranges: a list of bytes, and the packed form
    outs, st = engine.read_ranges(comp, arc.c, arc.d, offs, lens)
    assert not st.any()
    for (o, n), b in zip(ranges, outs):
        assert b == arc.data[o:o + n].tobytes(), (name, o, n)
    blob, pk, st = engine.read_ranges(comp, arc.c, arc.d, offs, lens, packed=True)
    assert not st.any() and len(blob) == int(lens.sum())
    for i, (o, n) in enumerate(ranges):
        assert blob[int(pk[i]):int(pk[i + 1])] == arc.data[o:o + n].tobytes()
    # zk_read_ranges with destinations of the caller: nothing but the ranges is written; a bad range among them
    bad = [(arc.total - 1, 2), (arc.total + 1, 0)] if arc.total > 1 else [(arc.total + 1, 0)]
    ranges2 = ranges[:40] + bad + ranges[40:]
    _, dst_offs, end = destinations(ranges2, "padded", 5)
    dst = np.full(end + TAIL, POISON, np.uint8)
    st = np.full(len(ranges2), -12345, np.int32)
    src = np.frombuffer(comp, np.uint8)
    o2 = np.array([o for o, _ in ranges2], np.uint64); l2 = np.array([n for _, n in ranges2], np.uint64); do2 = np.array(dst_offs, np.uint64)
    rc = zk.lib.zk_read_ranges(engine._h, src.ctypes.data, len(g.comp), arc.c.ctypes.data, arc.d.ctypes.data, arc.n, o2.ctypes.data, l2.ctypes.data,
                               do2.ctypes.data, len(ranges2), dst.ctypes.data, end, 1, st.ctypes.data)
    skip = set(range(40, 40 + len(bad)))
    assert rc == OUT_OF_RANGE
    assert all(st[i] == (OUT_OF_RANGE if i in skip else 0) for i in range(len(ranges2))), st
    assert np.array_equal(dst, expected(arc, ranges2, dst_offs, len(dst), skip))


# ---- 3. a frame is decoded once
def test_each_touched_frame_is_decoded_once(engine):
    torch, dev = _torch()
    arc = made_arc(engine, "t2m")
    frames = [1, 4, 5]
    rng = np.random.default_rng(0xD44)
    ranges = []
    for k in range(500):
        f = frames[k % 3]
        lo, hi = int(arc.d[f]), int(arc.d[f + 1])
        off = int(rng.integers(lo, hi))
        ranges.append((off, int(rng.integers(1, min(8192, hi - off) + 1))))
    ids = torch.tensor(frames, dtype=torch.int32, device=dev)
    sizes = [int(arc.d[f + 1] - arc.d[f]) for f in frames]
    oo = np.zeros(4, np.uint64); oo[1:] = np.cumsum(sizes)
    d_oo = _dev_u64(oo)
    d_out = torch.empty(int(oo[-1]) + 64, dtype=torch.uint8, device=dev)
    stage = ("zk_k_huf", "zk_k_fse", "zk_k_exec", "zk_k_xxh64")
    engine.set_profiling(True)
    try:
        check(engine, arc, ranges, "packed")                                   # warm: scratch allocations
        assert engine.decode_frame_list_dev(arc.d_comp, len(arc.comp), arc.d_c, arc.d_d, ids, d_oo, 3, d_out, int(oo[-1]), True) == 0
        t_list, t_rng = [], []
        for _ in range(5):
            assert engine.decode_frame_list_dev(arc.d_comp, len(arc.comp), arc.d_c, arc.d_d, ids, d_oo, 3, d_out, int(oo[-1]), True) == 0
            kt = engine.kernel_times()
            t_list.append(sum(kt.get(k, 0.0) for k in stage))
            check(engine, arc, ranges, "packed")
            assert engine.ranges_frames_decoded() == 3
            kt = engine.kernel_times()
            assert kt.get("zk_k_range_gather", 0) > 0 and kt.get("zk_k_range_plan", 0) > 0, kt
            t_rng.append(sum(kt.get(k, 0.0) for k in stage))
    finally:
        engine.set_profiling(False)
    a, b = float(np.median(t_list)), float(np.median(t_rng))
    print(f"\ndecode-stage kernels, 3 frames of 2 MiB: frame list {a:.3f} ms, 500 ranges in them {b:.3f} ms")
    # the same three frames through the same kernels: the same time but for noise.  Decoding per range would be 500 / 3 times the work;
    # a factor of three either way (and 0.1 ms for the timers' granularity) tells the two apart with a wide margin.
    assert b <= 3 * a + 0.1 and a <= 3 * b + 0.1, (a, b)


# ---- 4. passes
def test_passes_over_the_scratch(engine):
    arc = made_arc(engine, "t64k")
    ranges = make_ranges(arc, 0xE55, 400)
    touched = set()
    for o, n in ranges:
        if n:
            touched.update(range(int(np.searchsorted(arc.d, o, "right")) - 1, int(np.searchsorted(arc.d, o + n - 1, "right"))))
    assert len(touched) >= 200
    try:
        base = check(engine, arc, ranges, "padded")
        assert engine.ranges_frames_decoded() == len(touched)
        engine.set_kernel_choice(range_pass_mib=1)                              # sixteen frames per pass
        one = check(engine, arc, ranges, "padded")
        assert engine.ranges_frames_decoded() == len(touched)
        assert np.array_equal(base, one)
        big = made_arc(engine, "t2m")                                           # a pass below one frame: a frame per pass
        r2 = make_ranges(big, 0xE56, 200)
        check(engine, big, r2, "packed")
        check(engine, big, r2, "padded")
        assert engine.ranges_frames_decoded() == big.n
    finally:
        engine.set_kernel_choice(reset=0)
    check(engine, arc, ranges[:50], "packed")


# ---- 5. bad ranges
def test_bad_ranges_get_their_status_and_neighbours_are_served(engine):
    arc = made_arc(engine, "t64k")
    total = arc.total
    U64 = (1 << 64) - 1
    good = make_ranges(arc, 0xF66, 60)
    bad_src = [(total, 1), (total + 1, 0), (total - 10, 11), (5, U64), (U64, 2), (U64 - 1, 1), (1 << 63, 1 << 63)]
    ranges = good[:20] + bad_src[:3] + good[20:40] + bad_src[3:] + good[40:]
    bad_at = set(range(20, 23)) | set(range(43, 43 + len(bad_src) - 3))
    for mode in ("packed", "padded"):
        given, offs, end = destinations([(o, 0 if i in bad_at else n) for i, (o, n) in enumerate(ranges)], mode)
        rc, st, got, _ = read(engine, arc, ranges, dst_offs=given, dst_cap=end, end=end)
        assert rc == OUT_OF_RANGE, rc                                               # the first failing range in list order
        assert all(st[i] == (OUT_OF_RANGE if i in bad_at else 0) for i in range(len(ranges))), (mode, st)
        assert np.array_equal(got, expected(arc, ranges, offs, len(got), bad_at)), mode
    # destinations past dst_cap: explicit offsets, a capacity that cuts the last two destinations off and one offset that overflows
    given, offs, end = destinations(good, "padded")
    cap = offs[-2] + max(good[-2][1] - 1, 0)
    cut = {i for i, ((_, n), at) in enumerate(zip(good, offs)) if at + n > cap}
    assert cut and len(cut) < len(good)
    rc, st, got, _ = read(engine, arc, good, dst_offs=given, dst_cap=cap, end=end)
    assert rc == DST_TOO_SMALL
    assert all(st[i] == (DST_TOO_SMALL if i in cut else 0) for i in range(len(good))), st
    assert np.array_equal(got, expected(arc, good, offs, len(got), cut))
    # packed: the capacity ends inside a range; everything behind it is cut as well, zero-length ranges at the very end of the capacity are not
    _, poffs, pend = destinations(good, "packed")
    k = max(i for i, (_, n) in enumerate(good) if n > 1 and poffs[i] > 0)
    cap = poffs[k] + good[k][1] - 1
    rc, st, got, _ = read(engine, arc, good, dst_cap=cap)
    cut = {i for i, ((_, n), at) in enumerate(zip(good, poffs)) if at + n > cap}
    assert k in cut and rc == DST_TOO_SMALL
    assert all(st[i] == (DST_TOO_SMALL if i in cut else 0) for i in range(len(good))), st
    assert np.array_equal(got[:cap + TAIL], expected(arc, good, poffs, len(got), cut)[:cap + TAIL])


# ---- 6. a damaged frame
def test_damaged_frames_fail_their_ranges_only(engine):
    torch, dev = _torch()
    a = made_arc(engine, "t64k")
    comp = bytearray(a.comp)
    fp, fc = 10, 20                                                              # a bit in frame 10's payload, one in frame 20's checksum
    comp[(int(a.c[fp]) + int(a.c[fp + 1])) // 2] ^= 0x10
    comp[int(a.c[fc + 1]) - 1] ^= 0x01
    arc = Arc("t64k_damaged", bytes(comp), a.c, a.d, a.data.tobytes())
    # what the frames themselves say
    d_out = torch.empty(arc.total + 64, dtype=torch.uint8, device=dev)
    d_fs = torch.zeros(arc.n, dtype=torch.int32, device=dev)
    fst = {}
    for verify in (True, False):
        engine.decode_frames_dev(arc.d_comp, len(arc.comp), arc.d_c, arc.d_d, 0, arc.n, d_out, arc.total, verify, d_fs)
        fst[verify] = d_fs.cpu().numpy().copy()
    assert fst[True][fp] != 0 and fst[True][fc] == 22 and np.count_nonzero(fst[True]) == 2
    assert fst[False][fc] == 0
    rng = np.random.default_rng(0x1177)
    ranges = []
    for k in range(300):
        off = int(rng.integers(0, arc.total))
        ranges.append((off, min(int(rng.integers(0, (300, 5000, 200000)[k % 3])), arc.total - off)))
    ranges += [(int(a.d[fp]) - 1, 1), (int(a.d[fp]), 1), (int(a.d[fp + 1]) - 1, 2), (int(a.d[fc]) - 3, 4), (int(a.d[fc + 1]), 9), (int(a.d[8]), 65536 * 14)]
    for verify in (True, False):
        want_st = []
        for o, n in ranges:
            code = 0
            if n:
                for f in range(int(np.searchsorted(arc.d, o, "right")) - 1, int(np.searchsorted(arc.d, o + n - 1, "right"))):
                    if fst[verify][f]:
                        code = -int(fst[verify][f]); break
            want_st.append(code)
        assert sum(1 for s in want_st if not s) >= 100
        if verify:
            assert sum(1 for s in want_st if -s == fst[True][fp]) >= 3 and sum(1 for s in want_st if s == -22) >= 3
        rc, st, got, offs = read(engine, arc, ranges, "padded", verify=verify)
        assert st.tolist() == want_st, (verify, [(i, st[i], want_st[i]) for i in range(len(ranges)) if st[i] != want_st[i]][:8])
        assert rc == next((s for s in want_st if s), 0), (verify, rc)
        failed = {i for i, s in enumerate(want_st) if s}
        # (the bytes of a failed range are unspecified within its own destination: they are taken from the result before the comparison)
        want = expected(arc, ranges, offs, len(got), failed)
        for i in failed:
            want[offs[i]:offs[i] + ranges[i][1]] = got[offs[i]:offs[i] + ranges[i][1]]
        if not verify and fst[False][fp] == 0:
            pass                                                                # the payload damage shows in the checksum only: its ranges "succeed" with whatever the frame decodes to
        else:
            assert np.array_equal(got, want), verify
        if not verify:                                                          # the frame whose checksum field alone is damaged delivers its bytes
            for i, (o, n) in enumerate(ranges):
                if want_st[i] == 0 and n and int(np.searchsorted(arc.d, o, "right")) - 1 <= fc < int(np.searchsorted(arc.d, o + n - 1, "right")) \
                        and not (o < int(a.d[fp + 1]) and o + n > int(a.d[fp])):
                    assert np.array_equal(got[offs[i]:offs[i] + n], arc.data[o:o + n]), i


# ---- 7. past 2^32
BIG_FRAME = 0x200000
BIG_NF = 2304
BIG_N = BIG_NF * BIG_FRAME
TWO32 = 1 << 32


def _big_headers():
    return np.frombuffer(b"".join(f"frame {f:08d} of the archive past four gibibytes".ljust(64, ".").encode() for f in range(BIG_NF)), np.uint8).reshape(BIG_NF, 64)


def _big_fill():
    return ((np.arange(BIG_NF) * 37 + 11) & 0xFF).astype(np.uint8)


def _big_expected(hdr, fill, off, n):
    pos = np.arange(off, off + n, dtype=np.int64)
    f, r = pos // BIG_FRAME, pos % BIG_FRAME
    return np.where(r < 64, hdr[f, np.minimum(r, 63)], fill[f])


def test_ranges_past_4gib(engine):
    import zeekstd_amd as zk
    torch, dev = _torch()
    assert BIG_N == 9 * (1 << 29) and BIG_N > TWO32
    hdr, fill = _big_headers(), _big_fill()
    d_src = torch.empty(BIG_N, dtype=torch.uint8, device=dev)
    v = d_src.view(BIG_NF, BIG_FRAME)
    v[:] = torch.from_numpy(fill).to(dev)[:, None]
    v[:, :64] = torch.from_numpy(hdr.copy()).to(dev)
    cap = int(zk.lib.zk_compress_bound(BIG_N, BIG_FRAME))
    d_comp = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    d_cs = torch.zeros(BIG_NF, dtype=torch.int32, device=dev)
    d_ds = torch.zeros(BIG_NF, dtype=torch.int32, device=dev)
    nf, csize = engine.encode_frames_dev(d_src, BIG_N, BIG_FRAME, 1, True, d_comp, cap, d_cs, d_ds)
    torch.cuda.synchronize()
    assert nf == BIG_NF
    del d_src, v
    comp = d_comp[:csize + 64].clone()
    comp[csize:] = 0
    del d_comp
    torch.cuda.empty_cache()
    c = np.zeros(BIG_NF + 1, np.uint64); c[1:] = np.cumsum(d_cs.cpu().numpy().astype(np.uint64))
    d = np.zeros(BIG_NF + 1, np.uint64); d[1:] = np.cumsum(d_ds.cpu().numpy().astype(np.uint64))
    assert int(d[-1]) == BIG_N and int(c[-1]) == csize
    d_c, d_d = _dev_u64(c), _dev_u64(d)
    rng = np.random.default_rng(0x2032)
    ranges = []
    for k in range(2000):
        n = int(rng.integers(1, 8193))
        kind = k % 4
        if kind == 0 and k % 8 == 0:                                            # across 2^32: the first byte below it, the last one beyond
            off = TWO32 - int(rng.integers(1, n)) if n > 1 else TWO32 - 1
        elif kind == 0:                                                         # around 2^32
            off = TWO32 + int(rng.integers(-3 * BIG_FRAME, 3 * BIG_FRAME))
        elif kind == 1:                                                         # at a frame's edge, beyond 2^32 for most
            off = int(rng.integers(TWO32 // BIG_FRAME - 128, BIG_NF)) * BIG_FRAME + int(rng.integers(-n, 64))
        elif kind == 2:                                                         # anywhere beyond 2^32
            off = int(rng.integers(TWO32, BIG_N - n))
        else:                                                                   # anywhere below
            off = int(rng.integers(0, TWO32 - n))
        off = max(0, min(off, BIG_N - n))
        ranges.append((off, n))
    ranges += [(TWO32 - 1, 2), (TWO32, 1), (TWO32 - 1, 1), (BIG_N - 1, 1), (BIG_N, 0)]
    ranges.insert(700, (TWO32 - (3 << 19) - 5, 3 << 20))                        # 3 MiB straddling 2^32
    assert sum(1 for o, n in ranges if o < TWO32 < o + n) >= 20 and sum(1 for o, _ in ranges if o > TWO32) >= 900
    for mode in ("packed", "padded"):
        given, offs, end = destinations(ranges, mode)
        d_dst = torch.full((end + TAIL,), POISON, dtype=torch.uint8, device=dev)
        d_st = torch.full((len(ranges),), -12345, dtype=torch.int32, device=dev)
        rc = engine.read_ranges_dev(comp, csize, d_c, d_d, BIG_NF, _dev_u64([o for o, _ in ranges]), _dev_u64([n for _, n in ranges]),
                                    _dev_u64(given) if given is not None else None, len(ranges), d_dst, end, True, d_st)
        assert rc == 0 and not d_st.cpu().numpy().any()
        got = d_dst.cpu().numpy()
        want = np.full(len(got), POISON, np.uint8)
        for (o, n), at in zip(ranges, offs):
            want[at:at + n] = _big_expected(hdr, fill, o, n)
        assert np.array_equal(got, want), (mode, int(np.nonzero(got != want)[0][0]))


# ---- 8. kernel variants feed the copy
@pytest.mark.parametrize("choice", [dict(exec_seg=2), dict(small_path=1), dict(small_path=2)], ids=["exec_seg2", "small_path1", "small_path2"])
def test_ranges_under_pinned_kernel_variants(engine, choice):
    try:
        engine.set_kernel_choice(reset=0)
        engine.set_kernel_choice(**choice)
        for name in ("text_l1_64k", "slices_l19"):
            g = next(x for x in GOLDENS if x.name == name)
            arc = golden_arc(g)
            ranges = make_ranges(arc, 0x3141)
            for mode in ("packed", "padded"):
                check(engine, arc, ranges, mode)
            outs, st = engine.read_ranges(g.comp + b"\0" * 8, arc.c, arc.d, [o for o, _ in ranges], [n for _, n in ranges])
            assert not st.any() and all(b == arc.data[o:o + n].tobytes() for (o, n), b in zip(ranges, outs))
    finally:
        engine.set_kernel_choice(reset=0)


def test_ranges_of_a_reference_made_archive(engine):
    """frames written by libzstd at level 3: blocks with their own tables, the per-block-table kernels in front of the copy"""
    arc = made_arc(engine, "ref_l3")
    ranges = make_ranges(arc, 0x2718)
    for mode in ("packed", "padded"):
        check(engine, arc, ranges, mode)
    try:
        engine.set_kernel_choice(exec_seg=2)
        check(engine, arc, ranges, "ragged")
    finally:
        engine.set_kernel_choice(reset=0)

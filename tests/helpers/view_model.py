"""Byte ranges of a view of an archive (zk_read_view_ranges_dev, include/zeekstd_amd.h "THE RULE"): the rule in numpy and plain Python, the cases
the CPU tests run, and the kernels of zeekstd_amd/csrc/zk_view.h under the workgroup emulator (tests/sim/zk_view_sim.cpp).  The model never looks
at compressed bytes: its archive is the list of the frames' decoded bytes."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(os.path.dirname(HERE), "sim")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, n) for n in ("zk_view_sim.cpp", "hip_wg_emu.h")] + [os.path.join(CSRC, h) for h in ("zk_view.h", "zk_ranges.h", "zk_range_copy.h")]

POISON = 0xA5
ARGUMENT = -2003            # ZK_ERR_ARGUMENT
OUT_OF_RANGE = -1001        # ZK_ERR_OFFSET_OUT_OF_RANGE
DST_TOO_SMALL = -70
U64 = (1 << 64) - 1


def view_ok(sizes, ids, voff):
    """the three conditions on a view, over the whole of it"""
    n = len(sizes)
    if len(voff) != len(ids) + 1:
        return False
    for j, f in enumerate(ids):
        if int(f) >= n or int(voff[j + 1]) < int(voff[j]) or int(voff[j + 1]) - int(voff[j]) != int(sizes[int(f)]):
            return False
    return True


def entry_of(voff, off):
    """the LAST j with voff[j] <= off: an offset on a boundary belongs to the entry that starts there, empty entries are skipped"""
    return int(np.searchsorted(np.asarray(voff, np.uint64), np.uint64(off), "right")) - 1


def model(frames, ids, voff, offs, lens, dst_off, dst_cap, size, poison=POISON, frame_err=None, failed_fill=None):
    """frames: the decoded bytes of every archive frame (bytes or uint8 arrays; a frame that is never read may be given by a bytes-like of its
    size only); ids / voff: the view; offs / lens / dst_off (None: packed): the ranges; size: bytes of the destination buffer to model;
    frame_err: {frame: ZSTD_ErrorCode} of the frames that fail to decode; failed_fill: the byte a decoder is known to leave in their place (the
    emulator harness's), None: their pieces stay poison and are listed as unspecified.
    -> dict(rc, dst, status, decoded, unspecified): dst None and status None for a refused view; decoded: the set of distinct frames decoded;
    unspecified: [(at, n)] destinations of ranges that failed for a frame -- their bytes are nobody's promise"""
    frame_err = frame_err or {}
    sizes = [len(f) for f in frames]
    ids = [int(x) for x in ids]
    voff = [int(x) for x in voff]
    if not view_ok(sizes, ids, voff):
        return dict(rc=ARGUMENT, dst=None, status=None, decoded=set(), unspecified=[])
    v0, vend = voff[0], voff[-1]
    dst = np.full(size, poison, np.uint8)
    status, decoded, unspecified = [], set(), []
    at = 0
    for i, (off, n) in enumerate(zip(offs, lens)):
        off, n = int(off), int(n)
        src_ok = v0 <= off <= vend and n <= vend - off
        to = int(dst_off[i]) if dst_off is not None else at
        if dst_off is None and src_ok:
            at += n
        if not src_ok:
            status.append(OUT_OF_RANGE)
            continue
        if to > dst_cap or n > dst_cap - to:
            status.append(DST_TOO_SMALL)
            continue
        st = 0
        if n:
            j = entry_of(voff, off)
            pos = off
            while pos < off + n:
                e0, e1 = voff[j], voff[j + 1]
                if e1 > e0:
                    f = ids[j]
                    decoded.add(f)
                    hi = min(off + n, e1)
                    if st == 0 and f in frame_err:
                        st = -int(frame_err[f])
                    if f not in frame_err:
                        dst[to + pos - off:to + hi - off] = np.frombuffer(bytes(frames[f][pos - e0:hi - e0]), np.uint8)
                    elif failed_fill is not None:
                        dst[to + pos - off:to + hi - off] = failed_fill
                    pos = hi
                j += 1
            if st:
                unspecified.append((to, n))
        status.append(st)
    rc = next((s for s in status if s), 0)
    return dict(rc=rc, dst=dst, status=np.array(status, np.int32), decoded=decoded, unspecified=unspecified)


# ---------------------------------------------------------------------------------------------- views and ranges
def offsets_of(sizes, ids, base=0):
    return np.concatenate([[base], base + np.cumsum([int(sizes[int(f)]) for f in ids], dtype=np.uint64)]).astype(np.uint64)


def views(sizes, seed=7):
    """{name: (ids, voff)} over an archive with the given frame sizes: the shapes a store hands back, and the edges"""
    n = len(sizes)
    rng = np.random.default_rng(seed)
    empty = [f for f in range(n) if sizes[f] == 0]
    full = [f for f in range(n) if sizes[f] != 0]
    v = {}
    v["identity"] = list(range(n))
    v["reversed"] = list(range(n))[::-1]
    v["thrice_in_a_row"] = [f for f in range(n) for _ in range(3)]
    v["thrice_interleaved"] = list(range(n)) * 3
    v["random_300"] = rng.integers(0, n, 300).tolist()
    v["subset"] = list(range(1, n, 3))
    v["single"] = [max(range(n), key=lambda f: sizes[f])]
    if empty:
        e = empty[0]
        v["empty_runs"] = [e] * 5 + full[:4] + [e] * 70 + full[4:9] + [e] * 3
    out = {k: (np.array(ids, np.uint32), offsets_of(sizes, ids)) for k, ids in v.items()}
    out["based_12345"] = (np.array(v["random_300"][:60], np.uint32), offsets_of(sizes, v["random_300"][:60], 12345))
    return out


def ranges_of(voff, seed=3, dense=True):
    """[(off, len)] over a view: the whole of it, every entry, every boundary +- 1 and across, the 16-byte and 64 KiB lengths at stream positions
    0, 1 and 15 mod 16, empty ranges on every boundary and at the end, duplicates and overlaps.  dense=False: boundaries of the first and last
    40 entries only"""
    voff = [int(x) for x in voff]
    v0, vend = voff[0], voff[-1]
    cnt = len(voff) - 1
    r = [(v0, vend - v0)]
    pick = list(range(cnt)) if dense or cnt <= 80 else list(range(40)) + list(range(cnt - 40, cnt))
    for j in pick:
        a, b = voff[j], voff[j + 1]
        r.append((a, b - a))
        r.append((a, 0))
        if a > v0:
            r.append((a - 1, 1))
            if a < vend:
                r.append((a - 1, 2))
        if a < vend:
            r.append((a, 1))
    r.append((vend, 0))
    for n in (1, 15, 16, 17, 65535, 65536, 65537):
        for m in (0, 1, 15):
            base = (v0 + 15) // 16 * 16 + m + 16 * (n % 7)
            if base + n <= vend:
                r.append((base, n))
            if vend - n >= v0:
                r.append((vend - n, n))
    rng = np.random.default_rng(seed)
    if vend > v0:
        for k in range(40):
            off = int(rng.integers(v0, vend))
            r.append((off, min(int(rng.integers(0, (300, 5000, 70000, 400000)[k % 4] + 1)), vend - off)))
    r += [r[1], r[1], r[len(r) // 2]]
    x = v0 + (vend - v0) // 3
    r += [(x, min(1000, vend - x)), (min(x + 500, vend), min(1000, vend - min(x + 500, vend)))]
    order = rng.permutation(len(r))
    return [r[i] for i in order]


def destinations(ranges, mode, seed=1, v0=0, vend=None):
    """packed -> (None, offsets the call will use, end); shuffled -> explicit destinations in a shuffled order, an odd gap in front of each,
    starting at 0, 1 and 15 mod 16 in turn"""
    if mode == "packed":
        offs, at = [], 0
        for o, n in ranges:
            offs.append(at)
            if vend is None or (v0 <= o <= vend and n <= vend - o):
                at += n
        return None, offs, at
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(ranges))
    offs, at = [0] * len(ranges), 0
    for k, i in enumerate(order):
        at += int(rng.integers(0, 40)) * 2 + 1
        at = (at + 15) // 16 * 16 + (0, 1, 15)[k % 3]
        offs[i] = at
        o, n = ranges[i]
        if vend is None or (v0 <= o <= vend and n <= vend - o):       # (a range outside the stream is given no room here either)
            at += n
    return offs, offs, at


def first_diff(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return None if bad.size == 0 else (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def payload(frame, size):
    """the bytes of frame `frame`: a function of (frame, position), so that a misplaced byte names its origin"""
    p = np.arange(size, dtype=np.uint64)
    return ((np.uint64(frame) * np.uint64(131) + p * np.uint64(7) + (p >> np.uint64(8)) * np.uint64(13) + (p >> np.uint64(16)) * np.uint64(29) + np.uint64(1))
            & np.uint64(0xFF)).astype(np.uint8)


EDGE_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 65535, 65537, 200000)


def edge_sizes(seed=11):
    """the frame sizes of the issue's archive: the 16-byte edges, the 64 KiB tile edges, a frame over four tiles, a dozen of 1-3 KiB"""
    rng = np.random.default_rng(seed)
    return list(EDGE_SIZES) + rng.integers(1024, 3073, 12).tolist()


# ---------------------------------------------------------------------------------------------- the kernels under the emulator
_LIB = None


def build_sim(out_dir):
    """tests/sim/zk_view_sim.cpp compiled with g++ into out_dir (a temporary directory of the test's)"""
    global _LIB
    if _LIB is None:
        so = os.path.join(str(out_dir), "libzk_view_sim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        P, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        l.zk_view_sim.restype = C.c_int
        l.zk_view_sim.argtypes = [P, P, u32, P, P, u32, P, P, P, u32, P, u64, u64, u32, u64, P, C.c_int, P, P]
        for f, k in ((l.zkv_sim_chunks, 2), (l.zkv_sim_chunk_begin, 2), (l.zkv_sim_chunk_end, 3)):
            f.restype = u64
            f.argtypes = [u64] * k
        l.zkv_sim_check.restype = C.c_int32
        l.zkv_sim_check.argtypes = [u64] * 6
        l.zkv_sim_chunk_wgs.restype = u32
        l.zkv_sim_chunk_wgs.argtypes = [u32, u64]
        _LIB = l
    return _LIB


def sim(lib, frames, ids, voff, offs, lens, dst_off, dst_cap, size, misalign=0, pass_bytes=0, frame_err=None, descending=False):
    """the kernels on a case -> dict(rc, dst, status, decoded (a count), passes); a refused view: dst and status still poisoned"""
    sizes = np.array([len(f) for f in frames], np.uint64)
    d_off = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
    data = np.concatenate([np.frombuffer(bytes(f), np.uint8) for f in frames] + [np.zeros(1, np.uint8)])
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    voff = np.ascontiguousarray(voff, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    do = np.ascontiguousarray(dst_off, dtype=np.uint64) if dst_off is not None else None
    dst = np.full(size, POISON, np.uint8)
    status = np.full(max(len(offs), 1), -12345, np.int32)
    ferr = np.zeros(len(frames) + 1, np.int32)
    for f, code in (frame_err or {}).items():
        ferr[f] = code
    out = (C.c_uint64 * 2)()
    rc = lib.zk_view_sim(data.ctypes.data, d_off.ctypes.data, len(frames), ids.ctypes.data, voff.ctypes.data, len(ids), offs.ctypes.data, lens.ctypes.data,
                         do.ctypes.data if do is not None else None, len(offs), dst.ctypes.data, dst_cap, size, misalign, pass_bytes, ferr.ctypes.data,
                         int(descending), status.ctypes.data, out)
    return dict(rc=rc, dst=dst, status=status[:len(offs)], decoded=int(out[0]), passes=int(out[1]))

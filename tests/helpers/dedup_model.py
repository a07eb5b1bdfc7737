"""Duplicate frames (zk_dedup_frames*, include/zeekstd_amd.h "THE RULE"): the model -- a dict from a frame's bytes to the first index
that had them --, the input list the CPU and the GPU tests share, and the kernels of zeekstd_amd/csrc/zk_dedup.h under the workgroup
emulator (tests/sim/zk_dedup_sim.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_dedup_sim.cpp"), os.path.join(SIM, "hip_wg_emu.h")] + [os.path.join(CSRC, h) for h in ("zk_dedup.h", "zk_device.h")]
KEY_BITS = (0, 1, 4, 16)
SLICES = (0, 1024)                      # bytes: ZK_CHOICE_DEDUP_SLICE_KIB 0 (the default) and 1
ALIGNS = (0, 1, 3, 7, 8, 15)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4097)
BIG = 200003                            # more than one piece of 64 KiB: the compare by several workgroups
PIECE = 64 << 10


def model(frames):
    """frames: a list of bytes -> (ref, uniq, ids) as np.uint32 arrays"""
    first = {}
    ref = np.zeros(len(frames), np.uint32)
    for i, f in enumerate(frames):
        ref[i] = first.setdefault(bytes(f), i)
    uniq = np.array([i for i in range(len(frames)) if ref[i] == i], np.uint32)
    place = {int(u): k for k, u in enumerate(uniq)}
    ids = np.array([place[int(r)] for r in ref], np.uint32)
    return ref, uniq, ids


class Case:
    """buf: the allocation's bytes; off: count + 1 offsets into it (off[0] = lead, off[count] = len(buf): the source ends with it)"""

    def __init__(self, name, frames, lead=0):
        self.name = name
        self.frames = [bytes(f) for f in frames]
        self.lead = lead
        self.buf = np.frombuffer(b"\xEE" * lead + b"".join(self.frames), np.uint8)
        self.off = np.zeros(len(frames) + 1, np.uint64)
        self.off[0] = lead
        self.off[1:] = lead + np.cumsum([len(f) for f in self.frames], dtype=np.uint64)
        self.count = len(frames)
        self._model = None

    def model(self):
        if self._model is None:
            self._model = model(self.frames)
        return self._model

    def unique_bytes(self):
        return b"".join(self.frames[int(u)] for u in self.model()[1])


def _edges():
    rng = np.random.default_rng(20)
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    frames = []
    pos = [0]

    def add(f):
        frames.append(bytes(f))
        pos[0] += len(f)

    def place(f, align):
        """f begins `align` bytes behind a 16-byte boundary of the source (a frame of fresh bytes fills up to there)"""
        gap = (align - pos[0]) % 16
        if gap:
            add(fresh(gap))
        add(f)

    def flip(f, at):
        b = bytearray(f)
        b[at] ^= 0x40
        return bytes(b)

    for n in LENGTHS + (BIG,):
        c = fresh(n)
        add(c)
        add(b"")                                            # several empty frames, all equal
        if n == 0:
            continue
        add(flip(c, 0))                                     # the first byte only
        add(flip(c, n - 1))                                 # the last byte only
        add(c[:-1])                                         # a strict prefix
        add(c + c[-1:])                                     # one byte longer
        add(b"\0" * n)
        add(b"\0" * (n + 1))                                # equal bytes, lengths one apart
        seams = [s for k in range(16, n, 16) for s in (k - 1, k)]
        if n == BIG:                                        # ... every seam of a long frame would be 25 000 frames: the first, the piece's, the last
            seams = [15, 16, PIECE - 1, PIECE, 2 * PIECE - 1, 2 * PIECE, 3 * PIECE, (n // 16) * 16 - 1, (n // 16) * 16]
        elif n > 64:
            seams = seams[:4] + seams[-4:]
        for s in seams:
            place(flip(c, s), rng.integers(0, 16))          # the byte on either side of a 16-byte seam, wherever the copy lies
        add(c)                                              # and a true copy behind all the near ones
    # two copies at every pair of alignments: a short frame (compared by a lane) and one of 333 bytes (by a workgroup)
    for n in (40, 333):
        for a in ALIGNS:
            for b in ALIGNS:
                c = fresh(n)
                place(c, a)
                place(c, b)
    c = fresh(BIG)
    place(c, 1)
    place(c, 8)
    return Case("edges", frames, lead=5)


def _far_pairs():
    """a content whose first copy is the list's first frame and whose second is its last, and one the other way round among 1000 others:
    the smallest index must win whichever workgroup inserts first"""
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(8, 200, 1000)]
    frames[999] = frames[0]
    frames[1] = frames[998]
    frames[700] = frames[300]
    return Case("far_pairs", frames)


def _many():
    rng = np.random.default_rng(22)
    contents = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(8, 41, 3000)]
    return Case("many", [contents[int(k)] for k in rng.integers(0, 3000, 70000)])


def _enc_mix():
    """frames worth compressing for the encode tests: sentences of a small vocabulary, some repeated, one of 70 000 bytes twice, an empty one"""
    rng = np.random.default_rng(24)
    words = [bytes(rng.integers(97, 123, int(n), dtype=np.uint8)) for n in rng.integers(2, 9, 200)]
    text = lambda n: b" ".join(words[int(k)] for k in rng.integers(0, 200, n // 5 + 1))[:n]
    distinct = [text(int(n)) for n in (1, 15, 40, 64, 65, 300, 333, 1000, 1500, 4097, 9000, 70000)]
    order = [0, 1, 2, 2, 3, 4, 5, 0, 6, 7, 7, 7, 8, 9, 5, 10, 11, 9, 11, 1]
    frames = [distinct[k] for k in order]
    frames.insert(4, b"")
    frames.insert(9, b"")
    return Case("enc_mix", frames, lead=3)


_CASES = None


def cases():
    """{name: Case}: the shared list"""
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(23)
        fresh = lambda n: rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()
        one = fresh(37)
        long_one = fresh(300)
        out = [_edges(), _far_pairs(), _many(), _enc_mix(),
               Case("one", [fresh(100)]), Case("one_empty", [b""]), Case("all_empty", [b""] * 300),
               Case("all_same", [one] * 600), Case("all_same_long", [long_one] * 300, lead=3),
               Case("all_distinct", [fresh(n) for n in rng.integers(8, 81, 600)], lead=1)]
        _CASES = {c.name: c for c in out}
    return _CASES


def frame_hash(f):
    """zk_k_dedup_hash's value (zk_dedup.h): the frame as 8-byte words counted from its first byte, zero-padded to a multiple of 16; word w gives
    fmix64(value + (w + 1) * 0x9E3779B97F4A7C15); the sum of the terms' low halves | the sum of their high halves << 32, each mod 2^32"""
    f = bytes(f)
    f += b"\0" * (-len(f) % 16)
    with np.errstate(over="ignore"):
        x = np.frombuffer(f, "<u8") + (np.arange(len(f) // 8, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    lo = int((x & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)) & 0xFFFFFFFF
    hi = int((x >> np.uint64(32)).sum(dtype=np.uint64)) & 0xFFFFFFFF
    return lo | hi << 32


def hashes(case):
    """XXH64 of every frame (the oracle's): another key function"""
    from oracle import zko
    memo = {}
    return np.array([memo.setdefault(f, zko.xxh64(f)) for f in case.frames], np.uint64)


# ---------------------------------------------------------------------------------------------- the kernels under the emulator
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_dedup_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_dedup_sim.restype = C.c_int
        l.zk_dedup_sim.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p]
        _LIB = l
    return _LIB


def sim(case, hash64=None, key_bits=0, misalign=0, descending=False, slice_bytes=None):
    """the map (and, with slice_bytes not None, the gather) as zk_dedup.hip runs them -> dict(ref, uniq, ids, rounds, gathered, slices, hash).
    hash64: the frames' hashes in zk_k_dedup_hash's place (None: the kernel's)"""
    src = np.ascontiguousarray(case.buf[case.lead:])
    h = np.ascontiguousarray(hash64, dtype=np.uint64) if hash64 is not None else None
    used = np.zeros(case.count, np.uint64)
    n = case.count
    ref, uniq, ids = (np.full(n, 0x5A5A5A5A, np.uint32) for _ in range(3))
    nu, rounds, slices = C.c_uint32(), C.c_uint32(), C.c_uint32()
    gathered = np.full(max(len(src), 1), 0x5A, np.uint8) if slice_bytes is not None else None
    rc = lib().zk_dedup_sim(src.ctypes.data, len(src), misalign, case.off.ctypes.data, n, h.ctypes.data if h is not None else None, key_bits, int(descending), ref.ctypes.data,
                            uniq.ctypes.data, ids.ctypes.data, C.byref(nu), C.byref(rounds), gathered.ctypes.data if gathered is not None else None,
                            slice_bytes or 0, C.byref(slices), used.ctypes.data)
    assert rc == 0, rc
    nb = sum(len(case.frames[int(u)]) for u in uniq[:nu.value]) if gathered is not None else 0
    return dict(ref=ref, uniq=uniq[:nu.value], ids=ids, rounds=rounds.value, gathered=gathered[:nb].tobytes() if gathered is not None else None,
                slices=slices.value, hash=used)

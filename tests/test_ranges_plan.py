"""The per-range arithmetic of zk_read_ranges* (zeekstd_amd/csrc/zk_ranges.h: the header the plan kernels and the host-pointer entry
point share) compiled with g++ and held against np.searchsorted and a plain Python piece splitter.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1

CLIENT = r"""
#include "zk_ranges.h"
extern "C" {
uint32_t t_frame_of(const uint64_t *d, uint32_t n, uint64_t off) { return zkr_frame_of(d, n, off); }
int32_t t_check(uint64_t total, uint64_t off, uint64_t len, uint64_t cap, uint64_t dst_off) { return zkr_check(total, off, len, cap, dst_off); }
int t_span(const uint64_t *d, uint32_t n, uint64_t off, uint64_t len, uint32_t *first, uint32_t *last) { return zkr_span(d, n, off, len, first, last); }
void t_piece(const uint64_t *d, uint32_t f, uint64_t off, uint64_t len, uint64_t *at, uint64_t *cnt, uint64_t *dst_at) { zkr_piece(d, f, off, len, at, cnt, dst_at); }
void t_clip(uint64_t off, uint64_t len, uint64_t wlo, uint64_t whi, uint64_t *lo, uint64_t *n) { zkr_clip(off, len, wlo, whi, lo, n); }
}
"""


@pytest.fixture(scope="module")
def zkr(tmp_path_factory):
    d = tmp_path_factory.mktemp("ranges_plan")
    src = d / "client.cpp"
    src.write_text(CLIENT)
    so = d / "libranges_plan.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "zeekstd_amd", "csrc"), "-o", str(so), str(src)])
    l = C.CDLL(str(so))
    P = C.c_void_p
    l.t_frame_of.restype = C.c_uint32
    l.t_frame_of.argtypes = [P, C.c_uint32, C.c_uint64]
    l.t_check.restype = C.c_int32
    l.t_check.argtypes = [C.c_uint64] * 5
    l.t_span.restype = C.c_int
    l.t_span.argtypes = [P, C.c_uint32, C.c_uint64, C.c_uint64, P, P]
    l.t_piece.restype = None
    l.t_piece.argtypes = [P, C.c_uint32, C.c_uint64, C.c_uint64, P, P, P]
    l.t_clip.restype = None
    l.t_clip.argtypes = [C.c_uint64] * 4 + [P, P]
    return l


def tables():
    """(name, frame sizes): empty frames in front, in the middle and at the end, one-frame tables, sums past 2^32, random ones"""
    rng = random.Random(20260817)
    t = [("one", [1000]), ("one_byte", [1]), ("one_empty", [0]), ("no_frames", []),
         ("empty_front", [0, 0, 5, 7]), ("empty_middle", [5, 0, 0, 0, 7, 0, 3]), ("empty_end", [4, 9, 0, 0]),
         ("empty_everywhere", [0, 3, 0, 0, 1, 1, 0, 8, 0]), ("all_empty", [0, 0, 0]),
         ("past_4g", [1 << 31, (1 << 31) - 1, 1, 0, 7, 1 << 32, 3]), ("past_4g_many", [0x200000] * 2304),
         ("huge", [(1 << 62), 0, (1 << 62), 5])]
    for k in range(40):
        n = rng.choice([1, 2, 3, 7, 64, 300])
        big = k % 5 == 0
        t.append((f"random{k}", [0 if rng.random() < 0.3 else rng.randrange(1, (1 << 33) if big else 5000) for _ in range(n)]))
    return t


def offsets_of(d, total, rng):
    """offsets exactly on every frame boundary, on both sides of them, at the end, and random ones"""
    offs = {0, total}
    for x in d[:400].tolist() + d[-400:].tolist():
        offs.update({x, max(x - 1, 0), min(x + 1, total)})
    offs.update(rng.randrange(0, total + 1) for _ in range(200))
    return sorted(offs)


@pytest.mark.parametrize("name,sizes", tables(), ids=[t[0] for t in tables()])
def test_frame_of_is_searchsorted_right_minus_one(zkr, name, sizes):
    rng = random.Random(name)
    d = np.zeros(len(sizes) + 1, np.uint64)
    d[1:] = np.cumsum(np.array(sizes, dtype=np.uint64), dtype=np.uint64)
    total = int(d[-1])
    for off in offsets_of(d, total, rng):
        want = int(np.searchsorted(d, np.uint64(off), "right")) - 1
        got = zkr.t_frame_of(d.ctypes.data, len(sizes), off)
        assert got == want, (off, got, want)
        if off < total:                                  # the frame is the one that holds the byte, never an empty one
            assert sizes[got] > 0 and int(d[got]) <= off < int(d[got + 1])
        else:
            assert got == len(sizes)                     # off == total: no frame


def py_pieces(d, sizes, off, length):
    """plain splitter: [(frame, at, n, dst_at)] of a valid range, frame by frame"""
    out = []
    end = off + length
    for f, sz in enumerate(sizes):
        fb, fe = int(d[f]), int(d[f + 1])
        lo, hi = max(off, fb), min(end, fe)
        if hi > lo:
            out.append((f, lo - fb, hi - lo, lo - off))
    return out


@pytest.mark.parametrize("name,sizes", [t for t in tables() if len(t[1]) <= 400], ids=[t[0] for t in tables() if len(t[1]) <= 400])
def test_span_and_pieces_against_a_plain_splitter(zkr, name, sizes):
    rng = random.Random("p" + name)
    n = len(sizes)
    d = np.zeros(n + 1, np.uint64)
    d[1:] = np.cumsum(np.array(sizes, dtype=np.uint64), dtype=np.uint64)
    total = int(d[-1])
    offs = offsets_of(d, total, rng)
    first, last = C.c_uint32(), C.c_uint32()
    at, cnt, dst_at = C.c_uint64(), C.c_uint64(), C.c_uint64()
    cases = [(total, 0), (0, total), (0, 0)]
    for off in offs:
        for length in {0, min(1, total - off), min(2, total - off), total - off, rng.randrange(0, total - off + 1), min(total - off, rng.randrange(1, 6000))}:
            cases.append((off, length))
    for off, length in cases:
        assert zkr.t_check(total, off, length, U64, 0) == 0
        want = py_pieces(d, sizes, off, length)
        touched = zkr.t_span(d.ctypes.data, n, off, length, C.byref(first), C.byref(last))
        assert bool(touched) == bool(want) == (length > 0)
        if not touched:
            continue
        assert (first.value, last.value) == (want[0][0], want[-1][0]), (off, length)
        got = []
        for f in range(first.value, last.value + 1):
            zkr.t_piece(d.ctypes.data, f, off, length, C.byref(at), C.byref(cnt), C.byref(dst_at))
            if cnt.value:
                got.append((f, at.value, cnt.value, dst_at.value))
            else:
                assert sizes[f] == 0                     # inside a span only empty frames hold nothing
        assert got == want, (off, length)
        assert sum(p[2] for p in got) == length
    # frames outside the span hold nothing of the range
    if n >= 2 and sizes[0] and sizes[-1]:
        zkr.t_piece(d.ctypes.data, n - 1, 0, 1, C.byref(at), C.byref(cnt), C.byref(dst_at))
        assert cnt.value == 0


def test_validation_codes_and_overflow(zkr):
    chk = zkr.t_check
    assert chk(100, 100, 0, 10, 10) == 0                 # off == total with len == 0; dst_off == dst_cap with len == 0
    assert chk(100, 101, 0, 10, 0) == -1001
    assert chk(100, 100, 1, 10, 0) == -1001
    assert chk(100, 0, 100, 100, 0) == 0
    assert chk(100, 0, 100, 99, 0) == -70
    assert chk(100, 1, 100, 1000, 0) == -1001
    # off + len overflows 2^64
    assert chk(100, 50, U64, U64, 0) == -1001
    assert chk(100, 50, U64 - 49, U64, 0) == -1001
    assert chk(U64, U64 - 1, 2, U64, 0) == -1001
    assert chk(U64, U64 - 1, 1, U64, 0) == 0
    # dst_off + len overflows 2^64
    assert chk(1 << 40, 0, 16, 1 << 40, U64 - 3) == -70
    assert chk(1 << 40, 0, 16, U64, U64 - 15) == -70
    assert chk(1 << 40, 0, 16, U64, U64 - 16) == 0
    # the source's verdict comes first
    assert chk(100, 200, 5, 1, 7) == -1001
    # past 2^32
    t = 9 << 32
    assert chk(t, (1 << 32) - 1, 3 << 20, t, 1 << 33) == 0
    assert chk(t, t - 5, 6, t, 0) == -1001


def test_clip_to_a_pass_window(zkr):
    rng = random.Random(7)
    lo, n = C.c_uint64(), C.c_uint64()
    for _ in range(3000):
        big = rng.random() < 0.3
        top = (1 << 40) if big else 1000
        off, length = rng.randrange(top), rng.randrange(top)
        wlo = rng.randrange(top)
        whi = wlo + 1 + rng.randrange(top)
        zkr.t_clip(off, length, wlo, whi, C.byref(lo), C.byref(n))
        a, b = max(off, wlo), min(off + length, whi)
        assert n.value == max(b - a, 0)
        if n.value:
            assert lo.value == a

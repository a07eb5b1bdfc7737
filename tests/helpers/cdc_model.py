"""TEST INFRASTRUCTURE -- a numpy model of the rule zk_chunk_boundaries cuts by (include/zeekstd_amd.h; zeekstd_amd/csrc/zk_cdc.h), written
from the rule's text and sharing nothing with the kernels but the gear table's three constants; the loader of tests/sim/zk_cdc_sim.cpp (the
kernels on the CPU under the workgroup emulator); and the inputs that the CPU and the GPU tests share.  Used by tests/test_cdc_model.py,
tests/test_sim_cdc.py and tests/test_gpu_cdc.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_cdc_sim.cpp"), os.path.join(SIM, "hip_wg_emu.h")] + [os.path.join(CSRC, h) for h in ("zk_cdc.h", "zk_device.h")]
M32 = np.uint64(0xFFFFFFFF)
SETTINGS = ((64, 256, 1024), (256, 1024, 4096), (1024, 4096, 16384))            # (min, avg, max)
MAX_FRAME_SIZE = 0x40000000


# ---------------------------------------------------------------------------------------------- the rule
def gear():
    """G[b], b = 0..255"""
    x = ((np.arange(256, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B1)) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def _arr(a):
    return np.frombuffer(bytes(a), np.uint8) if not isinstance(a, np.ndarray) else a


def hashes(a):
    """h(p) for every position: the sum over j = 0..31 of G[a[p - j]] << j mod 2^32, terms before the first byte absent"""
    a = _arr(a)
    n = len(a)
    g = gear()[a].astype(np.uint64)
    h = np.zeros(n, np.uint64)
    for j in range(min(32, n)):
        h[j:] += g[:n - j] << np.uint64(j)              # (uint64 wraps mod 2^64, of which 2^32 is a divisor)
    return (h & M32).astype(np.uint32)


def candidates(a, bits):
    """bool per position"""
    return (hashes(a) >> np.uint32(32 - bits)) == 0


def bitmap(a, bits):
    """the candidates as the device keeps them: position p is bit p & 7 of byte p >> 3"""
    return np.packbits(candidates(a, bits), bitorder="little")


def cuts(a, mn, bits, mx):
    """off[count + 1] as np.uint64"""
    a = _arr(a)
    n = len(a)
    if n == 0:
        return np.zeros(2, np.uint64)
    q = np.nonzero(candidates(a, bits))[0] + 1
    off, c = [0], 0
    while c < n:
        lo, hi = c + mn, min(c + mx, n)
        i = int(np.searchsorted(q, lo))
        c = int(q[i]) if i < len(q) and q[i] <= hi else hi
        off.append(c)
    return np.asarray(off, np.uint64)


def resolve(mn=0, avg=0, mx=0, flags=0):
    """zk_chunk_params -> (min, bits, max), or None for what the library refuses"""
    avg = avg or 1 << 21
    if flags or avg < 1 << 8 or avg > 1 << 24 or avg & (avg - 1):
        return None
    mn = mn or avg // 4
    if mn < 64 or mn > avg:
        return None
    mx = mx or min(4 * avg, 1 << 30)
    if mx < mn or mx > MAX_FRAME_SIZE:
        return None
    return mn, avg.bit_length() - 1, mx


def dense_bytes():
    """the byte values a run of which makes EVERY position (from the 32nd on) a candidate at avg_size = 256: the run's hash is
    G[b] * (2^32 - 1) = -G[b], and its top 8 bits are zero"""
    g = gear().astype(np.uint64)
    return [b for b in range(256) if int(((np.uint64(1 << 32) - g[b]) & M32) >> np.uint64(24)) == 0]


# zk_chunk_params rows (min, avg, max, flags): accepted ones, then every kind of refusal -- avg no power of two / out of range, min out of
# range, max out of range, a flag
PARAM_TABLE = [(0, 0, 0, 0), (0, 256, 0, 0), (0, 1 << 24, 0, 0), (64, 256, 64, 0), (256, 256, 256, 0), (64, 1 << 24, 0x40000000, 0), (1 << 24, 1 << 24, 0, 0),
               (100, 1024, 5000, 0), (0, 1024, 300, 0),
               (0, 1000, 0, 0), (0, 128, 0, 0), (0, 1 << 25, 0, 0), (63, 256, 0, 0), (257, 256, 0, 0), (512, 1024, 511, 0), (0, 1024, 255, 0),
               (0, 256, 0x40000001, 0), (0, 0, 0, 1), (1 << 22, 0, 0, 0), (64, 256, 1024, 0x80000000)]


# ---------------------------------------------------------------------------------------------- the kernels under the emulator
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_cdc_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_cdc_sim.restype = C.c_int
        l.zk_cdc_sim.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_uint64, C.POINTER(C.c_uint64)]
        _LIB = l
    return _LIB


def sim(a, mn, bits, mx, slice_bytes=0, misalign=0, descending=False, off_cap=None):
    """zk_k_cdc_mark / _emit / _select under the emulator as zk_cdc_pass runs them -> (bitmap bytes, offsets incl. off[0], count)"""
    a = np.ascontiguousarray(_arr(a))
    n = len(a)
    assert n > 0
    cap = n // mn + 1 if off_cap is None else off_cap
    bm = np.full((n + 7) // 8, 0x5A, np.uint8)
    off = np.full(cap + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
    count = C.c_uint64()
    rc = lib().zk_cdc_sim(a.ctypes.data, n, mn, bits, mx, slice_bytes, misalign, int(descending), bm.ctypes.data, off.ctypes.data, cap, C.byref(count))
    assert rc == 0, rc
    return bm, off, int(count.value)


# ---------------------------------------------------------------------------------------------- inputs
def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def word_text(seed, n):
    rng = np.random.default_rng(seed)
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 10)))) for _ in range(500)]
    out, size = [], 0
    while size < n:
        w = words[int(rng.integers(0, 500))]
        out.append(w)
        size += len(w) + 1
    return np.frombuffer(" ".join(out).encode()[:n], np.uint8)


class Case:
    def __init__(self, name, data, mn, avg, mx):
        self.name, self.data, self.mn, self.avg, self.mx, self.bits = name, np.ascontiguousarray(data), mn, avg, mx, avg.bit_length() - 1

    def cuts(self):
        return cuts(self.data, self.mn, self.bits, self.mx)

    def bitmap(self):
        return bitmap(self.data, self.bits)


def _first_candidate(data, bits, at_least, at_most):
    q = np.nonzero(candidates(data, bits))[0] + 1
    q = q[(q >= at_least) & (q <= at_most)]
    assert len(q), "no candidate to build the input from"
    return int(q[0])


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}: every input of the shared list under the three settings (the inputs built for one bound bring their own min / max)"""
    dense = dense_bytes()
    assert len(dense) == 3
    mid = rand(3, 65536).copy()
    mid[30000:35000] = dense[0]
    base = {"random": rand(1, 256 << 10), "text": word_text(2, 200000), "zeros": np.zeros(100000, np.uint8), "dense_mid": mid}
    for b in dense:
        base["dense_%d" % b] = np.full(40000, b, np.uint8)
    out = {}
    # every position a candidate and min beyond the 64 entries the selection looks at in one step: it has to search
    out["dense_min200"] = Case("dense_min200", base["dense_%d" % dense[1]], 200, 256, 1024)
    out["dense_mid_min256"] = Case("dense_mid_min256", mid, 256, 256, 700)
    # ... and long enough for several segments of the parallel selection (81 920 bytes each at min 64, avg 256): rows full of cuts, and a run that
    # begins and ends inside segments
    out["dense_long"] = Case("dense_long", np.full(200000, dense[2], np.uint8), 64, 256, 1024)
    out["dense_long_min200"] = Case("dense_long_min200", np.full(200000, dense[0], np.uint8), 200, 256, 1024)
    long_mid = rand(4, 250000).copy()
    long_mid[75000:95000] = dense[1]
    out["dense_mid_long"] = Case("dense_mid_long", long_mid, 64, 256, 1024)
    for mn, avg, mx in SETTINGS:
        tag = "_%d" % avg
        bits = avg.bit_length() - 1
        for name, data in base.items():
            out[name + tag] = Case(name + tag, data, mn, avg, mx)
        for n in sorted({0, 1, 31, 32, 33, mn - 1, mn, mn + 1, mx, mx + 1}):
            out["len%d%s" % (n, tag)] = Case("len%d%s" % (n, tag), rand(100 + n, n), mn, avg, mx)
        # a candidate offset exactly on lo = 0 + min, and one exactly on hi = 0 + max with none before it in [min, max)
        r = rand(7, 40000)
        q = _first_candidate(r, bits, 64, avg)
        out["on_lo" + tag] = Case("on_lo" + tag, r, q, avg, mx)
        q = _first_candidate(r, bits, mn, MAX_FRAME_SIZE)
        out["on_hi" + tag] = Case("on_hi" + tag, r, mn, avg, q)
        # the last frame shorter than min: cut off min / 2 bytes behind a cut
        r = rand(8, 30000)
        c = cuts(r, mn, bits, mx)
        out["short_last" + tag] = Case("short_last" + tag, r[:int(c[-3]) + mn // 2], mn, avg, mx)
        # min == max: the uniform grid
        out["equal" + tag] = Case("equal" + tag, rand(9, 10 * avg + 77), avg, avg, avg)
    return out

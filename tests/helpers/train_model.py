"""TEST INFRASTRUCTURE -- a numpy model of the rule zk_train_dictionary selects a dictionary's content by (include/zeekstd_amd.h;
zeekstd_amd/csrc/zk_train.h: zk_k_train_count, zk_k_train_select), written from the rule's text and sharing nothing with the kernels but the
hash's two multipliers; the loader of tests/sim/zk_train_sim.cpp (the kernels on the CPU under the workgroup emulator); and the inputs the
tests run, each with the facts that make it an edge, stated on the model alone.  Used by tests/test_sim_train.py and tests/test_gpu_train.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import dict_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_train_sim.cpp"), os.path.join(SIM, "hip_wg_emu.h")] + [os.path.join(CSRC, h) for h in ("zk_train.h", "zk_device.h", "zk_enc_device.h")]
TRIAL_BYTES = 64 << 20

NONE = 0xFFFFFFFF
PRIME = {6: 227718039650203, 8: 0xCF1BBCDCB7A56463}
HEADER_RESERVE = 512
K_SET = (64, 128, 256, 512)


def content_cap(cap):
    return min(cap - HEADER_RESERVE, (1 << 27) - 1)


def candidates(cap, k=0):
    return [k] if k else [c for c in K_SET if c <= cap // 4]


# ---------------------------------------------------------------------------------------------- the model
def join(samples):
    """list of bytes -> (uint8 array of all of them, uint64 offsets counted from 0)"""
    off = np.zeros(len(samples) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in samples], dtype=np.uint64)
    return np.frombuffer(b"".join(samples), np.uint8), off


def hashes(data, off, d, f):
    """hpos[N]: the hash of the d-mer at every position whose d bytes lie inside one sample, NONE elsewhere.  data[0] is position 0 and off
    counts from it (off[0] == 0)."""
    n = int(off[-1])
    data = np.asarray(data[:n], np.uint8)
    pad = np.concatenate([data, np.zeros(8, np.uint8)]).astype(np.uint64)
    v = np.zeros(n, np.uint64)
    for j in range(d):
        v |= pad[j:j + n] << np.uint64(8 * j)
    with np.errstate(over="ignore"):
        h = ((v << np.uint64(64 - 8 * d)) * np.uint64(PRIME[d])) >> np.uint64(64 - f)
    ends = np.asarray(off, np.uint64)[1:]
    end = ends[np.searchsorted(ends, np.arange(n, dtype=np.uint64), side="right")]        # the first offset above the position
    valid = np.arange(n, dtype=np.uint64) + np.uint64(d) <= end
    return np.where(valid, h, NONE).astype(np.uint32)


def count(hpos, f):
    return np.bincount(hpos[hpos != NONE], minlength=1 << f).astype(np.uint32)


def epochs(n, k, ccap):
    return max(1, min(ccap // k, n // (10 * k)))


def scores(hpos, freq, lo, hi, k, d):
    """the score of every segment start lo ... hi - k of one epoch"""
    h = hpos[lo:hi]
    val = np.where(h != NONE, freq[np.minimum(h, len(freq) - 1)], 0).astype(np.uint64)
    pre = np.concatenate([[0], np.cumsum(val, dtype=np.uint64)]).astype(np.uint64)
    ns, w = hi - lo - k + 1, k - d + 1
    return pre[w:w + ns] - pre[:ns]


def select(data, hpos, freq, k, d, ccap, trace=None):
    """-> (segment starts in the order taken, content bytes).  trace (a list): (round, epoch, start, score, maxima of that score) per take."""
    n = len(hpos)
    freq = freq.copy()
    E = epochs(n, k, ccap)
    es = n // E
    left, segs, rnd = ccap, [], 0
    more = True
    while more and left >= k:
        more = False
        for e in range(E):
            if left < k:
                break
            lo, hi = e * es, (e + 1) * es
            if es < k:
                continue
            sc = scores(hpos, freq, lo, hi, k, d)
            j = int(np.argmax(sc))                                  # (the first of equal maxima)
            if sc[j] == 0:
                continue
            if trace is not None:
                trace.append((rnd, e, lo + j, int(sc[j]), int((sc == sc[j]).sum())))
            segs.append(lo + j)
            h = hpos[lo + j:lo + j + k - d + 1]
            freq[h[h != NONE]] = 0
            left -= k
            more = True
        rnd += 1
    raw = bytes(np.asarray(data[:n], np.uint8))
    if not segs:
        m = min(n, ccap)
        return segs, raw[n - m:]
    return segs, b"".join(raw[s:s + k] for s in reversed(segs))


def trial_stride(sizes, limit=TRIAL_BYTES):
    """every j-th sample is tried: the smallest j whose samples 0, j, 2 j, ... total at most `limit`; the first sample alone when none does"""
    sizes = np.asarray(sizes, np.int64)
    for j in range(1, len(sizes)):
        if int(sizes[::j].sum()) <= limit:
            return j
    return max(len(sizes), 1)


def train(samples, cap, k, d=8, f=20):
    """the content zk_train_dictionary makes with k pinned"""
    data, off = join(samples)
    hp = hashes(data, off, d, f)
    return select(data, hp, count(hp, f), k, d, content_cap(cap))


# ---------------------------------------------------------------------------------------------- the emulated kernels
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_train_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_train_sim.restype = C.c_int
        l.zk_train_sim.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        l.zk_train_sim_stats.restype = C.c_int
        l.zk_train_sim_stats.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
        l.zk_train_sim_gather.restype = C.c_int
        l.zk_train_sim_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        _LIB = l
    return _LIB


def sim(buf, off, d, f, ks, ccap, descending=False):
    """zk_k_train_count and zk_k_train_select under the emulator with the launchers' grids.  buf: the caller's whole buffer, off: its
    offsets as given (off[0] may be above 0).  -> (hpos, freq as counted, [(segment starts, content bytes) per candidate])"""
    buf = np.frombuffer(bytes(buf), np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    n = int(off[-1] - off[0])
    ks_a = np.asarray(ks, np.uint32)
    segs_cap = ccap // min(ks) + 1
    hpos, freq = np.full(max(n, 1), 0x5A5A5A5A, np.uint32), np.full(1 << f, 0x5A5A5A5A, np.uint32)
    segs, content, out = np.full((len(ks), segs_cap), 0x5A5A5A5A, np.uint32), np.full((len(ks), ccap), 0x5A, np.uint8), np.zeros((len(ks), 2), np.uint32)
    rc = lib().zk_train_sim(buf.ctypes.data, off.ctypes.data, len(off) - 1, d, f, ks_a.ctypes.data, len(ks), ccap, int(descending),
                            hpos.ctypes.data, freq.ctypes.data, segs.ctypes.data, segs_cap, content.ctypes.data, out.ctypes.data)
    assert rc == 0, rc                                              # (-2: a write outside what the launcher's layout gives a candidate)
    res = []
    for c in range(len(ks)):
        nseg, nbytes = int(out[c, 0]), int(out[c, 1])
        res.append((segs[c, :nseg].tolist(), content[c, ccap - nbytes:].tobytes()))
    return hpos[:n], freq, res


# ---------------------------------------------------------------------------------------------- inputs
def fixture_samples():
    """the 3 000 samples the fixture's dictionary was trained on (tools/make_dict_goldens.py::train)"""
    rng = F.Lcg(7)
    return [b"".join(F.record(rng) for _ in range(1 + rng.next(4))) for _ in range(3000)]


def held_out():
    """the 120 frames the trained dictionary is judged on: 71 680 bytes"""
    return [F.records(9000 + i, fs) for fs in (256, 512, 1024) for i in range(40)]


class Case:
    def __init__(self, name, samples, k=32, d=8, f=16, ccap=1024, lead=0):
        self.name, self.samples, self.k, self.d, self.f, self.ccap, self.lead = name, samples, k, d, f, ccap, lead

    def buffers(self):
        """(the caller's buffer, offsets as the caller gives them): `lead` bytes of something else come first"""
        data, off = join(self.samples)
        return b"\xEE" * self.lead + data.tobytes(), off + np.uint64(self.lead)

    def model(self, trace=None):
        data, off = join(self.samples)
        hp = hashes(data, off, self.d, self.f)
        fr = count(hp, self.f)
        return hp, fr, select(data, hp, fr, self.k, self.d, self.ccap, trace)


def _recs(seed, n):
    return F.records(seed, n)


def cases():
    out = []
    # samples of d - 1, d and d + 1 bytes and empty ones among ordinary records; the list does not start at 0
    for d in (6, 8):
        s = [_recs(10, 700), b"", _recs(11, d - 1), _recs(12, d), b"", b"", _recs(13, d + 1), _recs(14, 900)] + [_recs(20 + i, 300 + 17 * i) for i in range(12)] + [b""]
        out.append(Case(f"short_samples_d{d}", s, d=d, lead=37))
    # f = 10: 1024 counters for several thousand different d-mers
    out.append(Case("collisions_f10", [_recs(40 + i, 400) for i in range(16)], f=10))
    # N / (10 k) = 1: one epoch, and the content cannot fill
    out.append(Case("one_epoch", [_recs(60 + i, 60) for i in range(10)], k=32))
    # N / (10 k) = 19 epochs against content_cap / k = 32: a second round is needed
    out.append(Case("second_round", [_recs(70 + i, 512) for i in range(12)]))
    # content_cap / k = 32 epochs against N / (10 k) = 62: the first round fills the content exactly
    out.append(Case("filled_exactly", [_recs(90 + i, 500) for i in range(40)]))
    # one period of 64 bytes throughout: the first segment clears every d-mer there is, the rest of the round and the next add nothing
    unit = _recs(5, 64)
    out.append(Case("nothing_left", [unit * 12] * 9))
    # the d-mers that occur most often lie around a boundary between two samples
    hot_a, hot_b = b"<<hot-region-A>>", b"<<hot-region-B>>"
    s = []
    for i in range(12):
        s += [F.noise(100 + i, 200) + hot_a, hot_b + F.noise(200 + i, 200)]
    out.append(Case("straddle", s, ccap=32, k=32))
    # two places of one epoch with the same score: the same 400 bytes twice in the one epoch
    blk = F.noise(7, 200)
    out.append(Case("tie", [blk, blk] + [bytes([i]) * 8 for i in range(8)], ccap=32, k=32))
    return {c.name: c for c in out}

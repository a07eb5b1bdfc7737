"""A frame list deduplicated against an existing archive (zk_dedup_against_dev, include/zeekstd_amd.h "THE RULE"): the model -- a dict from
bytes to the smallest archive id, then the in-call dict --, a numpy statement of the frame key, the generations the CPU and the GPU tests
share (built from helpers/dedup_model.cases()), and the kernels of zeekstd_amd/csrc/zk_dedup_index.h under the workgroup emulator
(tests/sim/zk_dedup_index_sim.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from helpers import dedup_model as M

DEPS = [os.path.join(M.SIM, "zk_dedup_index_sim.cpp"), os.path.join(M.SIM, "zk_dedup_sim.cpp"), os.path.join(M.SIM, "hip_wg_emu.h")] + \
       [os.path.join(M.CSRC, h) for h in ("zk_dedup_index.h", "zk_dedup.h", "zk_device.h")]
KEY_BITS = (0, 4, 1)
PASS_1K = 1024


def model(archive, frames):
    """archive: the decoded frames the index knows; frames: the list -> (ids, fresh) as np.uint32 arrays"""
    held = {}
    for s, f in enumerate(archive):
        held.setdefault(bytes(f), s)
    m = len(archive)
    local, fresh, ids = {}, [], []
    for i, f in enumerate(frames):
        f = bytes(f)
        if f in held:
            ids.append(held[f])
            continue
        if f not in local:
            local[f] = len(fresh)
            fresh.append(i)
        ids.append(m + local[f])
    return np.array(ids, np.uint32), np.array(fresh, np.uint32)


def frame_key(f):
    """The frame key as include/zeekstd_amd.h spells it out: little-endian 8-byte words from the frame's first byte, zero-padded to a multiple
    of 16 bytes; word w of value v gives fmix64(v + (w + 1) * 0x9E3779B97F4A7C15); the key is the sum of the terms' low halves | the sum of
    their high halves << 32, each mod 2^32"""
    f = bytes(f)
    f += b"\0" * (-len(f) % 16)
    if not f:
        return 0
    with np.errstate(over="ignore"):
        x = np.frombuffer(f, "<u8") + (np.arange(len(f) // 8, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        for mul in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
            x ^= x >> np.uint64(33)
            x *= np.uint64(mul)
        x ^= x >> np.uint64(33)
    lo = int((x & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)) & 0xFFFFFFFF
    hi = int((x >> np.uint64(32)).sum(dtype=np.uint64)) & 0xFFFFFFFF
    return lo | hi << 32


def frame_keys(frames):
    memo = {}
    return np.array([memo.setdefault(bytes(f), frame_key(f)) for f in frames], np.uint64)


def _flip(f, at):
    b = bytearray(f)
    b[at] ^= 0x40
    return bytes(b)


_GENS = None


def generations():
    """{name: [Case, ...]}: lists appended one after the other to an archive that starts empty (or as the test says)"""
    global _GENS
    if _GENS is not None:
        return _GENS
    cases = M.cases()
    rng = np.random.default_rng(31)
    words = [bytes(rng.integers(97, 123, int(n), dtype=np.uint8)) for n in rng.integers(2, 9, 150)]
    text = lambda n: b" ".join(words[int(k)] for k in rng.integers(0, 150, n // 5 + 1))[:n]
    mix = cases["enc_mix"]
    a, b, c, big = text(700), text(64), text(5000), text(150000)
    long_ = mix.frames[max(range(mix.count), key=lambda i: len(mix.frames[i]))]            # 70 000 bytes: more than one piece
    g2 = [mix.frames[5], a, mix.frames[0], _flip(long_, 0), _flip(long_, len(long_) - 1), b"", b, a, long_, _flip(long_, M.PIECE), c, text(1), mix.frames[2], big]
    g3 = [c, _flip(long_, M.PIECE - 1), b, big, mix.frames[7], text(15), text(17), _flip(big, 2 * M.PIECE), a, _flip(a, 699), b"", big]
    out = {"mix": [mix, M.Case("mix2", g2, lead=1), M.Case("mix3", g3, lead=7)]}
    # the list of edges -- frames of 0, 1, 15..17, 63..65 bytes and of several 64 KiB pieces, near-duplicates that differ in the first, the
    # last and the seam bytes --, then the same list again (the archive holds every frame: n_fresh == 0), then its near-duplicates once more
    # in another order among new ones
    edges = cases["edges"]
    order = rng.permutation(edges.count)
    again = [edges.frames[int(i)] for i in order[:150]] + [_flip(edges.frames[int(i)], 0) for i in order[:40] if edges.frames[int(i)]]
    out["edges"] = [edges, M.Case("edges_again", edges.frames, lead=3), M.Case("edges_mixed", again, lead=2)]
    # near-duplicates of equal length only: with 4 and 1 key bits they sit in one key group, and a frame meets several candidates in turn
    base = {n: bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (17, 65, 333, 2 * M.PIECE + 77)}
    near1, near2 = [], []
    for n, f in base.items():
        spots = sorted({0, n - 1, 15, 16, (n // 16) * 16 - 1} | ({M.PIECE - 1, M.PIECE, 2 * M.PIECE} if n > M.PIECE else set()))
        spots = [s for s in spots if 0 <= s < n]
        near1 += [_flip(f, s) for s in spots]
        near2 += [f] + [_flip(f, s) for s in reversed(spots)] + [_flip(_flip(f, spots[0]), spots[-1]), f]
    out["near"] = [M.Case("near1", near1, lead=1), M.Case("near2", near2, lead=5)]
    _GENS = out
    return out


def dup_archive():
    """an archive WITH duplicate contents (as one written without dedup holds them), and a list against it: the smallest s wins"""
    mix = M.cases()["enc_mix"]
    archive = [mix.frames[i] for i in (3, 0, 3, 5, 0, 12, 5, 12, 3)] + [b"", mix.frames[7], b""]
    frames = [mix.frames[i] for i in (12, 5, 3, 0, 7, 1)] + [b"", mix.frames[1], _flip(mix.frames[12], 1)]
    return archive, M.Case("dup_list", frames, lead=3)


# ---------------------------------------------------------------------------------------------- the kernels under the emulator
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(M.SIM, "libzk_dedup_index_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zkx_sim_create.restype = C.c_void_p
        l.zkx_sim_create.argtypes = [C.c_uint32]
        l.zkx_sim_free.argtypes = [C.c_void_p]
        for f in (l.zkx_sim_count, l.zkx_sim_slots):
            f.restype = C.c_uint32
            f.argtypes = [C.c_void_p]
        l.zkx_sim_table_ok.argtypes = [C.c_void_p]
        l.zkx_sim_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        l.zkx_sim_truncate.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        l.zkx_sim_export.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        l.zkx_sim_against.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.c_int, C.c_uint64, C.c_int] + [C.c_void_p] * 2 + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_uint64)]
        _LIB = l
    return _LIB


class SimIndex:
    """the index as zk_dedup_index.hip keeps it, its kernels under the emulator"""

    def __init__(self, bits=0):
        self._h = C.c_void_p(lib().zkx_sim_create(bits))

    def close(self):
        if self._h:
            lib().zkx_sim_free(self._h)
            self._h = None

    count = property(lambda self: lib().zkx_sim_count(self._h))
    slots = property(lambda self: lib().zkx_sim_slots(self._h))

    def table_ok(self):
        return bool(lib().zkx_sim_table_ok(self._h))

    def add(self, keys, lens, descending=False):
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        n = np.ascontiguousarray(lens, dtype=np.uint32)
        assert lib().zkx_sim_add(self._h, k.ctypes.data, n.ctypes.data, len(k), int(descending)) == 0

    def truncate(self, count, descending=False):
        assert lib().zkx_sim_truncate(self._h, count, int(descending)) == 0

    def export(self, first=0, count=None):
        count = self.count - first if count is None else count
        k, n = np.zeros(max(count, 1), np.uint64), np.zeros(max(count, 1), np.uint32)
        assert lib().zkx_sim_export(self._h, first, count, k.ctypes.data, n.ctypes.data) == 0
        return k[:count], n[:count]

    def against(self, archive, case, hash64=None, key_bits=0, misalign=0, descending=False, pass_bytes=0, take=False):
        """archive: the decoded archive frames (a list of bytes, at least self.count) -> dict(ids, fresh, rounds, passes, largest_pass)"""
        arch = np.frombuffer(b"".join(archive) + b"\0", np.uint8)
        arch_off = np.zeros(len(archive) + 1, np.uint64)
        arch_off[1:] = np.cumsum([len(f) for f in archive], dtype=np.uint64)
        src = np.ascontiguousarray(case.buf[case.lead:])
        h = np.ascontiguousarray(hash64, dtype=np.uint64) if hash64 is not None else None
        n = case.count
        ids, fresh = (np.full(n, 0x5A5A5A5A, np.uint32) for _ in range(2))
        nf, rounds, passes, largest = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        rc = lib().zkx_sim_against(self._h, arch.ctypes.data, arch_off.ctypes.data, len(archive), src.ctypes.data, len(src), misalign, case.off.ctypes.data, n,
                                   h.ctypes.data if h is not None else None, key_bits, int(descending), pass_bytes, int(take), ids.ctypes.data, fresh.ctypes.data,
                                   C.byref(nf), C.byref(rounds), C.byref(passes), C.byref(largest))
        assert rc == 0, rc
        return dict(ids=ids, fresh=fresh[:nf.value], rounds=rounds.value, passes=passes.value, largest_pass=largest.value)

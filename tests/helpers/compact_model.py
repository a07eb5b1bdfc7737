"""Frames removed from a device-resident archive (zk_compact_archive_dev, include/zeekstd_amd.h "THE RULE"): the rule in numpy, the inputs the
CPU and the GPU tests share, and the kernels of zeekstd_amd/csrc/zk_compact.h under the workgroup emulator (tests/sim/zk_compact_sim.cpp).
The inputs are small and chosen for the edges of the move kernel, not for realism; the payload need not be zstd, because the call never looks
inside it.  Every payload byte is a function of (frame, position), so a misplaced byte names its origin."""
import ctypes as C
import os
import subprocess

import numpy as np

from helpers import dedup_model as M

DEPS = [os.path.join(M.SIM, n) for n in ("zk_compact_sim.cpp", "zk_dedup_index_sim.cpp", "zk_dedup_sim.cpp", "hip_wg_emu.h")] + \
       [os.path.join(M.CSRC, h) for h in ("zk_compact.h", "zk_dedup_index.h", "zk_dedup.h", "zk_device.h")]
REMOVED = 0xFFFFFFFF
TILE = 64 << 10
EDGE_SIZES = (0, 1, 15, 16, 17, 31, 32, 33, 255, 4096, 65535, 65536, 65537, 200000)
STARTS = (0, 1, 3, 7)                          # bytes off a 256-byte boundary at which the GPU tests (and the emulator) place the buffer


def payload(frame, size):
    """the bytes of frame `frame`: a function of (frame, position)"""
    p = np.arange(size, dtype=np.uint64)
    return ((np.uint64(frame) * np.uint64(131) + p * np.uint64(7) + (p >> np.uint64(8)) * np.uint64(13) + (p >> np.uint64(16)) * np.uint64(29) + np.uint64(1))
            & np.uint64(0xFF)).astype(np.uint8)


def origin(frame_sizes, base, pos):
    """(frame, position) of the source byte at buffer position pos -- for a failure message"""
    c = base + np.concatenate([[0], np.cumsum(frame_sizes)])
    s = int(np.searchsorted(c, pos, side="right")) - 1
    return s, int(pos - c[s])


class Case:
    """an archive: comp (c_off[0] bytes of 0xC3 that belong to nobody, then the frames), c_off, d_off (uint64), live (uint8)"""

    def __init__(self, name, c_sizes, live, base=0):
        self.name = name
        n = len(c_sizes)
        self.n = n
        cs = np.asarray(c_sizes, dtype=np.uint64)
        self.c_off = np.uint64(base) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(cs, dtype=np.uint64)])
        ds = cs * np.uint64(3) + (np.arange(n, dtype=np.uint64) % np.uint64(5))
        self.d_off = np.uint64(7 * base) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(ds, dtype=np.uint64)])
        self.live = np.ascontiguousarray(live, dtype=np.uint8)
        assert len(self.live) == n
        self.comp = np.concatenate([np.full(base, 0xC3, np.uint8)] + [payload(s, int(cs[s])) for s in range(n)]) if n else np.full(base, 0xC3, np.uint8)
        self.comp_size = len(self.comp)
        self._model = None

    def model(self):
        if self._model is None:
            self._model = model(self.comp, self.c_off, self.d_off, self.live)
        return self._model

    def expect_in_place(self):
        """the whole buffer after an in-place compaction: [c_off[0], written) the model's bytes, everything else as it was"""
        m = self.model()
        out = self.comp.copy()
        out[int(self.c_off[0]):m["written"]] = m["dst"]
        return out

    def first_removed(self):
        """the offset where an in-place compaction begins to move: of the first removed frame (the end when none is)"""
        gone = np.nonzero(self.live == 0)[0]
        return int(self.c_off[int(gone[0])] if len(gone) else self.c_off[self.n])


def model(comp, c_off, d_off, live):
    """THE RULE -> dict(remap, c_off_out, d_off_out, n_kept, written, dst): dst = the bytes [c_off[0], written) of the destination"""
    c_off, d_off = np.asarray(c_off, np.uint64).astype(np.int64), np.asarray(d_off, np.uint64).astype(np.int64)
    n = len(c_off) - 1
    kept = np.nonzero(np.asarray(live) != 0)[0]
    nk = len(kept)
    remap = np.full(n, REMOVED, np.uint32)
    remap[kept] = np.arange(nk, dtype=np.uint32)
    cs, ds = np.diff(c_off)[kept], np.diff(d_off)[kept]
    c_out = c_off[0] + np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    d_out = d_off[0] + np.concatenate([[0], np.cumsum(ds)]).astype(np.int64)
    total = int(cs.sum())
    src = np.repeat(c_off[kept] - c_out[:-1], cs) + np.arange(int(c_out[0]), int(c_out[0]) + total, dtype=np.int64)
    dst = np.asarray(comp)[src] if total else np.zeros(0, np.uint8)
    return dict(remap=remap, c_off_out=c_out.astype(np.uint64), d_off_out=d_out.astype(np.uint64), n_kept=nk, written=int(c_out[nk]), dst=dst)


def model_loop(comp, c_off, d_off, live):
    """the same in plain Python, frame by frame"""
    n = len(c_off) - 1
    remap, c_out, d_out, dst = [], [int(c_off[0])], [int(d_off[0])], bytearray()
    for s in range(n):
        if not live[s]:
            remap.append(REMOVED)
            continue
        remap.append(len(c_out) - 1)
        a, b = int(c_off[s]), int(c_off[s + 1])
        dst += bytes(comp[a:b])
        c_out.append(c_out[-1] + b - a)
        d_out.append(d_out[-1] + int(d_off[s + 1]) - int(d_off[s]))
    return dict(remap=np.array(remap, np.uint32), c_off_out=np.array(c_out, np.uint64), d_off_out=np.array(d_out, np.uint64), n_kept=len(c_out) - 1,
                written=c_out[-1], dst=np.frombuffer(bytes(dst), np.uint8))


_CASES = None


def cases():
    """{name: Case}"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    # every edge size twice, once kept and once removed, shuffled
    rng = np.random.default_rng(53)
    sizes = np.array(list(EDGE_SIZES) * 2)
    live = np.array([1] * len(EDGE_SIZES) + [0] * len(EDGE_SIZES), np.uint8)
    order = rng.permutation(len(sizes))
    out["sizes_edges"] = Case("sizes_edges", sizes[order], live[order])
    out["sizes_edges_base"] = Case("sizes_edges_base", sizes[order][::-1], live[order][::-1], base=4099)       # c_off[0] != 0
    # the live patterns over 400 frames of 0..3000 bytes
    rng = np.random.default_rng(59)
    n = 400
    fs = rng.integers(0, 3001, n)
    fs[rng.integers(0, n, 25)] = 0
    pat = {"all_kept": np.ones(n, np.uint8), "none_kept": np.zeros(n, np.uint8), "alternating": (np.arange(n) & 1).astype(np.uint8)}
    pat["first_removed"] = np.ones(n, np.uint8); pat["first_removed"][0] = 0
    pat["last_removed"] = np.ones(n, np.uint8); pat["last_removed"][n - 1] = 0
    pat["middle_run"] = np.zeros(n, np.uint8); pat["middle_run"][150:230] = 1
    pat["older_half"] = np.zeros(n, np.uint8); pat["older_half"][n // 2:] = 1
    pat["random_10"] = (rng.random(n) >= 0.10).astype(np.uint8)
    pat["random_90"] = (rng.random(n) >= 0.90).astype(np.uint8)
    pat["empty_only"] = (fs == 0).astype(np.uint8)                               # kept runs made only of empty frames: nothing moves
    for name, lv in pat.items():
        out[name] = Case(name, fs, lv)
    # kept runs made only of empty frames, between removed frames that have bytes (and one kept frame with bytes, so that something moves)
    es = np.array([500, 0, 0, 700, 0, 900, 0, 0, 0, 1100, 300, 0])
    out["empty_runs"] = Case("empty_runs", es, np.array([0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1], np.uint8))
    out["all_empty"] = Case("all_empty", np.zeros(9, np.int64), np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], np.uint8), base=5)
    _CASES = out
    return out


PATTERNS = ("all_kept", "none_kept", "alternating", "first_removed", "last_removed", "middle_run", "older_half", "random_10", "random_90", "empty_only", "empty_runs")


# ---------------------------------------------------------------------------------------------- the kernels under the emulator
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(M.SIM, "libzk_compact_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        u64 = C.c_uint64
        l.zkc_sim_step_direct.argtypes = [u64, u64]
        for f, k in ((l.zkc_sim_step_bytes, 1), (l.zkc_sim_nsteps, 2), (l.zkc_sim_step_begin, 2), (l.zkc_sim_step_end, 3), (l.zkc_sim_stage_bytes, 2)):
            f.restype = u64
            f.argtypes = [u64] * k
        l.zkc_sim_move_grid.restype = C.c_uint32
        l.zkc_sim_move_grid.argtypes = [u64]
        l.zkc_sim_tile.restype = C.c_uint32
        l.zk_compact_sim_mark.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
        l.zk_compact_sim_remap_ids.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
        l.zk_compact_sim.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, u64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_uint32), C.POINTER(u64), C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        l.zkx_sim_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        _LIB = l
    return _LIB


def sim(case, in_place, slice_bytes=0, misalign=0, descending=False, c_off=None):
    """the kernels on the case -> dict(rc, remap, c_off_out, d_off_out, n_kept, written, buf, steps, staged); buf: in place the whole buffer,
    out of place the destination's bytes [0, written)"""
    n = case.n
    c_off = case.c_off if c_off is None else np.ascontiguousarray(c_off, dtype=np.uint64)
    c_end = int(c_off[n])
    comp = np.ascontiguousarray(case.comp[:c_end]) if c_end <= case.comp_size else np.concatenate([case.comp, np.zeros(c_end - case.comp_size, np.uint8)])
    remap = np.full(n, 0x5A5A5A5A, np.uint32)
    c_out, d_out = (np.full(n + 1, 0x5A5A5A5A5A5A5A5A, np.uint64) for _ in range(2))
    buf = np.zeros(max(c_end, 1), np.uint8)
    nk, steps, staged, wr = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    rc = lib().zk_compact_sim(comp.ctypes.data, misalign, c_off.ctypes.data, case.d_off.ctypes.data, n, case.live.ctypes.data, int(in_place), slice_bytes, int(descending),
                              remap.ctypes.data, c_out.ctypes.data, d_out.ctypes.data, C.byref(nk), C.byref(wr), buf.ctypes.data, C.byref(steps), C.byref(staged))
    return dict(rc=rc, remap=remap, c_off_out=c_out[:nk.value + 1], d_off_out=d_out[:nk.value + 1], n_kept=nk.value, written=wr.value,
                buf=buf[:c_end] if in_place else buf[:wr.value], steps=steps.value, staged=staged.value)


def first_diff(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return None if bad.size == 0 else (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))

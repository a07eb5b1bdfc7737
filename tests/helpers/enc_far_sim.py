"""TEST INFRASTRUCTURE -- loader of tests/sim/zk_enc_far_sim.cpp (the encoder's far-history kernels of zeekstd_amd/csrc/zk_enc_far.h on the
CPU under the workgroup emulator), the calls into it, the reference out of the CPU twin (oracle/zstd_oracle_enc.c zko_enc_far_debug) and the
rule the two are compared by.  Used by tests/test_sim_enc_far.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import zko

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_enc_far_sim.cpp"), os.path.join(SIM, "hip_wg_emu.h")] + \
       [os.path.join(CSRC, h) for h in ("zk_enc_far.h", "zk_enc_match.h", "zk_enc_sched.h", "zk_enc_plan.h", "zk_enc_device.h", "zk_device.h")]
_LIB = None

# zk_enc_device.h
WINDOW, SEGMENT, DENSE_MIN, LDM_MIN, LDM_MAX_OFF, LDM_NONE = 57280, 256 << 10, 6, 16, (1 << 27) - 1, 0xFFFFFFFF
NBMAX, PLOG, POISON = 32, 13, 0x5A5A5A5A      # (what the output arrays hold before the harness copies into them)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_enc_far_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_enc_far_sim_dense.restype = C.c_int
        l.zk_enc_far_sim_dense.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.zk_enc_far_sim_ldm_frames.restype = C.c_int
        l.zk_enc_far_sim_ldm_frames.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_uint64]
        l.zk_enc_far_sim_ldm_prefix.restype = C.c_int
        l.zk_enc_far_sim_ldm_prefix.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
        l.zk_enc_far_sim_stage_hist.restype = C.c_int
        l.zk_enc_far_sim_stage_hist.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        _LIB = l
    return _LIB


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8)


def frame_sizes(n, frame_size):
    return [min(frame_size, n - o) for o in range(0, n, frame_size)]


def segments(n, frame_size):
    """(first byte in the source, first byte inside its frame, bytes, frame size) of every matcher segment, in plan order"""
    out = []
    for f, fsz in enumerate(frame_sizes(n, frame_size)):
        out += [(f * frame_size + at, at, min(SEGMENT, fsz - at), fsz) for at in range(0, fsz, SEGMENT)]
    return out


# ---------------------------------------------------------------------------------------------- the emulated kernels
def dense(data, frame_size, level, slice_bytes=0, descending=False):
    """-> (cand[n], part[n], poff[nseg, NBMAX + 1]) as the two dense kernels leave them; None when the call has no dense history"""
    src, n = _u8(data), len(data)
    nseg = len(segments(n, frame_size))
    cand, part = np.full(n, POISON, np.uint32), np.full(n, POISON, np.uint32)
    poff = np.full((nseg, NBMAX + 1), POISON, np.uint32)
    rc = lib().zk_enc_far_sim_dense(src.ctypes.data, n, frame_size, level, slice_bytes, int(descending), cand.ctypes.data, part.ctypes.data, poff.ctypes.data)
    if rc == -1:
        return None
    assert rc == nseg, rc                                   # (-2: a write into the slack behind cand / part)
    return cand, part, poff


def ldm_frames(data, frame_size, level, descending=False):
    """-> (tables[nf, 1 << log], log) of zk_k_enc_ldm_build_frames; None when the call has no in-frame far history"""
    src, n = _u8(data), len(data)
    nf = len(frame_sizes(n, frame_size))
    table = np.full(nf << (23 if nf <= 4 else 16), POISON, np.uint32)
    log = lib().zk_enc_far_sim_ldm_frames(src.ctypes.data, n, frame_size, level, int(descending), table.ctypes.data, table.size)
    if log < 0:
        return None
    return table[:nf << log].reshape(nf, 1 << log).copy(), log


def ldm_prefix(prefix, descending=False):
    """-> table[1 << log] of zk_k_enc_ldm_build; None for a prefix the ring holds"""
    p = _u8(prefix)
    table = np.full(1 << 23, POISON, np.uint32)
    log = lib().zk_enc_far_sim_ldm_prefix(p.ctypes.data, len(prefix), int(descending), table.ctypes.data, table.size)
    return None if log < 0 else table[:1 << log].copy()


def stage_hist(data, frame_size, level, prefix):
    """-> (the matcher's [prefix tail | frame] records, nf * (hist + frame_size) bytes with 0xA5 where no record byte lies, hist)"""
    src, p, n = _u8(data), _u8(prefix), len(data)
    nf = max(1, len(frame_sizes(n, frame_size)))
    stage = np.zeros(nf * (WINDOW + frame_size), np.uint8)
    hist = lib().zk_enc_far_sim_stage_hist(src.ctypes.data, n, frame_size, level, p.ctypes.data, len(prefix), stage.ctypes.data, stage.size)
    assert hist >= 0
    return stage[:nf * (hist + frame_size)].tobytes(), hist


# ---------------------------------------------------------------------------------------------- the reference
def reference(data, frame_size, level, dense_triples=True):
    """the twin's far history frame by frame: [(sampled table or None, (d, l, bk) per position [fsz, 3] or None, dense on)]"""
    return [zko.enc_far_debug(data[o:o + frame_size], level, dense_triples) for o in range(0, len(data), frame_size)]


def hash5(frame, dlog):
    """zke_hash of every position q with q + 8 <= len(frame) (two 24-bit multiplies, zk_enc_device.h)"""
    b = np.frombuffer(bytes(frame), np.uint8).astype(np.uint32)
    m = len(b) - 7
    if m <= 0:
        return np.zeros(0, np.uint32)
    a = b[0:m] | (b[1:m + 1] << 8) | (b[2:m + 2] << 16)
    c = b[3:m + 3] | (b[4:m + 4] << 8)
    return ((a * np.uint32(0x9E3779) + c * np.uint32(0x85EBCB)) & np.uint32(0xFFFFFFFF)) >> np.uint32(32 - dlog)


def is_run(frame):
    """per position q with q + 8 <= len(frame): its four bytes are one byte"""
    b = np.frombuffer(bytes(frame), np.uint8)
    m = len(b) - 7
    if m <= 0:
        return np.zeros(0, bool)
    return (b[1:m + 1] == b[0:m]) & (b[2:m + 2] == b[0:m]) & (b[3:m + 3] == b[0:m])


def compare_dense(data, frame_size, level, got, refs):
    """The rule (what zk_k_enc_dense_part / zk_k_enc_dense_cand must leave, against the twin's triples):
      cand   an entry where the twin has one and nowhere else -- every other position reads 0, not stale scratch; distance and catch-up
             equal; the length compared as min(kernel's, frame end - position): the kernel reads zeros behind the frame's last byte and
             the match kernel caps the length later
      part   per segment and pass, as a SET, exactly the positions of the segment that are no byte run, have q + 8 <= frame size and whose
             slot >> 13 is the pass, each with its slot's low 13 bits; poff non-decreasing, ending at the total"""
    cand, part, poff = got
    n = len(data)
    dlog = 18 if level >= 9 else 17
    nb = 1 << (dlog - PLOG)
    for f, o in enumerate(range(0, n, frame_size)):
        frame = data[o:o + frame_size]
        fsz = len(frame)
        dlb = refs[f][1]
        c = cand[o:o + fsz]
        if dlb is None:                                     # a frame within the ring's reach in a call with dense history: no candidates
            assert not c.any(), (f, int(np.nonzero(c)[0][0]))
            continue
        d, l, bk = dlb[:, 0], dlb[:, 1], dlb[:, 2]
        q = np.arange(fsz, dtype=np.int64)
        kl = np.minimum(c & 31, fsz - q).astype(np.uint32)
        want = np.where(d > 0, l | (bk << 5) | (d << 8), 0).astype(np.uint32)
        have = np.where(c > 0, kl | (c & ~np.uint32(31)), 0).astype(np.uint32)
        bad = np.nonzero(want != have)[0]
        assert bad.size == 0, (f, int(bad[0]), "kernel (l, bk, d)", (int(c[bad[0]] & 31), int(c[bad[0]] >> 5 & 7), int(c[bad[0]] >> 8)),
                               "twin (d, l, bk)", dlb[bad[0]].tolist(), bad.size)
    row = 0
    for o, at, sz, fsz in segments(n, frame_size):
        f0 = o - at
        h = hash5(data[f0:f0 + fsz], dlog)
        run = is_run(data[f0:f0 + fsz])
        qs = np.arange(at, min(at + sz, len(h)), dtype=np.int64) if len(h) > at else np.zeros(0, np.int64)
        qs = qs[~run[qs]]
        po = poff[row, :nb + 1].astype(np.int64)
        assert po[0] == 0 and (np.diff(po) >= 0).all() and po[nb] == len(qs), (row, po.tolist(), len(qs))
        lst = part[o:o + int(po[nb])]
        ent = (((qs - at) << PLOG) | (h[qs] & ((1 << PLOG) - 1))).astype(np.uint32)
        hp = h[qs] >> PLOG
        for p in range(nb):
            g = np.sort(lst[po[p]:po[p + 1]])
            w = np.sort(ent[hp == p])
            assert len(g) == len(w) and (g == w).all(), (row, p, len(g), len(w))
        row += 1


def served_by(dlb):
    """of the twin's entries of one frame: how many lie in the position's own segment (the `first` table), how many in the segment before (`last`)"""
    q = np.nonzero(dlb[:, 0])[0]
    c = q - dlb[q, 0]
    own = (c // SEGMENT) == (q // SEGMENT)
    return int(own.sum()), int((~own).sum())

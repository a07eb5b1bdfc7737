"""The plan of an encode over a caller-given frame list (zk_encode_frame_list*), on the CPU: zke_plan_fill_list against zke_plan_fill, the
plan kernels of zk_enc_plan_dev.h against zke_plan_fill_list, the host pipeline's chunks, and the list forms of the far-history kernels and
the match kernel against the CPU twin frame by frame -- all through tests/sim/zk_enc_plan_list_sim.cpp (the sources hipcc compiles, under
the workgroup emulator); tests/sim/enc_plan_list_san.cpp runs the kernels under AddressSanitizer + UBSan as a program of its own."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import enc_list_inputs as E
from oracle import zko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_enc_plan_list_sim.cpp"), os.path.join(SIM, "hip_wg_emu.h"), os.path.join(SIM, "zk_enc_match_emu.h")] + \
       [os.path.join(CSRC, h) for h in ("zk_enc_plan_dev.h", "zk_enc_plan.h", "zk_enc_sched.h", "zk_enc_far.h", "zk_enc_match.h", "zk_enc_match2.h", "zk_enc_device.h", "zk_device.h")]
WINDOW, SEGMENT, LDM_NONE = E.WINDOW, E.SEGMENT, 0xFFFFFFFF
_LIB = None
P = C.c_void_p


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_enc_plan_list_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_plan_list_sim_equal.restype = C.c_int
        l.zk_plan_list_sim_equal.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64]
        l.zk_plan_list_sim_dev.restype = C.c_int
        l.zk_plan_list_sim_dev.argtypes = [P, C.c_uint32, C.c_int, C.c_uint64, C.c_int]
        l.zk_plan_list_sim_chunks.restype = C.c_int
        l.zk_plan_list_sim_chunks.argtypes = [P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, P, C.c_uint32]
        l.zk_plan_list_sim_encode.restype = C.c_int
        l.zk_plan_list_sim_encode.argtypes = [P, P, C.c_uint32, C.c_int, C.c_uint64, C.c_int, C.c_int, P, C.c_uint32, P, P, C.c_uint64, P,
                                              C.c_uint32, P, P, P, P, P, P, C.c_uint64, P, C.c_uint64]
        _LIB = l
    return _LIB


# ---------------------------------------------------------------------------------------------- host plan
@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("prefix_len", [0, 3, 1000, 200000])
def test_equal_sizes_give_the_uniform_plan(level, prefix_len):
    """frames, blocks, segments, offsets and totals by memcmp; a short tail, n = 0, a frame of one byte, frames above a segment"""
    for n, fs in ((0, 1024), (1, 1), (10, 1), (4096 * 3, 4096), (4097 * 3 - 5, 4097), (100000, 30000), (57281 * 2 + 1, 57281),
                  (600001, 262145), (700000, 700000), (5000, 1 << 30)):
        for base in (0, 12345):
            assert lib().zk_plan_list_sim_equal(n, fs, level, prefix_len, base) == 0, (n, fs, base)


def _lists():
    out = [("edge", E.edge_list()[1]), ("edge+lead", E.edge_list(lead=777)[1])]
    for seed in (1, 2):
        out.append(("small%d" % seed, E.small_list(seed, count=3000, hi=5000)[1]))
    out.append(("one empty", np.array([9, 9], np.uint64)))
    out.append(("empty run", np.array([0, 0, 0, 0, 5, 5], np.uint64)))
    out.append(("one large", np.array([0, 3 * SEGMENT + 17], np.uint64)))
    out.append(("1025 frames", np.arange(0, 1026 * 100, 100, dtype=np.uint64)))            # one more than the scan's lanes
    return out


@pytest.mark.parametrize("descending", [False, True])
def test_plan_kernels_equal_the_host_plan(descending):
    """zk_k_enc_plan_scan + zk_k_enc_plan_fill under the emulator, both lane orders: every ZkEncFrame, ZkEncBlock, segment record, offset and
    total is zke_plan_fill_list's"""
    for name, off in _lists():
        off = np.ascontiguousarray(off, np.uint64)
        for level, plen in ((1, 0), (3, 0), (3, 1000), (2, 200000)):
            assert lib().zk_plan_list_sim_dev(off.ctypes.data, len(off) - 1, level, plen, int(descending)) == 0, (name, level, plen)


def test_host_pipeline_chunks_are_whole_frames_to_the_targets():
    rng = np.random.default_rng(4)
    for trial in range(30):
        count = int(rng.integers(1, 400))
        sizes = rng.integers(0, 900, count).astype(np.uint64)
        if trial % 3 == 0:
            sizes[rng.integers(0, count)] = 5000                                            # a frame above the most a chunk may hold
        off = np.concatenate([[7], 7 + np.cumsum(sizes)]).astype(np.uint64)
        min_bytes, min_frames, max_bytes = 4000, 8, 12000
        cuts = np.zeros(count + 2, np.uint32)
        k = lib().zk_plan_list_sim_chunks(off.ctypes.data, count, min_bytes, min_frames, max_bytes, cuts.ctypes.data, len(cuts))
        assert k >= 1 and cuts[0] == 0 and cuts[k] == count and (np.diff(cuts[:k + 1].astype(np.int64)) > 0).all()
        for i in range(k):
            f0, f1 = int(cuts[i]), int(cuts[i + 1])
            b = int(off[f1] - off[f0])
            assert b <= max_bytes or f1 - f0 == 1, (trial, i, b)
            if i + 1 < k:                                                                   # every chunk but the last met the targets, or the next frame did not fit
                assert (b >= min_bytes and f1 - f0 >= min_frames) or int(off[f1 + 1] - off[f0]) > max_bytes, (trial, i, b, f1 - f0)


# ---------------------------------------------------------------------------------------------- far history and match under a list
def encode_sim(data, off, level, slice_bytes=0, descending=False, with_match=True):
    off = np.ascontiguousarray(off, np.uint64)
    count = len(off) - 1
    n = int(off[-1] - off[0])
    src = np.frombuffer(bytes(data) + b"\0" * 8, np.uint8)
    lf = np.zeros(3 * count, np.uint64)
    nlf = C.c_uint32()
    table = np.zeros(1 << 20, np.uint32)
    cand = np.full(max(n, 1), 0x5A5A5A5A, np.uint32)
    cap = n // 1024 + 64 * count + 64
    nseq, nlit, bsz = (np.zeros(cap, np.uint32) for _ in range(3))
    seq_at, lit_at = (np.zeros(cap, np.uint64) for _ in range(2))
    seqs = np.zeros(n // 4 + 2 * cap + 64, np.uint64)
    lits = np.zeros(n + 64, np.uint8)
    nb = lib().zk_plan_list_sim_encode(src.ctypes.data, off.ctypes.data, count, level, slice_bytes, int(descending), int(with_match),
                                       lf.ctypes.data, count, C.byref(nlf), table.ctypes.data, table.size, cand.ctypes.data,
                                       cap, nseq.ctypes.data, nlit.ctypes.data, bsz.ctypes.data, seq_at.ctypes.data, lit_at.ctypes.data,
                                       seqs.ctypes.data, len(seqs), lits.ctypes.data, len(lits))
    assert nb >= 0, nb
    blocks = [(seqs[int(seq_at[b]):int(seq_at[b]) + int(nseq[b])].copy(), lits[int(lit_at[b]):int(lit_at[b]) + int(nlit[b])].tobytes(), int(bsz[b]))
              for b in range(nb)] if with_match else None
    return lf[:3 * nlf.value].reshape(-1, 3), table, cand[:n], blocks


def compare_with_twin(data, off, level, got):
    """per frame: the sampled table of a frame beyond the window is the twin's (and only such frames have one); every position's dense
    candidate is the twin's (tests/helpers/enc_far_sim.py compare_dense has the rule for the length); the blocks' sequences and literals
    are the twin's matcher's for that frame alone"""
    lf, table, cand, blocks = got
    frames = E.frames_of(data, off)
    base = int(off[0])
    want_lf = [(int(off[i]) - base, len(f)) for i, f in enumerate(frames) if len(f) > WINDOW and level >= 2]
    assert [(int(a), int(c)) for a, _, c in lf] == want_lf
    by_start = {int(a): int(t) for a, t, _ in lf}
    bi = 0
    for i, f in enumerate(frames):
        o = int(off[i]) - base
        ttab, dlb, dense_on = zko.enc_far_debug(f, level, True)
        if o in by_start and len(f):
            assert ttab is not None
            assert (table[by_start[o]:by_start[o] + len(ttab)] == ttab).all(), (i, len(f))
        else:
            assert ttab is None or len(f) <= WINDOW
        c = cand[o:o + len(f)]
        if dlb is None or not dense_on:
            assert not c.any(), (i, len(f))
        else:
            d, l, bk = dlb[:, 0], dlb[:, 1], dlb[:, 2]
            q = np.arange(len(f), dtype=np.int64)
            kl = np.minimum(c & 31, len(f) - q).astype(np.uint32)
            want = np.where(d > 0, l | (bk << 5) | (d << 8), 0).astype(np.uint32)
            have = np.where(c > 0, kl | (c & ~np.uint32(31)), 0).astype(np.uint32)
            bad = np.nonzero(want != have)[0]
            assert bad.size == 0, (i, len(f), int(bad[0]), bad.size)
        if blocks is not None:
            for ws, wl in zko.enc_match_debug(f, level) if len(f) else []:
                gs, gl, bsz = blocks[bi]; bi += 1
                assert len(gs) == len(ws) and (gs == ws).all() and gl == wl, (i, len(f), bi)
                assert sum((int(x) >> 16) & 0xFFFF for x in gs) + len(gl) == bsz
    if blocks is not None:
        assert bi == len(blocks)
    assert (table[:1 << 12] == LDM_NONE).all() or not len(lf)                               # the shared empty table stays empty


@pytest.mark.parametrize("level", [2, 3])
def test_far_history_and_match_under_a_list_equal_the_twin(level):
    data, off = E.edge_list()
    compare_with_twin(data, off, level, encode_sim(data, off, level))


def test_slices_and_lane_order_do_not_change_the_candidates():
    """dense scratch of 64 KiB (every frame beyond the window exceeds a slice: never less than a frame) and descending lanes"""
    data, off = E.edge_list(lead=5)
    compare_with_twin(data, off, 3, encode_sim(data, off, 3, slice_bytes=64 << 10, descending=True, with_match=False))


# ---------------------------------------------------------------------------------------------- sanitizers
def test_plan_and_far_kernels_under_sanitizers(tmp_path):
    """tests/sim/enc_plan_list_san.cpp, a program of its own built with -fsanitize=address,undefined: the plan kernels and the list forms of
    the far kernels on the edge list and on lists that end in a frame of fewer than 8 bytes"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "listsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(SIM, "enc_plan_list_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    data, off = E.edge_list()
    runs = [(data, off, 3, 0), (data, off, 9, 64 << 10)]
    text = zko.gen_text(70000 + 7, 5)
    for tail in (1, 7):
        runs.append((text[:70000 + tail], np.array([0, 0, 70000, 70000, 70000 + tail], np.uint64), 3, 0))
        runs.append((text[:60 + tail], np.array([0, 60, 60 + tail], np.uint64), 3, 0))
    first = True
    for i, (d, o, level, sl) in enumerate(runs):
        dp, op = str(tmp_path / f"d{i}"), str(tmp_path / f"o{i}")
        with open(dp, "wb") as f:
            f.write(d)
        with open(op, "wb") as f:
            f.write(np.ascontiguousarray(o, np.uint64).tobytes())
        r = subprocess.run([exe, dp, op, str(level), str(sl)], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (i, r.stdout[-300:], r.stderr[-3000:])

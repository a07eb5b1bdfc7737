"""The kernels that remove frames from an archive (zeekstd_amd/csrc/zk_compact.h -- the source hipcc compiles for gfx950: zk_k_cmp_check_ids,
_mark, _flags, _emit, _step_gaps, _move, _remap_ids, _remap_flags, _remap_check, _take) executed on the CPU by tests/sim/zk_compact_sim.cpp
under the workgroup emulator, with the launchers' grids and the plan functions' steps, in both lane orders, out of place and in place with
slices of 1 KiB, 64 KiB and the default, and compared entry by entry and byte by byte with the numpy model of
tests/helpers/compact_model.py.  The plan functions against literal expectations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import compact_model as K
from helpers import dedup_against_model as A

CASES = K.cases()
ORDERS = [(0, False), (3, True)]                 # (misalign, descending order of lanes and workgroups)
SLICES = (1 << 10, 64 << 10, 0)
TILE = 64 << 10


def check(c, got, in_place, what):
    m = c.model()
    assert got["rc"] == 0, (what, got["rc"])
    assert got["n_kept"] == m["n_kept"] and got["written"] == m["written"], (what, got["n_kept"], got["written"])
    for key in ("remap", "c_off_out", "d_off_out"):
        assert len(got[key]) == len(m[key]) and K.first_diff(got[key], m[key]) is None, (what, key, K.first_diff(got[key], m[key]))
    base = int(c.c_off[0])
    if in_place:
        bad = K.first_diff(got["buf"], c.expect_in_place()[:len(got["buf"])])
    else:
        bad = K.first_diff(got["buf"][base:], m["dst"])
    assert bad is None, (what, bad)


@pytest.mark.parametrize("name", list(CASES))
def test_out_of_place_equals_the_model(name):
    c = CASES[name]
    for misalign, descending in ORDERS:
        check(c, K.sim(c, False, 0, misalign, descending), False, (name, misalign))
    for misalign in (1, 7):
        check(c, K.sim(c, False, 0, misalign, False), False, (name, misalign))


@pytest.mark.parametrize("name", list(CASES))
def test_in_place_equals_the_model_under_every_slice(name):
    c = CASES[name]
    m = c.model()
    moved = m["written"] - c.first_removed()
    for slice_bytes in SLICES:
        for misalign, descending in ORDERS:
            got = K.sim(c, True, slice_bytes, misalign, descending)
            check(c, got, True, (name, slice_bytes, misalign))
            step = TILE if slice_bytes else 256 << 20
            assert got["steps"] == (max(moved, 0) + step - 1) // step if m["n_kept"] else got["steps"] == 0, (name, slice_bytes, got["steps"])


def expected_staged(c, step):
    """the steps of an in-place compaction that must go through scratch, from the model alone: the gap src - dst at a step's first byte (the
    bytes removed before it) is below the step's length"""
    m = c.model()
    kept = np.nonzero(c.live)[0]
    lo, hi = c.first_removed(), m["written"]
    ends = m["c_off_out"][1:].astype(np.int64)
    staged, steps = 0, 0
    for a in range(lo, hi, step):
        k = int(np.searchsorted(ends, a, side="right"))          # the kept frame that holds destination byte a
        gap = int(c.c_off[kept[k]]) - int(m["c_off_out"][k])
        staged += gap < min(step, hi - a)
        steps += 1
    return steps, staged


def test_steps_are_direct_and_staged():
    """one-tile steps: which go source -> destination directly and which through scratch is what the model's gaps say, and the cases take both
    kinds; with the older half removed the gap is half the archive and every step is direct; one step of the default 256 MiB is staged"""
    kinds = set()
    for name in ("sizes_edges", "sizes_edges_base", "alternating", "random_10", "random_90", "first_removed", "older_half", "middle_run"):
        got = K.sim(CASES[name], True, 1 << 10)
        assert (got["steps"], got["staged"]) == expected_staged(CASES[name], TILE), name
        kinds |= {"staged"} if got["staged"] else set()
        kinds |= {"direct"} if got["staged"] < got["steps"] else set()
        kinds |= {"both"} if 0 < got["staged"] < got["steps"] else set()
    assert kinds == {"staged", "direct", "both"}
    h = K.sim(CASES["older_half"], True, 1 << 10)
    assert h["steps"] > 3 and h["staged"] == 0
    d = K.sim(CASES["alternating"], True, 0)
    assert d["steps"] == 1 and d["staged"] == 1


def test_plan_functions_literal():
    l = K.lib()
    assert l.zkc_sim_tile() == TILE == K.TILE
    # direct / staged at gap = step - 1, step, step + 1
    for step in (1, TILE, 5 * TILE + 17):
        assert l.zkc_sim_step_direct(step - 1, step) == 0
        assert l.zkc_sim_step_direct(step, step) == 1
        assert l.zkc_sim_step_direct(step + 1, step) == 1
    assert l.zkc_sim_step_direct(0, 0) == 1 and l.zkc_sim_step_direct(0, 1) == 0
    # bytes per step: whole tiles, one at least; 0 = 256 MiB
    assert [l.zkc_sim_step_bytes(s) for s in (0, 1, 1 << 10, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 1 << 32)] == \
        [256 << 20, TILE, TILE, TILE, TILE, TILE, 3 * TILE, 1 << 32]
    # the step boundaries for 0, 1, tile - 1, tile and tile + 1 bytes, in steps of one tile
    want = {0: [], 1: [(0, 1)], TILE - 1: [(0, TILE - 1)], TILE: [(0, TILE)], TILE + 1: [(0, TILE), (TILE, TILE + 1)]}
    for moved, steps in want.items():
        n = l.zkc_sim_nsteps(moved, TILE)
        assert [(l.zkc_sim_step_begin(k, TILE), l.zkc_sim_step_end(k, TILE, moved)) for k in range(n)] == steps, moved
    assert l.zkc_sim_nsteps(5 * TILE + 1, 2 * TILE) == 3 and l.zkc_sim_step_end(2, 2 * TILE, 5 * TILE + 1) == 5 * TILE + 1
    # the scratch: the longest step; the grid: a workgroup per tile up to 65 536
    assert [l.zkc_sim_stage_bytes(m, 2 * TILE) for m in (0, 1, 2 * TILE, 2 * TILE + 1)] == [0, 1, 2 * TILE, 2 * TILE]
    assert [l.zkc_sim_move_grid(b) for b in (0, 1, TILE, TILE + 1, 65536 * TILE, 65536 * TILE + 1, 1 << 40)] == [1, 1, 1, 2, 65536, 65536, 65536]


def test_offsets_that_decrease_or_pass_the_end_are_refused():
    c = CASES["alternating"]
    bad = c.c_off.copy()
    bad[200], bad[201] = bad[201], bad[200] + 0
    assert bad[201] < bad[200] or bad[200] == bad[201]
    bad[200] += 1
    got = K.sim(c, False, c_off=bad)
    assert got["rc"] == -100 and got["n_kept"] == 0


def test_mark_and_remap_ids():
    l = K.lib()
    n = 300
    for descending in (0, 1):
        live = np.zeros(n, np.uint8)
        a = np.array([5, 7, 7, 299, 0, 5], np.uint32)
        b = np.array([8, 7, 100], np.uint32)
        assert l.zk_compact_sim_mark(a.ctypes.data, len(a), n, live.ctypes.data, descending) == 0
        assert l.zk_compact_sim_mark(b.ctypes.data, len(b), n, live.ctypes.data, descending) == 0           # marks accumulate
        assert np.nonzero(live)[0].tolist() == [0, 5, 7, 8, 100, 299] and set(live.tolist()) == {0, 1}
        before = live.copy()
        bad = np.array([3, n, 4], np.uint32)
        assert l.zk_compact_sim_mark(bad.ctypes.data, 3, n, live.ctypes.data, descending) == -100
        assert (live == before).all()                                                                      # checked first, then written
        remap = np.full(n, K.REMOVED, np.uint32)
        remap[np.nonzero(live)[0]] = np.arange(6)
        ids = np.array([299, 0, 7, 7, 100], np.uint32)
        out = np.full(5, 0x5A5A5A5A, np.uint32)
        assert l.zk_compact_sim_remap_ids(remap.ctypes.data, n, ids.ctypes.data, 5, out.ctypes.data, descending) == 0
        assert out.tolist() == [5, 0, 2, 2, 4]
        for wrong in ([0, 6, 5], [0, n, 5], [0xFFFFFFFF]):
            w = np.array(wrong, np.uint32)
            out = np.full(len(w), 0x5A5A5A5A, np.uint32)
            assert l.zk_compact_sim_remap_ids(remap.ctypes.data, n, w.ctypes.data, len(w), out.ctypes.data, descending) == -100
            assert (out == 0x5A5A5A5A).all()


@pytest.mark.parametrize("bits", A.KEY_BITS)
def test_the_index_compacted_is_the_index_of_the_kept_frames(bits):
    """an index of the archive the generations leave, compacted with the remap of a live pattern: its export, its table and its answers are
    those of an index built by add from the kept frames"""
    gens = A.generations()["mix"]
    archive = []
    for c in gens:
        archive += [c.frames[int(j)] for j in A.model(archive, c.frames)[1]]
    n = len(archive)
    keys, lens = A.frame_keys(archive), np.array([len(f) for f in archive], np.uint32)
    rng = np.random.default_rng(5)
    for descending, live in ((False, rng.random(n) < 0.5), (True, np.arange(n) % 3 != 0), (False, np.zeros(n, bool)), (True, np.ones(n, bool))):
        kept = np.nonzero(live)[0]
        remap = np.full(n, K.REMOVED, np.uint32)
        remap[kept] = np.arange(len(kept))
        x = A.SimIndex(bits)
        x.add(keys, lens, descending)
        # refused: another count, a remap that is not a compaction's -- the index stays
        assert K.lib().zkx_sim_compact(x._h, remap.ctypes.data, n - 1, int(descending)) == -100
        if len(kept) > 1:
            twisted = remap.copy()
            twisted[kept[0]], twisted[kept[1]] = twisted[kept[1]], twisted[kept[0]]
            assert K.lib().zkx_sim_compact(x._h, twisted.ctypes.data, n, int(descending)) == -100
        assert x.count == n and x.table_ok()
        assert K.lib().zkx_sim_compact(x._h, remap.ctypes.data, n, int(descending)) == 0
        y = A.SimIndex(bits)
        y.add(keys[kept], lens[kept], descending)
        assert x.count == len(kept) == y.count and x.slots == y.slots and x.table_ok()
        k, m = x.export()
        assert (k == keys[kept]).all() and (m == lens[kept]).all()
        kept_frames = [archive[int(s)] for s in kept]
        probe = gens[2]
        want = A.model(kept_frames, probe.frames)
        for idx in (x, y):
            got = idx.against(kept_frames, probe, None, bits, 1, descending)
            assert (got["ids"] == want[0]).all() and (got["fresh"] == want[1]).all()
        x.close()
        y.close()


def test_kernels_under_sanitizers(tmp_path):
    """The same harness as a program of its own under AddressSanitizer + UBSan (tests/sim/compact_san.cpp): exact-size heap allocations for
    the source, the destination, a staged step and every array of the scratch"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from conftest import ROOT
    exe = str(tmp_path / "cmpsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "compact_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    first = True
    for i, (name, misalign, slice_bytes) in enumerate([("sizes_edges", 0, 1024), ("sizes_edges_base", 3, 0), ("alternating", 1, 1024), ("random_90", 7, 65536),
                                                       ("empty_runs", 1, 1024), ("none_kept", 0, 0), ("all_kept", 5, 1024)]):
        c = CASES[name]
        paths = [str(tmp_path / ("%s%d" % (k, i))) for k in ("comp", "coff", "doff", "live")]
        for p, a in zip(paths, (c.comp, c.c_off, c.d_off, c.live)):
            with open(p, "wb") as f:
                f.write(a.tobytes())
        r = subprocess.run([exe, str(misalign), str(slice_bytes), *paths], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (name, r.stdout[-300:], r.stderr[-3000:])
        m = c.model()
        h = 0xCBF29CE484222325
        for b in m["remap"].tobytes() + m["c_off_out"].tobytes() + m["d_off_out"].tobytes() + m["dst"].tobytes():
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        out = r.stdout.split()
        assert out == [str(m["n_kept"]), str(m["written"]), "%016x" % h, "%016x" % h], (name, r.stdout)

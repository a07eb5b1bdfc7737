"""The kernels of the dedup index (zeekstd_amd/csrc/zk_dedup_index.h -- the source hipcc compiles for gfx950: zk_k_dxi_insert, _take, _lookup,
_compare, _flags, _emit) executed on the CPU by tests/sim/zk_dedup_index_sim.cpp under the workgroup emulator, with the launchers' grids,
the rounds, the passes and the scratch layout of zk_dedup_index.hip -- the harness hands over the candidates' decoded bytes in place of the
decode --, and compared entry by entry with the model of tests/helpers/dedup_against_model.py (a dict from bytes to the smallest archive id,
then the in-call dict) on the generations the GPU tests share: in both lane orders, under key bits 0, 4 and 1 and with the all-zero hash."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import dedup_against_model as A
from helpers import dedup_model as M

GENS = A.generations()
CASES = M.cases()
ORDERS = [(0, False), (3, True)]                 # (misalign, descending order of lanes and workgroups)


def check(got, want, what):
    ids, fresh = want
    assert len(got["fresh"]) == len(fresh), (what, len(got["fresh"]), len(fresh))
    for name, w in (("ids", ids), ("fresh", fresh)):
        bad = np.nonzero(got[name] != w)[0]
        assert bad.size == 0, (what, name, int(bad[0]), int(got[name][bad[0]]), int(w[bad[0]]))


def append_all(gens, bits, zero_hash=False, misalign=0, descending=False, pass_bytes=0, archive=None, index=None):
    """every generation against the archive so far, then appended: ids and fresh equal the model's, the index grows by the fresh frames"""
    x = index or A.SimIndex(bits)
    archive = list(archive or [])
    rounds = 0
    for c in gens:
        want = A.model(archive, c.frames)
        got = x.against(archive, c, np.zeros(c.count, np.uint64) if zero_hash else None, bits, misalign, descending, pass_bytes, take=True)
        check(got, want, (c.name, bits, zero_hash, descending))
        archive += [c.frames[int(j)] for j in want[1]]
        assert x.count == len(archive) and x.table_ok(), c.name
        if pass_bytes:
            assert got["largest_pass"] <= max(pass_bytes, max(len(f) for f in c.frames))
        rounds = max(rounds, got["rounds"])
    return x, archive, rounds


@pytest.mark.parametrize("bits", A.KEY_BITS)
@pytest.mark.parametrize("name", list(GENS))
def test_ids_and_fresh_equal_the_model(name, bits):
    for (misalign, descending) in (ORDERS if name != "edges" else ORDERS[bits & 1:][:1]):
        x, archive, rounds = append_all(GENS[name], bits, False, misalign, descending)
        if not bits:
            # the keys the index took from the hash pass are the frame keys of the model
            keys, lens = x.export()
            assert (keys == A.frame_keys(archive)).all() and lens.tolist() == [len(f) for f in archive]
        if name == "near" and bits:
            assert rounds > 2                                      # what the short keys are for: several candidates per frame, in turn
        x.close()


@pytest.mark.parametrize("name", ["mix", "near"])
def test_any_key_gives_the_rule(name):
    """every frame the key 0: the length alone tells candidates apart, and equal lengths are tried one after the other, ascending"""
    for bits, (misalign, descending) in zip((0, 4), ORDERS):
        x, _, rounds = append_all(GENS[name], bits, True, misalign, descending)
        assert rounds > 1
        x.close()


def test_an_empty_archive_gives_the_in_call_map():
    for name in ("enc_mix", "far_pairs", "all_empty", "one_empty", "all_same_long"):
        c = CASES[name]
        ref, uniq, ids = c.model()
        x = A.SimIndex(0)
        for misalign, descending in ORDERS:
            got = x.against([], c, None, 4, misalign, descending)
            assert (got["ids"] == ids).all() and (got["fresh"] == uniq).all(), name
            assert got["passes"] == 0
        x.close()


def test_an_archive_that_holds_every_frame():
    c = CASES["far_pairs"]
    x, archive, _ = append_all([c], 0)
    got = x.against(archive, M.Case("again", list(reversed(c.frames)), lead=1), None, 0, 1, True)
    assert len(got["fresh"]) == 0 and got["rounds"] == 1
    check(got, A.model(archive, list(reversed(c.frames))), "held")
    x.close()


@pytest.mark.parametrize("bits", A.KEY_BITS)
def test_an_archive_with_duplicates_the_smallest_wins(bits):
    archive, c = A.dup_archive()
    want = A.model(archive, c.frames)
    assert len(set(archive)) < len(archive) and want[0].min() == 0
    for zero in (False, True):
        for misalign, descending in ORDERS:
            x = A.SimIndex(bits)
            x.add(np.zeros(len(archive), np.uint64) if zero else A.frame_keys(archive), [len(f) for f in archive], descending)
            check(x.against(archive, c, np.zeros(c.count, np.uint64) if zero else None, bits, misalign, descending), want, (bits, zero, descending))
            x.close()


def test_rebuilds_truncate_and_export():
    """33 then 40 more frames into a fresh index: lookups before and after the 64 -> 128 -> 256 slot rebuilds; truncate back and add again;
    export -> a new index -> the same answers"""
    frames = CASES["all_distinct"].frames
    probe = M.Case("probe", frames[:80] + frames[10:20] + [b"", frames[79][:-1]], lead=3)
    keys, lens = A.frame_keys(frames), [len(f) for f in frames]
    for descending in (False, True):
        x = A.SimIndex(0)
        assert x.slots == 64 and x.count == 0
        check(x.against([], probe, descending=descending), A.model([], probe.frames), 0)
        x.add(keys[:33], lens[:33], descending)
        assert x.slots == 128 and x.table_ok()
        check(x.against(frames[:33], probe, descending=descending), A.model(frames[:33], probe.frames), 33)
        x.add(keys[33:73], lens[33:73], descending)
        assert x.slots == 256 and x.count == 73 and x.table_ok()
        check(x.against(frames[:73], probe, descending=descending), A.model(frames[:73], probe.frames), 73)
        # an archive longer than the index: frames at or beyond m are not looked at
        check(x.against(frames[:80], probe, descending=descending), A.model(frames[:73], probe.frames), "beyond m")
        x.truncate(40, descending)
        assert x.count == 40 and x.slots == 128 and x.table_ok()
        check(x.against(frames[:40], probe, descending=descending), A.model(frames[:40], probe.frames), 40)
        other = list(reversed(frames[100:130]))
        x.add(A.frame_keys(other), [len(f) for f in other], descending)
        archive = frames[:40] + other
        again = M.Case("again", probe.frames + other[5:9], lead=1)
        want = A.model(archive, again.frames)
        check(x.against(archive, again, descending=descending), want, "truncated and grown")
        k, n = x.export()
        assert (k == A.frame_keys(archive)).all() and n.tolist() == [len(f) for f in archive]
        y = A.SimIndex(0)
        y.add(k, n, not descending)
        assert y.slots == x.slots and y.table_ok()
        check(y.against(archive, again, descending=descending), want, "exported")
        x.close()
        y.close()


def test_the_pass_cut():
    """passes of 1 KiB: a candidate longer than the pass is a pass of its own, the others share passes of at most 1 KiB; the same answers"""
    x, archive, _ = append_all(GENS["mix"][:1], 0)
    c = GENS["mix"][1]
    want = A.model(archive, c.frames)
    one = x.against(archive, c)
    cut = x.against(archive, c, pass_bytes=A.PASS_1K, misalign=1, descending=True)
    check(one, want, "one pass")
    check(cut, want, "1 KiB")
    assert one["passes"] == 1 and cut["passes"] > 2 and cut["largest_pass"] > A.PASS_1K
    x.close()
    for bits in (4, 1):
        x, _, _ = append_all(GENS["near"], bits, False, 1, True, A.PASS_1K)
        x.close()


def test_kernels_under_sanitizers(tmp_path):
    """The same harness as a program of its own under AddressSanitizer + UBSan (tests/sim/dedup_index_san.cpp): the source ends with its
    allocation, a pass's decoded candidates are an allocation of exactly their bytes, the index's arrays of exactly its frames"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from conftest import ROOT
    exe = str(tmp_path / "dxisan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "dedup_index_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    first = True
    for i, (name, bits, zero, misalign, pass_bytes) in enumerate([("mix", 0, 0, 0, 0), ("mix", 4, 1, 1, 1024), ("near", 1, 0, 3, 1024), ("near", 4, 1, 7, 0),
                                                                  ("edges", 0, 0, 1, 1024)]):
        gens = GENS[name][:2]
        cfg = [str(bits), str(zero), str(misalign), str(pass_bytes)]
        archive, h = [], 0xCBF29CE484222325
        for g, c in enumerate(gens):
            src, off = (str(tmp_path / ("%s%d_%d" % (k, i, g))) for k in ("src", "off"))
            with open(src, "wb") as f:
                f.write(c.buf[c.lead:].tobytes())
            with open(off, "wb") as f:
                f.write(c.off.tobytes())
            cfg += [src, off]
            ids, fresh = A.model(archive, c.frames)
            archive += [c.frames[int(j)] for j in fresh]
            for b in ids.tobytes() + fresh.tobytes():
                h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        r = subprocess.run([exe, *cfg], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (cfg[:4], r.stdout[-300:], r.stderr[-3000:])
        out = r.stdout.split()
        assert out[0] == str(len(archive)) and out[1] == "%016x" % h, (cfg[:4], r.stdout)

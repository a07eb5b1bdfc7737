"""The kernels that find duplicate frames (zeekstd_amd/csrc/zk_dedup.h -- the source hipcc compiles for gfx950: zk_k_dedup_insert, _verify,
_verify_long, _settle_long, _flags, _emit, _gather) executed on the CPU by tests/sim/zk_dedup_sim.cpp under the workgroup emulator, with the
launchers' grids, the rounds and the scratch layout of zk_dedup_core, and compared entry by entry with the model of
tests/helpers/dedup_model.py (a dict from bytes to first index) on the input list the GPU tests share: under every ZK_CHOICE_DEDUP_KEY_BITS
of the list, gathered in one slice and in slices of 1 KiB, in both lane orders, from sources that start 0, 1, 3 and 7 bytes into their
allocation and end with it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import dedup_model as M

CASES = M.cases()
PLACES = [(0, False), (1, True), (3, False), (7, True)]          # (misalign, descending order of lanes and workgroups)


def check(c, got, what):
    ref, uniq, ids = c.model()
    assert len(got["uniq"]) == len(uniq), (what, len(got["uniq"]), len(uniq))
    for name, want in (("ref", ref), ("uniq", uniq), ("ids", ids)):
        bad = np.nonzero(got[name] != want)[0]
        assert bad.size == 0, (what, name, int(bad[0]), int(got[name][bad[0]]), int(want[bad[0]]))
    if got["gathered"] is not None:
        assert got["gathered"] == c.unique_bytes(), what


@pytest.mark.parametrize("bits", M.KEY_BITS)
@pytest.mark.parametrize("name", list(CASES))
def test_ref_uniq_ids_equal_the_model(name, bits):
    c = CASES[name]
    # every place for the list of edges; two of them, one per slice, for the others
    runs = [(m, d, s) for (m, d) in PLACES for s in M.SLICES] if name == "edges" else [(1, True, 0), (3, False, 1024)] if bits else [(0, False, 1024), (7, True, 0)]
    for misalign, descending, slice_bytes in runs:
        got = M.sim(c, None, bits, misalign, descending, slice_bytes)
        check(c, got, (misalign, descending, slice_bytes))
        if slice_bytes and len(c.unique_bytes()) > 4096:
            assert got["slices"] > 1
    full = M.sim(c, None, 0)
    assert full["rounds"] == 1                                     # no two contents of the list share a length and the 64 bits of the hash
    memo = {}
    want = np.array([memo.setdefault(f, M.frame_hash(f)) for f in c.frames], np.uint64)
    assert (full["hash"] == want).all(), int(np.nonzero(full["hash"] != want)[0][0])


def test_short_keys_reach_the_rounds():
    """what ZK_CHOICE_DEDUP_KEY_BITS is for: with one bit two keys hold every content, and a round settles one content per key"""
    c = CASES["edges"]
    n_unique = len(c.model()[1])
    assert M.sim(c, None, 1)["rounds"] >= n_unique // 2
    assert M.sim(c, None, 16)["rounds"] >= 1


@pytest.mark.parametrize("name", ["edges", "far_pairs", "all_same_long", "all_distinct"])
def test_any_key_function_gives_the_rule(name):
    """the result must not depend on the hash: every frame the same hash (the length alone tells keys apart), a hash of two values (the
    parity of the bytes' sum), and XXH64"""
    c = CASES[name]
    for h in (np.zeros(c.count, np.uint64), np.array([sum(f) % 2 for f in c.frames], np.uint64), M.hashes(c)):
        for bits, (misalign, descending) in zip((0, 1, 4), PLACES):
            got = M.sim(c, h, bits, misalign, descending, 1024)
            check(c, got, (bits, misalign))
    if name == "all_distinct":
        # distinct frames of one length under one hash: as many rounds as frames
        same_len = M.Case("same_len", [bytes([k & 255, k >> 8]) * 40 for k in range(300)])
        got = M.sim(same_len, np.zeros(300, np.uint64), 0, 3, True)
        check(same_len, got, "same_len")
        assert got["rounds"] == 300


def test_kernels_under_sanitizers(tmp_path):
    """The same kernels under the emulator, built with AddressSanitizer + UBSan (tests/sim/dedup_san.cpp, a program of its own): the source
    ends with its allocation and starts 0, 1, 3 or 7 bytes into it, so a load that leaves the frames is a report; the short, the misaligned
    and the end-of-allocation cases, the long compare, the gather in slices of 1 KiB."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from conftest import ROOT
    exe = str(tmp_path / "dedupsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "dedup_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    # frames that end the allocation: a short one, one of 17 bytes, one that ends on a 16-byte seam, and a copy of each further up
    rng = np.random.default_rng(5)
    tails = {}
    for n in (1, 15, 17, 64, 65, 333, 4097):
        f = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        tails["tail_%d" % n] = M.Case("tail_%d" % n, [f, rng.integers(0, 256, 7, dtype=np.uint8).tobytes(), f[:-1], f], lead=2)
    runs = []
    for i, (c, bits, misalign, slice_bytes) in enumerate([(CASES["edges"], 0, 0, 0), (CASES["edges"], 1, 1, 1024), (CASES["edges"], 4, 3, 1024), (CASES["edges"], 16, 7, 0),
                                                        (CASES["far_pairs"], 1, 3, 1024), (CASES["all_same_long"], 0, 7, 1024), (CASES["one"], 0, 1, 0),
                                                        (CASES["all_empty"], 0, 0, 0)] + [(c, b, m, 1024) for c, b, m in zip(tails.values(), (0, 1, 0, 4, 0, 1, 0), (0, 1, 3, 7, 1, 3, 7))]):
        src, off, h = (str(tmp_path / ("%s%d" % (k, i))) for k in ("src", "off", "hash"))
        with open(src, "wb") as f:
            f.write(c.buf[c.lead:].tobytes())
        with open(off, "wb") as f:
            f.write(c.off.tobytes())
        with open(h, "wb") as f:
            f.write(np.zeros(c.count, np.uint64).tobytes())
        # zk_k_dedup_hash's hashes; for some runs every hash 0, so that frames of one length meet wrong leaders and are compared
        runs.append(([src, off, h if i % 3 == 2 else "-", str(bits), str(misalign), str(slice_bytes)], c))
    first = True
    for cfg, c in runs:
        r = subprocess.run([exe, *cfg], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (cfg, r.stdout[-300:], r.stderr[-3000:])
        ref, uniq, ids = c.model()
        h = 0xCBF29CE484222325
        for b in ref.tobytes() + ids.tobytes():
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        out = r.stdout.split()
        assert out[0] == str(len(uniq)) and out[3] == "%016x" % h, (cfg, r.stdout)

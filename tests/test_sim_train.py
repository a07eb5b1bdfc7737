"""The kernels that select a trained dictionary's content (zeekstd_amd/csrc/zk_train.h -- the source hipcc compiles for gfx950:
zk_k_train_count, zk_k_train_select) executed on the CPU by tests/sim/zk_train_sim.cpp under the workgroup emulator, with the launchers' grids
and the scratch layout of zk_train_run, and compared with the numpy model of tests/helpers/train_model.py: every position's hash, every
counter, the segments in the order taken and the content's bytes, in both lane orders.  The reference has no trainer (it is handed contexts
that already hold a dictionary) and libzstd's ZDICT_trainFromBuffer follows another rule, so the rule of include/zeekstd_amd.h, restated in
numpy, is the yardstick.  The inputs are built for the rule's edges (train_model.cases); what makes each one an edge is asserted on the model
alone first."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import train_model as M

CASES = M.cases()


def _facts(c, hp, fr, segs, content, trace):
    """what makes the input the edge its name says, on the model alone"""
    n, k, d = len(hp), c.k, c.d
    E, full = M.epochs(n, k, c.ccap), c.ccap // k
    off = np.cumsum([0] + [len(s) for s in c.samples])
    rounds = trace[-1][0] + 1 if trace else 0
    if c.name.startswith("short_samples"):
        sizes = [len(s) for s in c.samples]
        assert {0, d - 1, d, d + 1} <= set(sizes) and c.lead > 0 and sizes[-1] == 0
        i = sizes.index(d - 1)                                  # no position of the sample of d - 1 bytes has a d-mer; exactly one / two of the next two
        assert (hp[off[i]:off[i + 1]] == M.NONE).all()
        i = sizes.index(d)
        assert (hp[off[i]:off[i + 1]] != M.NONE).sum() == 1 and hp[off[i]] != M.NONE
        i = sizes.index(d + 1)
        assert (hp[off[i]:off[i + 1]] != M.NONE).sum() == 2
        assert int((hp != M.NONE).sum()) == sum(max(0, s - d + 1) for s in sizes) == int(fr.sum())
    elif c.name == "collisions_f10":
        wide = M.hashes(*M.join(c.samples), d, 24)
        distinct = len(np.unique(wide[wide != M.NONE]))
        assert distinct > 2 * (1 << c.f) and np.count_nonzero(fr) < distinct // 2       # d-mers share counters
    elif c.name == "one_epoch":
        assert E == 1 and n // (10 * k) == 1 and rounds > 1 and len(content) < c.ccap
    elif c.name == "second_round":
        assert E == n // (10 * k) < full and rounds == 2 and len(segs) == full > E
    elif c.name == "filled_exactly":
        assert E == full < n // (10 * k) and rounds == 1 and len(content) == c.ccap and len(segs) == full
    elif c.name == "nothing_left":
        assert 0 < len(segs) < E and rounds == 1 and len(content) < c.ccap           # later epochs and the second round found only zeros
    elif c.name == "straddle":
        assert len(segs) == 1 and any(segs[0] < b < segs[0] + k for b in off[1:-1]), (segs, "lies inside one sample")
    elif c.name == "tie":
        assert trace[0][4] > 1 and segs[0] == 0                     # several starts share the best score: the lowest is taken
    else:
        raise AssertionError("an input without facts: " + c.name)


@pytest.mark.parametrize("name", list(CASES))
def test_count_and_select_equal_the_model(name):
    c = CASES[name]
    trace = []
    hp, fr, (segs, content) = c.model(trace)
    _facts(c, hp, fr, segs, content, trace)
    buf, off = c.buffers()
    for descending in (False, True):
        shp, sfr, res = M.sim(buf, off, c.d, c.f, [c.k], c.ccap, descending)
        assert (shp == hp).all(), (descending, int(np.nonzero(shp != hp)[0][0]))
        assert (sfr == fr).all(), (descending, int(np.nonzero(sfr != fr)[0][0]))
        assert res[0][0] == segs, descending
        assert res[0][1] == content, descending


def test_candidates_share_the_count_and_not_the_counters():
    """the launcher's grid of candidates: a workgroup each on its own copy of the counters -- every candidate's result is the one it has alone;
    and no segment at all (fewer bytes than k in the one epoch): the tail of the samples"""
    c = CASES["filled_exactly"]
    data, off = M.join(c.samples)
    hp = M.hashes(data, off, 8, 16)
    fr = M.count(hp, 16)
    ks = [64, 128, 256, 512]
    _, _, res = M.sim(data.tobytes(), off, 8, 16, ks, 2048)
    for k, got in zip(ks, res):
        assert got == M.select(data, hp, fr, k, 8, 2048), k
    tiny = [bytes([65 + i]) * 8 for i in range(8)]
    data, off = M.join(tiny)
    _, _, res = M.sim(data.tobytes(), off, 8, 16, [256], 512)
    assert res[0] == ([], b"".join(tiny)) == M.train(tiny, 1024, 256, f=16)


def _code(v, base):
    """the code whose baseline is the largest not above v (RFC 8878 3.1.1.3.2.1.1: the tables of tests/helpers/zstd_gen.py)"""
    return int(np.searchsorted(np.asarray(base), v, side="right")) - 1


def test_stats_equal_an_independent_count():
    """zk_k_train_stats under the emulator, with more blocks than workgroups and with one workgroup, both lane orders: 256 literal counts and
    the LL / ML / OF code counts equal a count made here from the format's baseline tables -- every literal-length code a packed sequence can hold and every match-length code
    occurs, the values at both edges of every code, offsets from repeat codes (Offset_Value 1..3) to 2^27"""
    from helpers import zstd_gen as zg
    rng = np.random.default_rng(11)
    ll_edges = sorted(set([b for b in zg.LL_BASE if b < 65536] + [b - 1 for b in zg.LL_BASE[1:]]))       # (16 bits hold a literal length: code 35 cannot occur)
    ml_edges = sorted(set([b for b in zg.ML_BASE if b < 65536] + [b - 1 for b in zg.ML_BASE[1:] if b - 1 < 65536] + [65535]))
    assert zg.ML_BASE[0] == 3 and len(zg.LL_BASE) == 36 and len(zg.ML_BASE) == 53
    nb = 37
    nseq, nlit, seqs, lits = [], [], [], []
    want = np.zeros(377, np.int64)
    for b in range(nb):
        k = 0 if b in (3, 20) else int(rng.integers(1, 700))
        ll = rng.choice(ll_edges, k) if b % 2 else rng.integers(0, 40, k)
        ml = rng.choice(ml_edges, k) if b % 3 else rng.integers(3, 60, k)
        ov = np.where(rng.integers(0, 4, k) == 0, rng.integers(1, 4, k), (1 << rng.integers(2, 28, k)) + rng.integers(0, 4, k))
        for a, m, o in zip(ll, ml, ov):
            want[256 + _code(int(a), zg.LL_BASE)] += 1
            want[292 + _code(int(m), zg.ML_BASE)] += 1
            want[345 + int(o).bit_length() - 1] += 1
        seqs.append(np.asarray(ll, np.uint64) | (np.asarray(ml, np.uint64) << np.uint64(16)) | (np.asarray(ov, np.uint64) << np.uint64(32)))
        lt = rng.integers(0, 256, 0 if b == 5 else int(rng.integers(1, 3000)), dtype=np.uint8) if b % 4 else np.full(513, b, np.uint8)
        want[:256] += np.bincount(lt, minlength=256)
        lits.append(lt); nseq.append(k); nlit.append(len(lt))
    assert (want[256:291] > 0).all() and want[291] == 0 and (want[292:345] > 0).sum() >= 50 and (want[345:373] > 0).all()
    # (the blocks lie in their buffers with gaps, as the plan leaves them)
    sb = np.concatenate([[0], np.cumsum(np.asarray(nseq) + 3)])[:-1].astype(np.uint64)
    lb = np.concatenate([[0], np.cumsum(np.asarray(nlit) + 5)])[:-1].astype(np.uint64)
    S = np.full(int(sb[-1]) + nseq[-1], (7 << 32) | (9 << 16) | 50000, np.uint64)
    Lb = np.full(int(lb[-1]) + nlit[-1], 0xEE, np.uint8)
    for b in range(nb):
        S[int(sb[b]):int(sb[b]) + nseq[b]] = seqs[b]
        Lb[int(lb[b]):int(lb[b]) + nlit[b]] = lits[b]
    nq, nl = np.asarray(nseq, np.uint32), np.asarray(nlit, np.uint32)
    for wgs in (nb, 4, 1):
        for desc in (0, 1):
            got = np.full(377, 0x5A5A5A5A, np.uint32)
            assert M.lib().zk_train_sim_stats(nq.ctypes.data, nl.ctypes.data, sb.ctypes.data, lb.ctypes.data, nb, S.ctypes.data, len(S), Lb.ctypes.data, len(Lb),
                                              wgs, desc, got.ctypes.data) == 0
            assert (got.astype(np.int64) == want).all(), (wgs, desc, np.nonzero(got != want)[0][:5])


def test_trial_samples():
    """every j-th sample above the trial limit: the stride rule (the smallest j that fits; the first sample alone when none does; all when
    they fit), and zk_k_train_gather puts exactly those samples behind one another"""
    assert M.trial_stride([100] * 10, 1000) == 1 and M.trial_stride([100] * 10, 999) == 2 and M.trial_stride([100] * 10, 499) == 3
    assert M.trial_stride([100] * 10, 99) == 10 and M.trial_stride([50] + [100] * 9, 99) == 10
    assert M.trial_stride([10, 500, 10, 500, 10, 500], 100) == 2           # (j = 2 takes samples 0, 2, 4)
    c = CASES["short_samples_d8"]
    buf, off = c.buffers()
    sizes = np.diff(off.astype(np.int64))
    for j in (2, 3, 7, len(sizes)):
        pick = c.samples[::j]
        sub = np.concatenate([[0], np.cumsum([len(x) for x in pick])]).astype(np.uint64)
        data = np.frombuffer(buf, np.uint8)
        got = np.zeros(max(int(sub[-1]), 1), np.uint8)
        assert M.lib().zk_train_sim_gather(data.ctypes.data, off.ctypes.data, len(sizes), j, sub.ctypes.data, len(pick), got.ctypes.data) == 0
        assert got[:int(sub[-1])].tobytes() == b"".join(pick), j


def test_kernels_under_sanitizers(tmp_path):
    """The same kernels under the emulator, built with AddressSanitizer + UBSan (tests/sim/train_san.cpp, a program of its own), on the inputs
    whose samples end a few bytes after a position's d-mer would (the last sample of d + 1 bytes, empty ones at the end, a list that does not
    start at 0) and on four candidates at once."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from conftest import ROOT
    exe = str(tmp_path / "trainsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "train_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    runs = []
    for i, (name, cfg) in enumerate([("short_samples_d6", ["6", "16", "1024", "32"]), ("short_samples_d8", ["8", "10", "1000", "32", "64"]),
                                     ("filled_exactly", ["8", "16", "2048", "64", "128", "256", "512"]), ("tie", ["8", "12", "32", "32"])]):
        c = CASES[name]
        samples = list(c.samples)
        if name.startswith("short"):
            samples += [b"x" * (c.d + 1), b""]                      # the buffer ends one byte behind the last d-mer
        data, off = M.join(samples)
        p, q = str(tmp_path / f"in{i}"), str(tmp_path / f"off{i}")
        with open(p, "wb") as f:
            f.write(b"\xEE" * 5 + data.tobytes())
        with open(q, "wb") as f:
            f.write((off + np.uint64(5)).tobytes())
        runs.append([p, q] + cfg)
    first = True
    for cfg in runs:
        r = subprocess.run([exe, *cfg], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (cfg, r.stdout[-300:], r.stderr[-3000:])

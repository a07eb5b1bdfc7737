"""The kernels that feed the encoder's matcher its far history (zeekstd_amd/csrc/zk_enc_far.h -- the source hipcc compiles for gfx950:
zk_k_enc_dense_part, zk_k_enc_dense_cand, zk_k_enc_ldm_build, zk_k_enc_ldm_build_frames, zk_k_enc_stage_hist) executed on the CPU by
tests/sim/zk_enc_far_sim.cpp under the workgroup emulator, with the engine's plan, the launchers' grids and the engine's slices, and compared
ENTRY BY ENTRY with the tables of the CPU twin (oracle/zstd_oracle_enc.c: zko_enc_far_debug over its own ldm_build_frame, dense_build_frame
and dense_lookup).  What the reference does here is libzstd's match finder with a 2 MiB window behind ZSTD_compressStream2
(lib/src/encode.rs:340-346; cli/src/args.rs:192 level 3); compressed bytes are unpinned by it, so the twin is the yardstick.  The final
bytes of a GPU encode are a weak witness for these kernels -- a wrong candidate is invisible wherever the ring offers the parse something
as good -- so here every position's candidate is looked at, on inputs built to reach the kernels' edges (tests/helpers/enc_far_inputs.py:
the facts that make them so are asserted on the twin alone first)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import enc_far_inputs as I
from helpers import enc_far_sim as S
from oracle import zko

CASES = [(name, level) for name in I.NAMES for level in I.get(name).levels]


@pytest.mark.parametrize("name,level", CASES, ids=[f"{n}-l{l}" for n, l in CASES])
def test_dense_candidates_equal_twin(name, level):
    """zk_k_enc_dense_part + zk_k_enc_dense_cand, every workgroup of every slice: the input reaches its facts on the twin; every position's
    entry equals the twin's triple under the rule of enc_far_sim.compare_dense, positions without one read 0 (the scratch was poisoned), the
    position lists are the right sets; and all of it again with the lanes visited in descending order -- minimum, maximum and cursors are
    atomics, a position is looked up in exactly one pass: `cand` and `poff` come out identical, `part` as the same sets."""
    e = I.get(name)
    refs = S.reference(e.data, e.frame_size, level)
    e.facts(refs, level)
    for sl in e.slices:
        up = S.dense(e.data, e.frame_size, level, sl)
        assert up is not None
        S.compare_dense(e.data, e.frame_size, level, up, refs)
        down = S.dense(e.data, e.frame_size, level, sl, descending=True)
        assert (up[2] == down[2]).all(), sl
        differ = np.nonzero(up[0] != down[0])[0]
        assert differ.size == 0, (sl, "first position whose entry depends on the lane order", int(differ[0]))
        S.compare_dense(e.data, e.frame_size, level, down, refs)


def test_no_dense_history_where_the_plan_has_none():
    """levels 1 and 2, and frames within the ring's reach: the engine launches neither kernel, nor does the harness"""
    e = I.get("window_edge")
    assert S.dense(e.data, e.frame_size, 2) is None and S.dense(e.data, e.frame_size, 1) is None
    assert S.dense(e.data[:50000], e.frame_size, 3) is None


@pytest.mark.parametrize("level", [2, 3])
def test_sampled_tables_per_frame_equal_twin(level):
    """zk_k_enc_ldm_build_frames over the launcher's grid (blockIdx.y = frame): two frames of different sizes in one call, each with its own
    zke_ldm_log inside the common stride -- equal to the twin's ldm_build_frame exactly, the rest of a smaller frame's stride still empty;
    the same under descending lane order; and the dense inputs whose frames end at every alignment."""
    shapes = I.ldm_frames_inputs() + [(n, I.get(n).data, I.get(n).frame_size) for n in ("frame_tail/r0", "frame_tail/r1", "frame_tail/r2", "frame_tail/r3")]
    for name, data, fs in shapes:
        refs = S.reference(data, fs, level, dense_triples=False)
        got = S.ldm_frames(data, fs, level)
        assert got is not None, name
        tables, log = got
        logs = set()
        for f, ref in enumerate(refs):
            assert ref[0] is not None, (name, f)
            want = np.full(1 << log, S.LDM_NONE, np.uint32)
            want[:len(ref[0])] = ref[0]
            logs.add(len(ref[0]))
            if name.startswith("ldm_frames"):
                assert int((ref[0] != S.LDM_NONE).sum()) > 1000, name               # (text: one position in 32 is sampled)
            assert (tables[f] == want).all(), (name, f, int(np.nonzero(tables[f] != want)[0][0]))
        if name.startswith("ldm_frames"):
            assert len(logs) == 2, (name, logs)
        down = S.ldm_frames(data, fs, level, descending=True)
        assert (down[0] == tables).all(), name


def test_sampled_table_over_a_prefix_equals_twin():
    """zk_k_enc_ldm_build: prefix lengths of every alignment (the fifth word put together byte by byte near the end), one byte beyond the
    ring's reach, and one whose last sampled position is n - ZKE_LDM_MIN -- the twin's ldm_build exactly, with exactly ZKE_LDM_SLACK bytes
    (of 0xA5, not zeros) behind the copy; a prefix the ring holds gets no table."""
    pre = I.prefixes()
    assert set(pre) == {"mod4=0", "mod4=1", "mod4=2", "mod4=3", "window+1", "last_selected"}
    assert sorted(len(pre[f"mod4={r}"]) % 4 for r in range(4)) == [0, 1, 2, 3] and len(pre["window+1"]) == S.WINDOW + 1
    for name, p in pre.items():
        want = zko.enc_ldm_prefix_debug(p)
        assert want is not None and int((want != S.LDM_NONE).sum()) > 1000, name
        if name == "last_selected":
            assert (want == len(p) - S.LDM_MIN).any()
        got = S.ldm_prefix(p)
        assert got.shape == want.shape and (got == want).all(), (name, int(np.nonzero(got != want)[0][0]))
        assert (S.ldm_prefix(p, descending=True) == want).all(), name
    assert S.ldm_prefix(pre["window+1"][:-1]) is None and zko.enc_ldm_prefix_debug(pre["window+1"][:-1]) is None


def test_sampled_table_over_a_prefix_longer_than_its_reach():
    """u0 > 0: the table covers the last ZKE_LDM_MAX_OFF = 2^27 - 1 bytes of the prefix, positions counted from u0.  128 MiB + 5 bytes (u0 = 6)
    is the smallest such prefix; a repeating 1 MiB of text with a counter stamped into each repeat keeps the generator out of the test's time."""
    n = S.LDM_MAX_OFF + 6
    unit = np.frombuffer(zko.gen_text(1 << 20, 191), np.uint8)
    buf = np.tile(unit, n // len(unit) + 1)[:n].copy()
    buf[::4099] = np.arange(len(buf[::4099]), dtype=np.uint32).astype(np.uint8)
    p = buf.tobytes()
    want = zko.enc_ldm_prefix_debug(p)
    assert want is not None and len(want) == 1 << 23
    got = S.ldm_prefix(p)
    assert (got == want).all(), int(np.nonzero(got != want)[0][0])
    used = want[want != S.LDM_NONE]
    assert len(used) > 40000 and int(used.max()) > S.LDM_MAX_OFF - (1 << 20) and int(used.min()) < 64       # positions counted from u0, up to the last MiB


@pytest.mark.parametrize("plen", [1003, S.WINDOW - 1, S.WINDOW + 1, 70001])
def test_matcher_records_equal_their_definition(plen):
    """zk_k_enc_stage_hist: every frame's record is [the last hist bytes of the prefix | the frame], hist = the ring's reach rounded down to
    a multiple of four; three frames, the last one short; nothing else is written"""
    prefix = zko.gen_text(plen, 201)
    data = zko.gen_text(2 * 9000 + 1234, 202)
    got, hist = S.stage_hist(data, 9000, 1, prefix)
    assert hist == min(plen, S.WINDOW) & ~3
    want = bytearray(b"\xA5" * (3 * (hist + 9000)))
    for f in range(3):
        rec = prefix[plen - hist:] + data[9000 * f:9000 * (f + 1)]
        want[f * (hist + 9000):f * (hist + 9000) + len(rec)] = rec
    assert got == bytes(want)


def test_far_history_kernels_under_sanitizers(tmp_path):
    """The same kernels under the emulator, built with AddressSanitizer + UBSan (tests/sim/enc_far_san.cpp, a program of its own): their
    `__shared__` tables, cursors and counters are real arrays on the CPU and every buffer is an exact-size heap allocation, so an LDS index
    out of range or a read or write beyond the source, the candidate / position arrays and their slack, the tables or the records is a
    report.  Shapes: enc_far_inputs.SAN_SHAPES (frame starts and tails at the four alignments, a third segment of five bytes, crowded
    chunks, 16 frames in slices of three), and the prefix table + records at a prefix length of 1 mod 4."""
    from conftest import ROOT
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "farsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "enc_far_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    runs = []
    for i, (name, level, sl) in enumerate(I.SAN_SHAPES):
        e = I.get(name)
        path = str(tmp_path / f"in{i}")
        with open(path, "wb") as f:
            f.write(e.data)
        runs.append(["frames", path, str(e.frame_size), str(level), str(sl)])
    path = str(tmp_path / "pre")
    with open(path, "wb") as f:
        f.write(I.prefixes()["mod4=1"] + zko.gen_text(20001, 211))
    runs.append(["prefix", path, "9000", "1", str(len(I.prefixes()["mod4=1"]))])
    first = True
    for cfg in runs:
        r = subprocess.run([exe, *cfg], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (cfg, r.stdout[-300:], r.stderr[-3000:])

"""The kernels that find content-defined frame boundaries (zeekstd_amd/csrc/zk_cdc.h -- the source hipcc compiles for gfx950: zk_k_cdc_mark,
zk_k_cdc_emit, zk_k_cdc_select and, from two segments on, zk_k_cdc_spec / zk_k_cdc_fix / zk_k_cdc_copy) executed on the CPU by tests/sim/zk_cdc_sim.cpp under the workgroup emulator, with the launchers' grids, the
slices and the scratch layout of zk_cdc_pass, and compared with the numpy model of tests/helpers/cdc_model.py: the candidate bitmap and
the offsets, entry by entry, on the input list the GPU tests share -- in both lane orders, in slices of 1 KiB (a seam every 1024 bytes: the
31-byte window read across it, the chain's cut carried over it) and in one slice, from sources that start 0, 1, 3 and 7 bytes into their
allocation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import cdc_model as M

CASES = M.cases()
# (misalign, descending lane order, slice bytes: 0 = the default): four of the combinations for every input, all sixteen for some
RUNS = [(0, False, 0), (1, True, 1024), (3, False, 1024), (7, True, 0)]
ALL_RUNS = [(m, d, s) for m in (0, 1, 3, 7) for d in (False, True) for s in (0, 1024)]
EVERY_COMBINATION = ("random_256", "text_1024", "dense_mid_256", "dense_mid_long", "zeros_256", "len33_256", "len1025_256", "short_last_1024",
                     "on_lo_256", "on_hi_4096", "equal_1024")


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if len(c.data)])
def test_bitmap_and_offsets_equal_the_model(name):
    c = CASES[name]
    want_bm, want_off = c.bitmap(), c.cuts()
    for misalign, descending, slice_bytes in (ALL_RUNS if name in EVERY_COMBINATION else RUNS):
        bm, off, count = M.sim(c.data, c.mn, c.bits, c.mx, slice_bytes, misalign, descending)
        assert (bm == want_bm).all(), (misalign, slice_bytes, int(np.nonzero(bm != want_bm)[0][0]))
        assert count == len(want_off) - 1, (misalign, slice_bytes, count)
        assert (off[:count + 1] == want_off).all(), (misalign, slice_bytes, int(np.nonzero(off[:count + 1] != want_off)[0][0]))
        assert (off[count + 1:] == 0xA5A5A5A5A5A5A5A5).all()           # (the harness's poison: no kernel wrote behind the last cut)


def test_slices_of_other_sizes_and_a_counting_pass():
    """seams that fall inside a tile's worth of positions and on a tile's edge; cuts that find no room are counted and not stored"""
    c = CASES["random_256"]
    data = c.data[:100000]
    want = M.cuts(data, c.mn, c.bits, c.mx)
    for slice_bytes in (32768, 33792, 65536, 3072, 98304):
        _, off, count = M.sim(data, c.mn, c.bits, c.mx, slice_bytes, 5, False)
        assert count == len(want) - 1 and (off[:count + 1] == want).all(), slice_bytes
    _, off, count = M.sim(data, c.mn, c.bits, c.mx, 4096, 0, False, off_cap=10)
    assert count == len(want) - 1 and (off == want[:11]).all()


def test_kernels_under_sanitizers(tmp_path):
    """The same kernels under the emulator, built with AddressSanitizer + UBSan (tests/sim/cdc_san.cpp, a program of its own): the source
    ends with its allocation and starts 0, 1, 3 or 7 bytes into it, so an aligned 16-byte load that leaves it is a report; short inputs,
    the dense run, seams every 1024 bytes."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from conftest import ROOT
    exe = str(tmp_path / "cdcsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "cdc_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    runs = []
    for i, (name, slice_bytes, misalign) in enumerate([("len1_256", 0, 0), ("len31_256", 0, 1), ("len33_1024", 1024, 3), ("len1025_256", 1024, 7),
                                                       ("dense_mid_256", 0, 3), ("text_4096", 0, 1), ("short_last_1024", 1024, 7),
                                                       # several segments: the parallel selection, in one slice and carried across two
                                                       ("dense_mid_long", 0, 3), ("random_256", 98304, 1), ("dense_long_min200", 0, 7), ("zeros_256", 0, 1)]):
        c = CASES[name]
        data = c.data
        p = str(tmp_path / f"in{i}")
        with open(p, "wb") as f:
            f.write(data.tobytes())
        want = len(M.cuts(data, c.mn, c.bits, c.mx)) - 1
        runs.append(([p, str(c.mn), str(c.bits), str(c.mx), str(slice_bytes), str(misalign), str(len(data) // c.mn + 1)], want))
    first = True
    for cfg, want in runs:
        r = subprocess.run([exe, *cfg], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (cfg, r.stdout[-300:], r.stderr[-3000:])
        assert r.stdout.split()[0] == str(want), (cfg, r.stdout)

"""The digest kernels (zeekstd_amd/csrc/zk_digest.h -- the source hipcc compiles for gfx950: zk_k_digest_counts, _sha256, _leaves, _roots)
executed on the CPU by tests/sim/zk_digest_sim.cpp under the workgroup emulator, with the launchers' grids, in both lane orders, and compared
with hashlib (tests/helpers/digest_model.py): every digest of every list, for both algorithms, the bytes behind the poisoned digest array
untouched.  The lane code alone hashes one frame longer than 2^32 bits.  The harness is compiled here, into a temporary directory."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import digest_model as D

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return D.build_sim(tmp_path_factory.mktemp("digest_sim"))


def check(lib, algo, name, misalign, descending, base=0):
    data, off = D.lists()[name]
    rc, got, tail = D.sim(lib, algo, data, off + np.uint64(base), misalign=misalign, descending=descending)
    assert rc == 0, (algo, name, misalign, descending, rc)
    want = D.want(algo, name)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (algo, name, misalign, descending, bad[:8].tolist(), [int(off[i + 1] - off[i]) for i in bad[:8]])
    assert (tail == D.POISON).all(), (algo, name, "a store behind the digests")


def test_the_model_gives_the_header_s_literals():
    assert hashlib.sha256(b"").hexdigest() == D.EMPTY_SHA256
    assert D.tree(b"").hex() == D.EMPTY_TREE
    assert D.tree(bytes(i & 255 for i in range(4097))).hex() == D.TREE_4097


@pytest.mark.parametrize("algo", list(D.ALGOS))
def test_the_literals_come_out_of_the_kernels(lib, algo):
    """the empty frame (both algorithms) and the 4097 bytes i & 255 (the tree), asserted as literals"""
    empty = {"sha256": D.EMPTY_SHA256, "blake2s-tree": D.EMPTY_TREE}[algo]
    for descending in (False, True):
        rc, got, _ = D.sim(lib, algo, np.zeros(0, np.uint8), np.zeros(2, np.uint64), descending=descending)
        assert rc == 0 and got[0].tobytes().hex() == empty
        if algo == "blake2s-tree":
            m = (np.arange(4097) & 255).astype(np.uint8)
            rc, got, _ = D.sim(lib, algo, m, np.array([0, 4097], np.uint64), descending=descending)
            assert rc == 0 and got[0].tobytes().hex() == D.TREE_4097


@pytest.mark.parametrize("algo", list(D.ALGOS))
@pytest.mark.parametrize("name", list(D.lists()))
def test_every_list_equals_hashlib_in_both_lane_orders(lib, algo, name):
    check(lib, algo, name, 0, False)
    check(lib, algo, name, 3, True, base=(1 << 32) + 12345)        # (the offsets are coordinates: only their differences reach the source)


@pytest.mark.parametrize("algo", list(D.ALGOS))
@pytest.mark.parametrize("misalign", D.MISALIGN)
def test_the_edge_list_at_every_misalignment(lib, algo, misalign):
    check(lib, algo, "edges", misalign, False)
    check(lib, algo, "edges", misalign, True)


def test_the_plan_functions(lib):
    """leaves per frame as the rule states them; the launchers' grids; the scratch of a call; the archive route's passes: whole frames of at most
    the pass size, one at least"""
    assert [lib.zkg_sim_leaves(n) for n in (0, 1, 4096, 4097, 8192, 8193, 1 << 30)] == [1, 1, 1, 2, 2, 3, 1 << 18]
    assert [lib.zkg_sim_blocks(n) for n in (1, 128, 129, 1 << 40)] == [1, 1, 2, 1 << 20]
    assert lib.zkg_sim_scratch(3, 10) == 3 * 8 + 4 * 8 + 10 * 32
    off = np.array([5, 5, 105, 1105, 1105, 1205, 1206], np.uint64)
    cuts = lambda cap: [lib.zkg_sim_pass_end(off.ctypes.data, a, 6, cap) for a in range(6)]
    assert cuts(1 << 30) == [6] * 6
    assert cuts(100) == [2, 2, 3, 5, 5, 6]                   # (the frame of 1000 bytes is a pass of its own)
    assert cuts(1100) == [4, 4, 5, 6, 6, 6]


def test_sha256_bit_length_above_2_to_the_32(lib):
    """one frame of 2^29 + 3 pattern bytes by the lane code alone (zkg_sha256_step, outside the fibre emulator): its length in bits does not fit
    32 bits.  Not repeated on the device, where it would be one lane's chain of the same source"""
    n = (1 << 29) + 3
    out = np.zeros(32, np.uint8)
    lib.zk_digest_sim_long_sha256(n, out.ctypes.data)
    assert out.tobytes().hex() == hashlib.sha256(D.long_pattern(n)).hexdigest()
    # and the padding edges through the same driver
    for k in (0, 55, 56, 63, 64, 119, 120):
        lib.zk_digest_sim_long_sha256(k, out.ctypes.data)
        assert out.tobytes().hex() == hashlib.sha256(D.long_pattern(k)).hexdigest(), k


def test_kernels_under_sanitizers(tmp_path):
    """The same kernels under the emulator, built with AddressSanitizer + UBSan (tests/sim/digest_san.cpp, a program of its own): source,
    offsets, digests and scratch are allocations of exactly the layout's sizes, the source starts 0, 1, 3 or 15 bytes into its own and ends
    with it, so a load that leaves the list is a report"""
    from conftest import ROOT
    exe = str(tmp_path / "digestsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "digest_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    runs = [(name, m) for name in ("edges", "short_65", "empty_300", "one_frame") for m in D.MISALIGN] + [("edges_waves", 1), ("short_257", 15)]
    first = True
    for name, misalign in runs:
        data, off = D.lists()[name]
        src, offs = str(tmp_path / "src.bin"), str(tmp_path / "off.bin")
        data.tofile(src)
        (off + np.uint64(777)).tofile(offs)
        for algo, code in D.ALGOS.items():
            r = subprocess.run([exe, str(code), str(misalign), src, offs], capture_output=True, text=True, timeout=900)
            if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
                pytest.skip("the sanitizer runtime cannot start here")
            first = False
            assert r.returncode == 0, (name, misalign, algo, r.stdout[-200:], r.stderr[-3000:])
            assert r.stdout.strip() == D.want(algo, name).tobytes().hex(), (name, misalign, algo)

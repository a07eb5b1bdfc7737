"""The kernels of zk_read_view_ranges_dev (zeekstd_amd/csrc/zk_view.h -- the source hipcc compiles for gfx950: zk_k_view_check, _lens, _plan,
_bases, _mark, _gather, _status) executed on the CPU by tests/sim/zk_view_sim.cpp under the workgroup emulator, with the launchers' grids and the
engine's pass loop, in both lane orders, and compared byte by byte with the model of tests/helpers/view_model.py: the whole poisoned
destination, the statuses, the return value and the number of distinct frames decoded.  The harness is compiled here, into a temporary
directory."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import view_model as V

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

SIZES = V.edge_sizes()
FRAMES = [V.payload(f, n) for f, n in enumerate(SIZES)]
VIEWS = V.views(SIZES)
TAIL = 33
CHUNK = 64 << 10


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return V.build_sim(tmp_path_factory.mktemp("view_sim"))


def run(lib, ids, voff, ranges, mode, what, frames=FRAMES, dst_cap=None, **kw):
    given, offs, end = V.destinations(ranges, mode, v0=int(voff[0]), vend=int(voff[-1]))
    cap = end if dst_cap is None else dst_cap
    size = max(end, cap) + TAIL
    o, n = [r[0] for r in ranges], [r[1] for r in ranges]
    fill = 0xEE if kw.get("frame_err") else None
    want = V.model(frames, ids, voff, o, n, given, cap, size, frame_err=kw.get("frame_err"), failed_fill=fill)
    for misalign, descending in ((0, False), (3, True)):
        got = V.sim(lib, frames, ids, voff, o, n, given, cap, size, misalign=misalign, descending=descending, **kw)
        assert got["rc"] == want["rc"], (what, misalign, got["rc"], want["rc"])
        if want["dst"] is None:
            assert (got["dst"] == V.POISON).all() and (got["status"] == -12345).all(), what
            continue
        assert got["status"].tolist() == want["status"].tolist(), (what, misalign, V.first_diff(got["status"], want["status"]))
        bad = V.first_diff(got["dst"], want["dst"])
        assert bad is None, (what, mode, misalign, bad)
        assert got["decoded"] == len(want["decoded"]), (what, got["decoded"], len(want["decoded"]))
    return want, got


@pytest.mark.parametrize("name", list(VIEWS))
@pytest.mark.parametrize("mode", ["packed", "shuffled"])
def test_every_view_equals_the_model(lib, name, mode):
    ids, voff = VIEWS[name]
    run(lib, ids, voff, V.ranges_of(voff, dense=len(ids) <= 120), mode, name)


def test_an_empty_view_and_an_empty_list(lib):
    ids, voff = np.zeros(0, np.uint32), np.array([77], np.uint64)
    want, _ = run(lib, ids, voff, [(77, 0), (76, 0), (78, 0), (77, 1)], "packed", "empty view")
    assert want["status"].tolist() == [0, V.OUT_OF_RANGE, V.OUT_OF_RANGE, V.OUT_OF_RANGE]


def test_passes_are_slices_of_the_distinct_frames(lib):
    """a pass of 64 KiB over the interleaved view: one range's entries fall into different passes; a frame above the pass is a pass of its own"""
    ids, voff = VIEWS["thrice_interleaved"]
    ranges = V.ranges_of(voff, dense=False)
    want, got = run(lib, ids, voff, ranges, "shuffled", "passes", pass_bytes=64 << 10)
    assert got["passes"] >= 5 and got["decoded"] == sum(1 for n in SIZES if n)
    _, one = run(lib, ids, voff, ranges, "shuffled", "one pass")
    assert one["passes"] == 1 and (one["dst"] == got["dst"]).all()


def test_a_frame_named_a_thousand_times_is_decoded_once(lib):
    f = SIZES.index(4096)
    ids = np.full(1000, f, np.uint32)
    voff = V.offsets_of(SIZES, ids)
    want, got = run(lib, ids, voff, [(0, 1000 * 4096), (4095, 2), (999 * 4096, 4096)], "packed", "x1000")
    assert got["decoded"] == 1


def test_offsets_past_2_to_the_32(lib):
    """the stream's coordinates are 64-bit: a view whose first offset lies just below 2^32, and one that reaches it through 70 000 entries of one
    64 KiB frame (no memory is needed for a stream nobody reads whole)"""
    ids, _ = VIEWS["subset"]
    voff = V.offsets_of(SIZES, ids, (1 << 32) - 1000)
    r = [((1 << 32) - 1000, 3000), ((1 << 32) - 1, 2), ((1 << 32), 17), (int(voff[-1]) - 5, 5), ((1 << 32) - 1001, 1), (int(voff[0]), int(voff[-1] - voff[0]))]
    want, _ = run(lib, ids, voff, r, "shuffled", "base below 2^32")
    assert want["status"].tolist() == [0, 0, 0, 0, V.OUT_OF_RANGE, 0]
    frames = [V.payload(0, 65536), V.payload(1, 100)]
    ids = np.zeros(70000, np.uint32)
    ids[65536:65540] = [1, 0, 1, 0]
    voff = V.offsets_of([65536, 100], ids)
    assert int(voff[-1]) > (1 << 32) + (1 << 28)
    at = 1 << 32
    r = [(at - 3000, 7000), (at - 1, 2), (at, 65736), (int(voff[-1]) - 4000, 4000), (int(voff[65536]) - 10, 300), (at + 65536 * 3 - 20000, 70000)]
    want, got = run(lib, ids, voff, r, "packed", "4.6 GB stream", frames=frames)
    assert not want["status"].any() and got["decoded"] == 2


def test_bad_views_are_refused_whole(lib):
    ids, voff = VIEWS["random_300"]
    ranges = [(int(voff[10]), int(voff[20] - voff[10])), (int(voff[100]) + 1, 5)]
    for j in (12, 250):                                      # an entry that a range touches, one that none touches
        for kind in ("id", "size", "order"):
            i2, v2 = ids.copy(), voff.copy()
            if kind == "id":
                i2[j] = len(SIZES)
            elif kind == "size":
                v2[j + 1:] += np.uint64(1)
            else:
                k = next(k for k in range(j, 300) if v2[k + 1] > v2[k])
                v2[k], v2[k + 1] = v2[k + 1], v2[k]
            want, _ = run(lib, i2, v2, ranges, "packed", (kind, j))
            assert want["rc"] == V.ARGUMENT


def test_bad_ranges_get_their_code_and_neighbours_are_served(lib):
    ids, voff = VIEWS["based_12345"]
    v0, vend = int(voff[0]), int(voff[-1])
    good = V.ranges_of(voff, dense=False)[:40]
    bad = [(v0 - 1, 1), (0, 0), (vend, 1), (vend + 1, 0), (vend - 10, 11), (v0 + 5, V.U64), (V.U64, 2), (1 << 63, 1 << 63)]
    ranges = good[:15] + bad[:4] + good[15:] + bad[4:]
    for mode in ("packed", "shuffled"):
        want, _ = run(lib, ids, voff, ranges, mode, "bad ranges")
        assert [int(s) for s in want["status"] if s] == [V.OUT_OF_RANGE] * len(bad) and want["rc"] == V.OUT_OF_RANGE
    # destinations past dst_cap
    given, offs, end = V.destinations(good, "shuffled", v0=v0, vend=vend)
    cap = sorted(offs)[-3] + 1
    want, _ = run(lib, ids, voff, good, "shuffled", "dst_cap", dst_cap=cap)
    assert V.DST_TOO_SMALL in want["status"].tolist() and 0 in want["status"].tolist()


def test_failed_frames_fail_their_ranges_in_view_order(lib):
    a, b = SIZES.index(4095), SIZES.index(65537)
    err = {a: 20, b: 22}
    for name, ids in (("a then b", [3, a, 5, b, 6, 7]), ("b then a", [3, b, 5, a, 6, 7])):
        ids = np.array(ids, np.uint32)
        voff = V.offsets_of(SIZES, ids)
        ranges = [(0, int(voff[-1])), (int(voff[1]), 10), (int(voff[3]) + 5, 10), (0, int(voff[1])), (int(voff[4]), int(voff[6] - voff[4])), (int(voff[2]) - 1, 2)]
        want, _ = run(lib, ids, voff, ranges, "shuffled", name, frame_err=err)
        first, second = (err[a], err[b]) if name == "a then b" else (err[b], err[a])
        assert want["status"].tolist() == [-first, -first, -second, 0, 0, -first] and want["rc"] == -first


def test_plan_functions_literal(lib):
    l = lib
    # the chunks of a range: none up to 16 KiB; cut on the destination's 16-byte grid
    assert [l.zkv_sim_chunks(n, 0) for n in (0, 1, 16384, 16385, CHUNK, CHUNK + 1, 3 * CHUNK)] == [0, 0, 0, 1, 1, 2, 3]
    assert [l.zkv_sim_chunks(n, 5) for n in (CHUNK - 5, CHUNK - 4, 2 * CHUNK - 5, 2 * CHUNK - 4)] == [1, 2, 2, 3]
    for dst, n in ((0, 3 * CHUNK), (5, 3 * CHUNK), (15, CHUNK + 1), (1, 16385)):
        k = l.zkv_sim_chunks(n, dst)
        cuts = [(l.zkv_sim_chunk_begin(c, dst), l.zkv_sim_chunk_end(c, dst, n)) for c in range(k)]
        assert cuts[0][0] == 0 and cuts[-1][1] == n and all(x[1] == y[0] for x, y in zip(cuts, cuts[1:])), (dst, n, cuts)
        assert all((dst + b) % 16 == 0 for b, _ in cuts[1:]) and all(e - b <= CHUNK for b, e in cuts)
    # validation: below the first offset, past the end, overflow, the destination
    assert l.zkv_sim_check(100, 200, 99, 0, 10, 0) == V.OUT_OF_RANGE
    assert l.zkv_sim_check(100, 200, 100, 100, 100, 0) == 0
    assert l.zkv_sim_check(100, 200, 200, 0, 0, 0) == 0
    assert l.zkv_sim_check(100, 200, 201, 0, 0, 0) == V.OUT_OF_RANGE
    assert l.zkv_sim_check(100, 200, 150, V.U64, 0, 0) == V.OUT_OF_RANGE
    assert l.zkv_sim_check(100, 200, 150, 50, 49, 0) == V.DST_TOO_SMALL
    assert l.zkv_sim_check(100, 200, 150, 1, 10, V.U64) == V.DST_TOO_SMALL
    assert [l.zkv_sim_chunk_wgs(c, cap) for c, cap in ((1, 0), (1, CHUNK), (3, 10 * CHUNK), (1, 1 << 40))] == [2, 3, 16, 4096]


def possum(a):
    """view_san.cpp's checksum: the sum of (byte + 1) * (position * K + 1) modulo 2^64"""
    with np.errstate(over="ignore"):
        w = np.arange(len(a), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
        return int(((a.astype(np.uint64) + np.uint64(1)) * w).sum(dtype=np.uint64))


def test_kernels_under_sanitizers(tmp_path):
    """The same harness as a program of its own under AddressSanitizer + UBSan (tests/sim/view_san.cpp): exact-size heap allocations for the
    destination, every pass's scratch and every array of the plan"""
    from conftest import ROOT
    exe = str(tmp_path / "viewsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "view_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    d_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
    data = np.concatenate(FRAMES)
    a, b = SIZES.index(4095), SIZES.index(65537)
    cases = [("identity", "packed", 0, 0, None), ("reversed", "shuffled", 3, 64 << 10, None), ("thrice_interleaved", "shuffled", 1, 64 << 10, None),
             ("random_300", "packed", 7, 0, {a: 20, b: 22}), ("empty_runs", "shuffled", 15, 1, None), ("based_12345", "packed", 5, 0, None),
             ("single", "shuffled", 0, 0, None)]
    first = True
    for i, (name, mode, misalign, pass_bytes, err) in enumerate(cases):
        ids, voff = VIEWS[name]
        ranges = V.ranges_of(voff, dense=False)
        ranges += [(int(voff[0]) - 1, 1) if int(voff[0]) else (int(voff[-1]), 1), (int(voff[-1]) + 1, 0)]
        given, offs, end = V.destinations(ranges, mode, v0=int(voff[0]), vend=int(voff[-1]))
        o, n = np.array([r[0] for r in ranges], np.uint64), np.array([r[1] for r in ranges], np.uint64)
        ferr = np.zeros(len(SIZES), np.int32)
        for f, code in (err or {}).items():
            ferr[f] = code
        arrays = dict(data=data, doff=d_off, ids=ids, voff=voff, offs=o, lens=n)
        if given is not None:
            arrays["dst"] = np.array(given, np.uint64)
        if err:
            arrays["err"] = ferr
        paths = {}
        for k, arr in arrays.items():
            paths[k] = str(tmp_path / ("%s%d" % (k, i)))
            with open(paths[k], "wb") as f:
                f.write(np.ascontiguousarray(arr).tobytes())
        r = subprocess.run([exe, str(misalign), str(pass_bytes), str(end), str(end), paths["data"], paths["doff"], paths["ids"], paths["voff"], paths["offs"],
                            paths["lens"], paths.get("dst", "-"), paths.get("err", "-")], capture_output=True, text=True, timeout=900)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (name, r.stdout[-300:], r.stderr[-3000:])
        m = V.model(FRAMES, ids, voff, o, n, given, end, end, frame_err=err, failed_fill=0xEE if err else None)
        h = possum(m["dst"]) ^ ((possum(np.frombuffer(m["status"].tobytes(), np.uint8)) << 1) & V.U64)
        out = r.stdout.split()
        assert out[0] == str(m["rc"]) and out[1] == str(len(m["decoded"])) and out[3] == "%016x" % h, (name, r.stdout, m["rc"], len(m["decoded"]))

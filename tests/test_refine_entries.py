"""zk_refine_entries on the CPU: the entry walk (zk_split_entry, zeekstd_amd/csrc/zk_refine.h -- the lane code zk_k_refine_split runs)
against a pure-Python splitter and libzstd 1.5.7 on archives whose entries are chains of frames (tests/helpers/entry_inputs.py), the
walker's rule for skippable-frame entries through the simulation library, and the walk under sanitizers.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sim_decode
from helpers import entry_inputs as EI
from helpers import sim_refine as SR

ARCHIVES = [mk.__name__ for mk in EI.GOOD]


def _archive(name):
    return next(mk for mk in EI.GOOD if mk.__name__ == name)()


def _same_split(a):
    buf = SR.padded(a.comp)
    for e in range(len(a.c) - 1):
        cb, ce = int(a.c[e]), int(a.c[e + 1])
        got, stop = SR.split(buf, cb, ce)
        want, why = EI.split(a.comp, cb, ce)
        assert got == want and (stop == 0) == (why is None), (a.name, e, stop, why)
        yield e, got, stop, why


@pytest.mark.parametrize("name", ARCHIVES)
def test_split_entry_finds_the_frames_the_python_splitter_finds(name):
    a = _archive(name)
    n = 0
    for e, got, stop, _ in _same_split(a):
        assert stop == 0 and len(got) == len(a.pieces[e])
        n += len(got)
    r = EI.refined(a)
    assert not r.bad and not r.lax and len(r.c) - 1 == n and np.array_equal(np.diff(r.d.astype(np.int64)), [len(p.data) for e in a.pieces for p in e])
    if name == "identity":
        assert np.array_equal(r.c, a.c) and np.array_equal(r.d, a.d)
    if name == "coarse":
        assert n > 1024                                      # the counts cross a scan workgroup's width
    if name == "plain":
        assert a.d is None and r.d[0] == 0 and int(r.d[-1]) == len(EI.plain_bytes(a))


def test_split_entry_on_damaged_entries_agrees_with_the_python_splitter_and_libzstd():
    """where structure alone decides -- the walk stops -- libzstd does not reach the end of the entry either; the damage done by hand gets the
    verdict it was made for; and the flipped bits leave enough entries on either side"""
    a, what = EI.damaged()
    r = EI.refined(a)
    stops = {}
    for e, got, stop, why in _same_split(a):
        if stop:
            stops[e] = stop
            out, state = EI.libzstd_verdict(a.comp[int(a.c[e]):int(a.c[e + 1])])
            assert state != "end", (e, why, state)
    by_name = {n: e for e, n in what.items() if n != "flip"}
    assert by_name["good"] not in r.bad and all(e in r.bad for n, e in by_name.items() if n != "good")
    assert by_name["size_wrong"] not in stops and by_name["size_wrong"] not in r.bad_deep         # whole frames: only the table's size is wrong
    for n in ("junk1", "junk2", "junk3", "truncated", "skip_past", "skip_short"):
        assert stops[by_name[n]] == 72, n                   # srcSize_wrong
    for n in ("junk4", "junk9", "junk40"):
        assert stops[by_name[n]] == 10, n                   # neither magic ... which is the ENTRY's srcSize_wrong behind a complete frame
        assert SR.lib().zk_sim_refine_verdict(len(a.pieces[by_name[n]]) - 1, 10) == 72
    assert SR.lib().zk_sim_refine_verdict(0, 10) == 10 and SR.lib().zk_sim_refine_verdict(3, 20) == 20
    flips = [e for e, n in what.items() if n == "flip"]
    refused = [e for e in flips if EI.entry_verdict(a, e) is None]
    assert len(refused) >= 20 and len(flips) - len(refused) >= 20, (len(refused), len(flips))
    assert set(refused) == {e for e in flips if e in r.bad}
    # a bad entry stays ONE refined entry with its own range
    for e in r.bad:
        j = np.flatnonzero(r.entry_of == e)
        assert len(j) == 1 and r.c[j[0]] == a.c[e] and r.c[j[0] + 1] == a.c[e + 1]


def test_the_lane_code_decodes_the_refined_table_where_libzstd_decodes_the_entry():
    """DAMAGED, refined as expected, through the decoder's lane code on the CPU: an entry libzstd accepts decodes to libzstd's bytes, every
    other entry has a failing piece -- and so may one that libzstd decodes although it is not valid Zstandard (Refined.lax: the
    format_refuses case of oracle/libzstd_ref.py's judge_damaged)"""
    a, _ = EI.damaged()
    r = EI.refined(a)
    frames = list(zip(np.diff(r.c.astype(np.int64)).tolist(), np.diff(r.d.astype(np.int64)).tolist()))
    rc, out, st = sim_decode(a.comp, frames)
    failed = {int(r.entry_of[j]) for j in np.flatnonzero(st)}
    assert failed >= r.bad and failed - r.bad <= r.lax, (sorted(r.bad - failed), sorted(failed - r.bad - r.lax))
    assert len(r.lax) < 10
    for e in range(len(a.c) - 1):
        if e not in failed:
            assert out[int(a.d[e]):int(a.d[e + 1])] == EI.entry_verdict(a, e), e


def test_walker_takes_a_skippable_frame_as_an_entry_of_size_zero():
    """zk_walk_frame through tests/sim/libzk_sim.so: status 0 and nothing written, whatever the magic's nibble and the content's size"""
    P = EI.pool()
    for s in EI.skips():
        comp = P[0].comp + s.comp + P[1].comp
        frames = [(len(P[0].comp), len(P[0].data)), (len(s.comp), 0), (len(P[1].comp), len(P[1].data))]
        rc, out, st = sim_decode(comp, frames)
        assert rc == 0 and not st.any() and out == P[0].data + P[1].data
    s = EI.skips()[4]
    rc, out, st = sim_decode(s.comp, [(len(s.comp), 0)])
    assert rc == 0 and st[0] == 0 and out == b""


def test_walker_refuses_a_skippable_entry_whose_size_field_or_table_size_is_wrong():
    P, s = EI.pool(), EI.skips()[4]                         # 100 bytes of content
    for comp, size in ((s.comp[:-1], 0), (s.comp + b"\0", 0), (s.comp[:7], 0), (s.comp[:4] + struct.pack("<I", 0xFFFFFFFF) + s.comp[8:], 0)):
        rc, out, st = sim_decode(P[0].comp + comp, [(len(P[0].comp), len(P[0].data)), (len(comp), size)])
        assert st.tolist() == [0, 72] and out[:len(P[0].data)] == P[0].data, len(comp)
    rc, out, st = sim_decode(s.comp, [(len(s.comp), 5)])
    assert st.tolist() == [20]
    # a first word that is neither magic stays prefix_unknown
    rc, out, st = sim_decode(b"\x51\x2A\x4D\x17" + s.comp[4:], [(len(s.comp), 0)])
    assert st.tolist() == [10]


def test_split_entry_under_sanitizers(tmp_path):
    """tests/sim/entry_split_fuzz.cpp: a stand-alone program built with AddressSanitizer + UBSan runs the lane code over a few thousand mutated
    and truncated entries of COARSE and SKIPS, every entry an exact-size heap allocation"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "splitfuzz")
    src = os.path.join(ROOT, "tests", "sim", "entry_split_fuzz.cpp")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    for k, a in enumerate((EI.head(EI.coarse(), 12), EI.skip_entries())):
        path = str(tmp_path / (a.name + ".bin"))
        with open(path, "wb") as f:
            f.write(struct.pack("<IQ", len(a.c) - 1, len(a.comp)))
            f.write(np.diff(a.c.astype(np.int64)).astype("<u8").tobytes())
            f.write(a.comp)
        r = subprocess.run([exe, path, "3000", str(11 + k)], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
        assert int(r.stdout.split()[3]) > 500               # the mutations do reach the walk's refusals

"""The decoder's lane code on the CPU with a dictionary (tests/sim/zk_sim_dict.cpp: frame walk -> Huffman -> sequence decode -> execution,
the dictionary's tables reached through its block entry, zk_dict.h): every frame of tests/golden/dict_archives.* bit-exact, and the
statuses around a dictionary.  What can be checked of the decode path on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import dict_fixtures as df

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX, BLOB = df.load()
CASES = {c["name"]: c for c in IDX["cases"]}


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(ROOT, "tests", "sim", "zk_sim_dict.cpp")
    so = os.path.join(ROOT, "tests", "sim", "libzk_sim_dict.so")
    hdrs = [os.path.join(ROOT, "zeekstd_amd", "csrc", h) for h in ("zk_device.h", "zk_dict.h")]
    if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.zk_sim_dict_decode.restype = C.c_int
    lib.zk_sim_dict_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def dict_bytes(name):
    ent = IDX["dicts"][name]
    if "of" in ent:
        return df.patch_reps(dict_bytes(ent["of"]), ent["header_size"], ent["reps"])
    return df.piece(BLOB, ent)


def run(sim, case, dictionary):
    comp, c, d = df.archive(BLOB, case)
    c, d = np.asarray(c, np.uint64), np.asarray(d, np.uint64)
    buf = np.frombuffer(comp + b"\0" * 8, np.uint8)
    out = np.full(int(d[-1]) + 1, 0x5A, np.uint8)
    st = np.full(len(c) - 1, -1, np.int32)
    db = np.frombuffer(dictionary, np.uint8) if dictionary else None
    rc = sim.zk_sim_dict_decode(buf.ctypes.data, len(comp), c.ctypes.data, d.ctypes.data, len(c) - 1, db.ctypes.data if dictionary else None,
                                len(dictionary) if dictionary else 0, out.ctypes.data, st.ctypes.data)
    assert rc == 0
    return out[:int(d[-1])].tobytes(), st, d


def want(case):
    return b"".join(bytes.fromhex(fr["expect"]) if "expect" in fr else df.plain(fr["recipe"]) for fr in case["frames"])


@pytest.mark.parametrize("name", list(CASES))
def test_every_fixture_frame_bit_exact(sim, name):
    case = CASES[name]
    out, st, _ = run(sim, case, dict_bytes(case["dict"]))
    assert not st.any(), (np.flatnonzero(st)[:5], st[st != 0][:5])
    assert out == want(case)


def test_statuses_around_a_dictionary(sim):
    mixed = [32 if i % 2 == 0 else 0 for i in range(len(CASES["mixed"]["frames"]))]
    # none loaded: as ever
    assert (run(sim, CASES["trained"], None)[1] == 32).all()
    assert (run(sim, CASES["no_id"], None)[1] == 20).all()
    out, st, d = run(sim, CASES["mixed"], None)
    assert list(st) == mixed
    data = want(CASES["mixed"])
    assert all(out[int(d[i]):int(d[i + 1])] == data[int(d[i]):int(d[i + 1])] for i in range(1, len(st), 2))
    # another ID: those frames only
    d0 = dict_bytes("trained")
    other = d0[:4] + (IDX["dicts"]["trained"]["id"] ^ 0x55).to_bytes(4, "little") + d0[8:]
    assert list(run(sim, CASES["mixed"], other)[1]) == mixed
    # raw content lends no tables, and has no ID
    assert (run(sim, CASES["no_id"], dict_bytes("raw"))[1] == 20).all()
    assert (run(sim, CASES["trained"], dict_bytes("raw"))[1] == 32).all()


def test_repeat_offsets_are_the_dictionarys(sim):
    """the hand-made frames under the unpatched dictionary: what libzstd recorded for it, not what the patched one gives"""
    case = CASES["rep"]
    out, st, d = run(sim, case, dict_bytes("trained"))
    for i, fr in enumerate(case["frames"]):
        if isinstance(fr["unpatched"], str):
            assert st[i] == 0 and out[int(d[i]):int(d[i + 1])] == bytes.fromhex(fr["unpatched"]) != bytes.fromhex(fr["expect"])
        else:
            assert st[i] == fr["unpatched"]

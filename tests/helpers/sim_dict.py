"""TEST INFRASTRUCTURE -- loader of tests/sim/zk_sim_dict.cpp (the decoder's lane code on the CPU with a dictionary; tests/test_sim_dict.py
builds the same library the same way) and a call that decodes a list of frames with it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "sim", "zk_sim_dict.cpp")
        so = os.path.join(ROOT, "tests", "sim", "libzk_sim_dict.so")
        hdrs = [os.path.join(ROOT, "zeekstd_amd", "csrc", h) for h in ("zk_device.h", "zk_dict.h")]
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        l = C.CDLL(so)
        l.zk_sim_dict_decode.restype = C.c_int
        l.zk_sim_dict_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        _LIB = l
    return _LIB


def decode(comp, sizes, dictionary):
    """comp: the frames back to back, sizes: [(compressed size, decoded size)] -> (return code, decoded bytes, statuses)"""
    c = np.concatenate([[0], np.cumsum([s[0] for s in sizes])]).astype(np.uint64)
    d = np.concatenate([[0], np.cumsum([s[1] for s in sizes])]).astype(np.uint64)
    buf = np.frombuffer(bytes(comp) + b"\0" * 8, np.uint8)
    out = np.full(int(d[-1]) + 1, 0x5A, np.uint8)
    st = np.full(len(sizes), -1, np.int32)
    db = np.frombuffer(bytes(dictionary), np.uint8) if dictionary else None
    rc = lib().zk_sim_dict_decode(buf.ctypes.data, len(comp), c.ctypes.data, d.ctypes.data, len(sizes), db.ctypes.data if dictionary else None,
                                  len(dictionary) if dictionary else 0, out.ctypes.data, st.ctypes.data)
    assert out[int(d[-1])] == 0x5A
    return rc, out[:int(d[-1])].tobytes(), st

"""TEST INFRASTRUCTURE -- loader of tests/sim/zk_refine_sim.cpp (zk_split_entry, the entry walk of zk_refine_entries, on the CPU), built on
demand the way tests/helpers/sim_dict.py builds its library, and a call that splits one entry with it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(ROOT, "tests", "sim", "zk_refine_sim.cpp")
        so = os.path.join(ROOT, "tests", "sim", "libzk_refine_sim.so")
        hdrs = [os.path.join(ROOT, "zeekstd_amd", "csrc", h) for h in ("zk_device.h", "zk_refine.h")]
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in [src] + hdrs) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        l = C.CDLL(so)
        l.zk_sim_split_entry.restype = C.c_uint32
        l.zk_sim_split_entry.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        l.zk_sim_refine_verdict.restype = C.c_uint32
        l.zk_sim_refine_verdict.argtypes = [C.c_uint32, C.c_uint32]
        _LIB = l
    return _LIB


def padded(comp):
    """the bytes + ZK_COMP_PADDING as a numpy array (keep it alive across the calls)"""
    return np.frombuffer(bytes(comp) + b"\0" * 8, np.uint8)


def split(buf, begin, end):
    """zk_split_entry on buf[begin, end) in both modes -> (first bytes of the pieces, stop code); the count and emit passes must agree"""
    stop = C.c_uint32()
    n = lib().zk_sim_split_entry(buf.ctypes.data, begin, end, None, C.byref(stop))
    starts = np.full(n + 1, 0xDEADBEEF, np.uint64)
    stop2 = C.c_uint32()
    n2 = lib().zk_sim_split_entry(buf.ctypes.data, begin, end, starts.ctypes.data, C.byref(stop2))
    assert (n2, stop2.value) == (n, stop.value) and starts[n] == 0xDEADBEEF
    return [int(x) for x in starts[:n]], stop.value

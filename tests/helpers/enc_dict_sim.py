"""TEST INFRASTRUCTURE -- loader of tests/sim/zk_enc_dict_sim.cpp (the host side of encoding against a dictionary, zeekstd_amd/csrc/zk_enc_dict.h,
on the CPU), the calls into it, the fixture dictionaries, and the rules restated in Python for the comparison.  Used by
tests/test_enc_dict_rules.py; nothing of the product imports this."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import dict_fixtures as D

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_enc_dict_sim.cpp")] + [os.path.join(CSRC, h) for h in ("zk_enc_dict.h", "zk_dict.h", "zk_enc_device.h", "zk_device.h")]
_LIB = None
COST_NONE = 0xFFFFFFFF
NOT_LEGAL = (1 << 64) - 1
PREDEF, OWN, DICT = 0, 1, 2
LL, OF, ML = 0, 1, 2
NSYM = (36, 32, 53)
FSE_MIN_SEQ, DESC_CAP = 256, 80
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
          -1, -1, -1, -1, -1, -1, -1]
PREDEF_NORMS = ((LL_DEF, 6), (OF_DEF, 5), (ML_DEF, 6))


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_enc_dict_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_enc_dict_sim_id_width.restype = C.c_uint32
        l.zk_enc_dict_sim_id_width.argtypes = [C.c_uint32]
        l.zk_enc_dict_sim_sym_cost.restype = C.c_uint32
        l.zk_enc_dict_sim_sym_cost.argtypes = [C.c_int, C.c_int]
        l.zk_enc_dict_sim_pick.restype = C.c_int
        l.zk_enc_dict_sim_pick.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64]
        l.zk_enc_dict_sim_treeless_size.restype = C.c_uint32
        l.zk_enc_dict_sim_treeless_size.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.zk_enc_dict_sim_build.restype = C.c_int
        l.zk_enc_dict_sim_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        l.zk_enc_dict_sim_huf_weights.restype = C.c_int
        l.zk_enc_dict_sim_huf_weights.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        l.zk_enc_dict_sim_huf_roundtrip.restype = C.c_int
        l.zk_enc_dict_sim_huf_roundtrip.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]
        l.zk_enc_dict_sim_fse_roundtrip.restype = C.c_int
        l.zk_enc_dict_sim_fse_roundtrip.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32]
        l.zk_enc_dict_sim_choose.restype = C.c_int
        l.zk_enc_dict_sim_choose.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        _LIB = l
    return _LIB


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(1, np.uint8)


# ---------------------------------------------------------------------------------------------- the fixture dictionaries
def fixture_dicts():
    """{"trained" | "patched" | "raw": bytes} of tests/golden/dict_archives.*"""
    idx, blob = D.load()
    ds = idx["dicts"]
    trained = D.piece(blob, ds["trained"])
    return {"trained": trained, "patched": D.patch_reps(trained, ds["patched"]["header_size"], tuple(ds["patched"]["reps"])), "raw": D.piece(blob, ds["raw"])}


# ---------------------------------------------------------------------------------------------- calls
def build(d):
    """-> None for a raw-content dictionary, else {"len": [256], "code": [256], "cost": [3][64], "al": [3], "maxbits"} as zk_cdict_create builds them"""
    buf = _u8(d)
    ln, code = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    cost, al, mb = np.zeros((3, 64), np.uint32), np.zeros(3, np.uint32), C.c_uint32()
    rc = lib().zk_enc_dict_sim_build(buf.ctypes.data, len(d), ln.ctypes.data, code.ctypes.data, cost.ctypes.data, al.ctypes.data, C.byref(mb))
    if rc == -1:
        return None
    assert rc == 0, rc
    return {"len": ln.tolist(), "code": code.tolist(), "cost": cost.tolist(), "al": al.tolist(), "maxbits": mb.value}


def decoder_weights(d):
    """-> (weights[256], number of symbols, maxbits) as zk_huf_read_weights derives them from the dictionary's tree description"""
    buf, w, n, mb = _u8(d), np.zeros(256, np.uint8), C.c_uint32(), C.c_uint32()
    assert lib().zk_enc_dict_sim_huf_weights(buf.ctypes.data, len(d), w.ctypes.data, C.byref(n), C.byref(mb)) == 0
    return w.tolist(), n.value, mb.value


def huf_roundtrip(d, lits):
    buf, l = _u8(d), _u8(lits)
    return lib().zk_enc_dict_sim_huf_roundtrip(buf.ctypes.data, len(d), l.ctypes.data, len(lits))


def fse_roundtrip(d, t, syms):
    buf, s = _u8(d), _u8(bytes(syms))
    return lib().zk_enc_dict_sim_fse_roundtrip(buf.ctypes.data, len(d), t, s.ctypes.data, len(syms))


def choose(hist, t, nseq, n_blocks, cost_dict, dict_al):
    """-> (pick, [cost predefined, own, dictionary] with NOT_LEGAL where a choice is not legal, bytes of the own description)"""
    h, c = np.zeros(64, np.uint32), np.array(cost_dict, np.uint32)
    h[:len(hist)] = hist
    costs, dlen = np.zeros(3, np.uint64), C.c_uint32()
    pick = lib().zk_enc_dict_sim_choose(h.ctypes.data, t, nseq, n_blocks, c.ctypes.data, dict_al, costs.ctypes.data, C.byref(dlen))
    return pick, [int(x) for x in costs], dlen.value


def treeless_size(nlit, bits):
    b, z, head = np.array(bits, np.uint64), np.zeros(4, np.uint32), np.zeros(8, np.uint8)
    sz = lib().zk_enc_dict_sim_treeless_size(nlit, b.ctypes.data, z.ctypes.data, head.ctypes.data)
    return sz, z.tolist(), bytes(head[:5])


# ---------------------------------------------------------------------------------------------- the rules restated
def id_width(i):
    return 0 if i == 0 else 1 if i < 1 << 8 else 2 if i < 1 << 16 else 4


def sym_cost(norm, al):
    """-log2(norm / 2^al) in 1/256 bit by eight squarings of the mantissa (integers only)"""
    if norm == 0:
        return COST_NONE
    p = 1 if norm < 0 else norm
    hb = p.bit_length() - 1
    x, frac = p << (16 - hb), 0
    for i in range(7, -1, -1):
        x = (x * x) >> 16
        if x >= 2 << 16:
            frac |= 1 << i
            x >>= 1
    return (al << 8) - ((hb << 8) | frac)


def table_cost(hist, cost):
    """cost of the counted codes under a table of per-symbol costs, None where a counted code has none: the brute-force legality rule"""
    total = 0
    for s, n in enumerate(hist):
        if n:
            if s >= len(cost) or cost[s] == COST_NONE:
                return None
            total += n * cost[s]
    return total


def overhead(desc_bytes, al, n_blocks):
    return (desc_bytes * 8 + al * n_blocks) << 8


def pick(c_predef, c_own, c_dict):
    """the minimum of the legal choices (None = not legal); ties: the other routes' choice (own where legal, else predefined), then
    predefined, then the dictionary's"""
    order = [(OWN, c_own), (PREDEF, c_predef), (DICT, c_dict)] if c_own is not None else [(PREDEF, c_predef), (DICT, c_dict)]
    best = None
    for which, c in order:
        if c is not None and (best is None or c < best[1]):
            best = (which, c)
    return best[0]

"""The host writer of a trained dictionary's header (zeekstd_amd/csrc/zk_train_host.h: zkt_write_header) alone, on the CPU, through
tests/sim/zk_train_hdr_sim.cpp.  For histograms of every kind the bytes it writes, with some content behind them, are a dictionary that
zk_dict_create accepts, that libzstd 1.5.7 loads for decoding and for encoding (skipped where 1.5.7 is absent, as tests/test_dict.py does),
and that the decoder's own parsers read back to tables in which every literal value and every code is present; the ID is the caller's and
the repeat offsets are 1 / 4 / 8."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import dict_fixtures as df
from helpers import libzstd_dict
from oracle import libzstd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_train_hdr_sim.cpp")] + [os.path.join(CSRC, h) for h in ("zk_train_host.h", "zk_enc_device.h", "zk_dict.h", "zk_device.h")]
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_train_hdr_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_train_hdr_sim_write.restype = C.c_uint64
        l.zk_train_hdr_sim_write.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_int), C.c_uint32]
        l.zk_train_hdr_sim_parse.restype = C.c_int
        l.zk_train_hdr_sim_parse.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + [C.POINTER(C.c_uint64)]
        l.zk_train_hdr_sim_xxh64.restype = C.c_uint64
        l.zk_train_hdr_sim_xxh64.argtypes = [C.c_char_p, C.c_uint64]
        l.zk_train_hdr_sim_id.restype = C.c_uint32
        l.zk_train_hdr_sim_id.argtypes = [C.c_char_p, C.c_uint64]
        _LIB = l
    return _LIB


def derived_id(content):
    """the ID rule: 32768 + XXH64(content) mod (2^31 - 65536), from the oracle's XXH64"""
    from oracle import zko
    return 32768 + zko.xxh64(bytes(content)) % ((1 << 31) - 65536)


def write(lit, ll, ml, of, dict_id, cap=512, desc_limit=128):
    h = [np.ascontiguousarray(x, np.uint64) for x in (lit, ll, ml, of)]
    assert [len(x) for x in h] == [256, 36, 53, 32]
    out = np.full(cap + 16, 0xA5, np.uint8)
    rb = C.c_int(-1)
    n = lib().zk_train_hdr_sim_write(*[x.ctypes.data for x in h], dict_id, out.ctypes.data, cap, C.byref(rb), desc_limit)
    assert (out[cap:] == 0xA5).all()
    return out[:n].tobytes(), rb.value


def parse(d):
    buf = np.frombuffer(d, np.uint8)
    w, norm = np.zeros(256, np.uint8), np.zeros((3, 64), np.int16)
    mb, nsym, al, reps, did, co = C.c_uint32(), np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.uint32), C.c_uint32(), C.c_uint64()
    rc = lib().zk_train_hdr_sim_parse(buf.ctypes.data, len(d), w.ctypes.data, C.byref(mb), norm.ctypes.data, nsym.ctypes.data, al.ctypes.data,
                                      reps.ctypes.data, C.byref(did), C.byref(co))
    assert rc == 0, rc
    return w, mb.value, norm, nsym, al, reps.tolist(), did.value, co.value


def _measured():
    text = np.frombuffer(df.records(1, 40000), np.uint8)
    lit = np.bincount(text, minlength=256)
    ll = [int(9000 * 0.7 ** i) for i in range(36)]
    ml = [int(7000 * 0.8 ** i) for i in range(53)]
    of = [0, 3, 10, 40, 90, 200, 500, 900, 1500, 2500, 3000, 2800, 2000, 900, 100] + [0] * 17
    return lit, ll, ml, of


def _one(i, n, v=1):
    a = [0] * n
    a[i] = v
    return a


HISTS = {
    "measured": _measured(),
    "all_zero": ([0] * 256, [0] * 36, [0] * 53, [0] * 32),
    "one_literal": (_one(101, 256, 77777), _one(0, 36, 5), _one(1, 53, 5), _one(2, 32, 5)),
    "two_to_the_31": (_one(0, 256, 1 << 31), _one(35, 36, 1 << 31), _one(52, 53, 1 << 31), _one(30, 32, 1 << 31)),
    "huge": (_one(255, 256, 1 << 62), _one(3, 36, 1 << 63), [1 << 40] * 53, [(1 << 50) + i for i in range(32)]),
    "uniform": ([1000] * 256, [10] * 36, [10] * 53, [10] * 32),
    # code lengths spread over 6 ... 11: many different weights, a long FSE form of them (it still fits: see test_the_paths_...)
    "spread": ([1 << (22 - (i * 11) // 256 * 2) for i in range(256)], list(range(1, 37)), list(range(1, 54)), list(range(1, 33))),
}


@pytest.fixture(scope="module")
def zstd():
    return libzstd_ref.load("1.5.7")


@pytest.mark.parametrize("name", list(HISTS))
def test_header_is_a_dictionary_every_reader_takes(name, zstd):
    every_reader_takes(name, zstd, 128)


@pytest.mark.parametrize("name,limit", [("measured", 50), ("measured", 30), ("spread", 50), ("spread", 40), ("measured", 12)])
def test_flattened_tree_is_a_dictionary_every_reader_takes(name, limit, zstd):
    """The flatten-and-retry path.  No histogram found makes the weights' FSE form reach the format's 128 bytes (see
    test_the_paths_the_inputs_are_there_for), so the writer takes the limit as a parameter and the test lowers it below what the histogram's
    first tree needs: the counts are flattened and the tree is built again until its description fits, and the result passes every reader"""
    lit, ll, ml, of = HISTS[name]
    first = write(lit, ll, ml, of, 1)[0]
    assert first[8] >= limit, (first[8], "the first tree's description already fits: lower the limit")
    hdr, rebuilds = every_reader_takes(name, zstd, limit)
    assert rebuilds >= 1 and hdr[8] < limit


def every_reader_takes(name, zstd, desc_limit):
    lit, ll, ml, of = HISTS[name]
    dict_id = 40000 + len(name)
    hdr, rebuilds = write(lit, ll, ml, of, dict_id, desc_limit=desc_limit)
    assert 8 + 12 < len(hdr) <= 512 and rebuilds >= 0
    content = df.records(3, 300)
    d = hdr + content
    # the engine's own reader
    h = zk.Dictionary(d)
    assert h.id == dict_id and h.content_offset == len(hdr)
    assert d[:8] == (0xEC30A437).to_bytes(4, "little") + dict_id.to_bytes(4, "little")
    # read back by the decoder's parsers: every literal value has a weight (code lengths <= 11, Kraft sum 1), every code a probability
    w, maxbits, norm, nsym, al, reps, did, co = parse(d)
    assert (w > 0).all() and maxbits <= 11 and int((1 << (w.astype(np.int64) - 1)).sum()) == 1 << maxbits
    assert reps == [1, 4, 8] and did == dict_id and co == len(hdr)
    for t, (n, log) in enumerate(((36, 9), (31, 8), (53, 9))):          # LL, OF, ML
        assert nsym[t] == n and al[t] == log, (t, nsym[t], al[t])
        assert (norm[t, :n] >= 1).all() and int(norm[t, :n].sum()) == 1 << log
    # libzstd 1.5.7, both directions
    if zstd is None:
        if desc_limit != 128:
            return hdr, rebuilds
        pytest.skip("libzstd 1.5.7 is not in this image")
    j = libzstd_dict.Judge(zstd)
    assert j.load_dictionary(d) == 0
    j.close()
    zstd.ZSTD_createCCtx.restype = C.c_void_p
    zstd.ZSTD_CCtx_loadDictionary.restype = C.c_size_t
    zstd.ZSTD_CCtx_loadDictionary.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    zstd.ZSTD_compress2.restype = C.c_size_t
    zstd.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    zstd.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    cctx = C.c_void_p(zstd.ZSTD_createCCtx())
    try:
        n = zstd.ZSTD_CCtx_loadDictionary(cctx, d, len(d))
        assert not zstd.ZSTD_isError(n), zstd.ZSTD_getErrorCode(n)
        src = df.records(4, 600)
        out = C.create_string_buffer(2048)
        n = zstd.ZSTD_compress2(cctx, out, 2048, src, len(src))             # (the tables are built from the dictionary at the first use)
        assert not zstd.ZSTD_isError(n), zstd.ZSTD_getErrorCode(n)
        j = libzstd_dict.Judge(zstd)
        assert j.using_dict(out.raw[:n], 1024, d) == src
        j.close()
    finally:
        zstd.ZSTD_freeCCtx(cctx)
    return hdr, rebuilds


def test_the_paths_the_inputs_are_there_for():
    """measured counts are written at the first build; a uniform histogram has one weight throughout and is built a second time with one
    count raised; a destination too small is refused.  The flatten-and-retry path (a description above 127 bytes) is not reached by any
    histogram found at the format's limit (test_flattened_tree_... lowers the limit): 255 weights of at most 12 values hold at most 255 * log2(12) / 8 = 114 bytes of information and the counts' description
    about ten more, and code lengths that satisfy Kraft's equality are far from equiprobable -- the widest spread here takes one build, and its description 54 bytes."""
    assert write(*HISTS["measured"], 1)[1] == 0
    assert write(*HISTS["uniform"], 1)[1] == 1
    assert write(*HISTS["all_zero"], 1)[1] == 1
    hdr, rebuilds = write(*HISTS["spread"], 1)
    assert rebuilds == 0 and len(set(parse(hdr + b"x" * 64)[0].tolist())) >= 6
    assert write(*HISTS["measured"], 1, cap=100)[0] == b""
    a, b = write(*HISTS["measured"], 7), write(*HISTS["measured"], 7)
    assert a == b


def test_derived_id_rule():
    from oracle import zko
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 100, 5000):
        c = df.records(n + 1, n)
        assert lib().zk_train_hdr_sim_xxh64(c, n) == zko.xxh64(c), n
        got = lib().zk_train_hdr_sim_id(c, n)
        assert got == derived_id(c) and 32768 <= got < (1 << 31) - 32768

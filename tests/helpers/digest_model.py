"""Content digests of frames (zk_frame_digests[_dev], zk_archive_digests_dev, include/zeekstd_amd.h "THE DIGEST"): the rule in hashlib, the frame
lists the CPU and GPU tests run, and the kernels of zeekstd_amd/csrc/zk_digest.h under the workgroup emulator (tests/sim/zk_digest_sim.cpp)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")

SHA256, BLAKE2S_TREE = 1, 2                                 # ZK_DIGEST_*
ALGOS = {"sha256": SHA256, "blake2s-tree": BLAKE2S_TREE}
LEAF = 4096
POISON = 0xA5
ARGUMENT = -2003                                            # ZK_ERR_ARGUMENT
FRAME_INDEX_TOO_LARGE = -1002

EMPTY_SHA256 = "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
EMPTY_TREE = "f516be67ca647aaa6b225e5844e35af8e4a7073cd445f0a41b3ba2a5d0584aa4"
TREE_4097 = "66d4770bed3555ad5838c35af7753df322a55172a6309c3a949d06919122f201"     # the 4097 bytes i & 255

# SHA-256's padding edges; BLAKE2s's block and leaf edges (a multiple of 64 keeps its last block for the final flag, two leaves make a root input of
# exactly one block); a whole wave of leaves and one more; a list of leaves that crosses a workgroup of leaf lanes, its root input 128.5 blocks
PAD_EDGES = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128]
LEAF_EDGES = [4095, 4096, 4097, 8191, 8192, 8193]
WAVE_EDGES = [4096 * 64, 4096 * 64 + 1, 4096 * 257 + 5]
MISALIGN = (0, 1, 3, 15)


def tree(m, L=LEAF):
    n = max(1, -(-len(m) // L))
    inner = b"".join(hashlib.blake2s(m[k * L:(k + 1) * L], digest_size=32, fanout=0, depth=2, leaf_size=L, node_offset=k,
                                     node_depth=0, inner_size=32, last_node=(k == n - 1)).digest() for k in range(n))
    return hashlib.blake2s(inner, digest_size=32, fanout=0, depth=2, leaf_size=L, node_offset=0, node_depth=1,
                           inner_size=32, last_node=True).digest()


def digest(algo, m):
    m = bytes(m)
    return hashlib.sha256(m).digest() if ALGOS.get(algo, algo) == SHA256 else tree(m)


def model(algo, data, off):
    """-> np.uint8[count, 32]: the digests of data[off[i]:off[i + 1]]"""
    data = np.ascontiguousarray(data, np.uint8)
    off = [int(x) for x in off]
    out = np.zeros((len(off) - 1, 32), np.uint8)
    for i in range(len(off) - 1):
        out[i] = np.frombuffer(digest(algo, data[off[i]:off[i + 1]].tobytes()), np.uint8)
    return out


def _list(lengths, seed):
    lengths = np.asarray(lengths, np.uint64)
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.random.default_rng(seed).integers(0, 256, int(off[-1]), dtype=np.uint8)
    return data, off


_LISTS = None


def lists():
    """name -> (data, off): off[0] == 0; the tests shift and misalign them"""
    global _LISTS
    if _LISTS is None:
        rng = np.random.default_rng(20261021)
        L = {"one_frame": _list([4097], 1), "one_empty": _list([0], 2), "empty_300": _list([0] * 300, 3)}
        L["one_frame"][0][:] = np.arange(4097) & 255        # the header's literal
        for n in (63, 64, 65, 257):
            L["short_%d" % n] = _list(rng.integers(0, 131, n), 10 + n)
        edges = np.array(PAD_EDGES + LEAF_EDGES)
        L["edges"] = _list(rng.permutation(edges), 4)                                        # (the list the misalignments run on)
        L["edges_waves"] = _list(rng.permutation(np.array(PAD_EDGES + LEAF_EDGES + WAVE_EDGES)), 5)
        _LISTS = L
    return _LISTS


_WANT = {}


def want(algo, name):
    """the model's digests of a list, computed once"""
    key = (ALGOS.get(algo, algo), name)
    if key not in _WANT:
        data, off = lists()[name]
        _WANT[key] = model(key[0], data, off)
        _WANT[key].setflags(write=False)
    return _WANT[key]


# ---------------------------------------------------------------- the kernels under the emulator
_LIB = None


def build_sim(out_dir):
    """tests/sim/zk_digest_sim.cpp compiled with g++ into out_dir (a temporary directory of the test's)"""
    global _LIB
    if _LIB is None:
        so = os.path.join(str(out_dir), "libzk_digest_sim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(SIM, "zk_digest_sim.cpp")])
        l = C.CDLL(so)
        l.zk_digest_sim.restype = C.c_int
        l.zk_digest_sim.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
        l.zk_digest_sim_long_sha256.restype = None
        l.zk_digest_sim_long_sha256.argtypes = [C.c_uint64, C.c_void_p]
        for f, res, args in ((l.zkg_sim_leaves, C.c_uint64, [C.c_uint64]), (l.zkg_sim_blocks, C.c_uint32, [C.c_uint64]),
                             (l.zkg_sim_pass_end, C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]), (l.zkg_sim_scratch, C.c_uint64, [C.c_uint32, C.c_uint64])):
            f.restype, f.argtypes = res, args
        _LIB = l
    return _LIB


def sim(lib, algo, data, off, misalign=0, descending=False, tail=64):
    """the launchers' kernels over the list -> (rc, digests np.uint8[count, 32], the `tail` bytes behind them); data is the bytes
    [off[0], off[count]); -5: a kernel wrote outside the digests"""
    off = np.ascontiguousarray(off, np.uint64)
    data = np.ascontiguousarray(data, np.uint8)
    count = len(off) - 1
    assert len(data) == int(off[-1] - off[0])
    out = np.full(count * 32 + tail, POISON, np.uint8)
    rc = lib.zk_digest_sim(ALGOS.get(algo, algo), data.ctypes.data if len(data) else None, off.ctypes.data, count, misalign, 1 if descending else 0,
                           out.ctypes.data, len(out))
    return rc, out[:count * 32].reshape(count, 32), out[count * 32:]


def long_pattern(n):
    """the bytes the harness's long SHA-256 frame is made of: byte i = (i ^ (i >> 8)) & 255, a period of 65536"""
    i = np.arange(65536, dtype=np.uint32)
    block = ((i ^ (i >> 8)) & 255).astype(np.uint8)
    return np.tile(block, -(-n // 65536))[:n]

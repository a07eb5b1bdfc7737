"""Batches of frames at the edges of the decoder's XXH64 kernels (zeekstd_amd/csrc/zk_xxh64.h), the emulated kernels themselves
(tests/sim/zk_xxh_sim.cpp under tests/sim/hip_wg_emu.h, built here with g++ as train_model.lib() builds the trainer's) and scripts
that stand in for the executor in front of the two followers.  tests/test_sim_xxh64.py runs them on the CPU, tests/test_gpu_xxh64_edges.py
the same batches on the device.

A BATCH is a list of frame lengths, the first offset of its table (off[0]) and the alignment of its first byte modulo 16, built for ONE
kernel's step size U -- the bytes of a batched step:
    wide    2 x 24 stripes = 1536        lean    2 x 12 = 768          follow  2 x 7 = 448
    frame, follow1  1 KiB chunks = 1024  fed4    chunks of 32 stripes = 1024, six under way: 1, 2, 5, 6, 7, 12, 13 chunks
and comes with the FACTS that make it an edge, as (wave or group, name, value) triples.  model() restates each kernel's split of a wave
(`least`, `common`, leftover stripes, tail bytes) in a few lines of Python; the facts are asserted on that model alone
(test_the_batches_are_the_edges_they_claim) before any kernel is asked."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIM = os.path.join(ROOT, "tests", "sim")
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
DEPS = [os.path.join(SIM, "zk_xxh_sim.cpp"), os.path.join(SIM, "hip_wg_emu.h")] + [os.path.join(CSRC, h) for h in ("zk_xxh64.h", "zk_progress.h", "zk_dec_plan.h", "zk_device.h")]

# the helper's copies of the kernels' loop constants (test_the_helper_knows_the_kernels_constants holds them against the header's)
ZK_XXW, ZK_XXL, ZK_FOLLOW_W, ZK_XF_CHUNK, ZK_XF_DEPTH, ZK_FOLLOW_PATIENCE = 24, 12, 7, 32, 6, 5000000
PROG_ABORT, PROG_VERIFIED, PROG_MISMATCH = 1 << 60, 1 << 61, 1 << 62
CHECKSUM_WRONG = 22
POISON = 0x5A5A5A5A5A5A5A5A
# kernel -> (ZkXxhKernel for the sim or None, frames per wave / group, stripes per batched step)
KERNELS = {"frame": (0, 1, 32), "wide": (1, 16, 2 * ZK_XXW), "lean": (2, 16, 2 * ZK_XXL), "fed4": (3, 4, ZK_XF_CHUNK),
           "follow": (None, 16, 2 * ZK_FOLLOW_W), "follow1": (None, 1, 32)}
PASSES = ("frame", "wide", "lean", "fed4")
FED_CHUNKS = (1, 2, 5, 6, 7, 12, 13)            # against D = 6 under way: fewer, D - 1, D, D + 1, 2 D, 2 D + 1
CHOICE = {"frame": 1, "wide": 2, "lean": 3, "fed4": 5}      # ZK_CHOICE_XXH64 that pins the kernel in zk_xxh64_frames_dev


def step_bytes(kernel):
    return 32 * KERNELS[kernel][2]


def edge_lengths(u):
    return [0, 1, 31, 32, 33, u - 32, u - 1, u, u + 1, u + 31, u + 32, 2 * u, 2 * u + 37, 3 * u - 1]


# ---------------------------------------------------------------------------------------------------------------- the model
Wave = namedtuple("Wave", "frames live least common leftover tails")


def model(kernel, lens, live=None):
    """the kernel's split, wave by wave (group by group): frames (indices), live (those it hashes), least (fewest stripes of a live
    frame, None: nothing to hash), common (stripes the batched loop takes from every frame), leftover (stripes taken one by one, per
    frame; 0 for a frame that is not live), tails (len % 32 per frame)"""
    _, per, step = KERNELS[kernel]
    n = len(lens)
    live = [True] * n if live is None else list(live)
    if kernel == "follow":                                    # wave g: frames (g >> 3) * 128 + class + 8 j
        groups = [[(g >> 3) * 128 + (g & 7) + 8 * j for j in range(16)] for g in range(8 * ((n + 127) // 128))]
    else:
        groups = [list(range(b, b + per)) for b in range(0, n, per)]
    out = []
    for fr in groups:
        fr = [f for f in fr if f < n]
        lv = [f for f in fr if live[f]]
        least = min((lens[f] >> 5 for f in lv), default=None)
        if kernel in ("frame", "follow1"):
            common = 0 if least is None else (lens[fr[0]] >> 10) * 32
        else:
            common = 0 if least is None else least - least % step
        out.append(Wave(fr, lv, least, common, [(lens[f] >> 5) - common if f in lv else 0 for f in fr], [lens[f] & 31 for f in fr]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the batches
class Batch:
    def __init__(self, name, kernel, lens, start=0, align=0, facts=(), seed=None):
        self.name, self.kernel, self.lens, self.start, self.align, self.facts = name, kernel, [int(x) for x in lens], start, align, list(facts)
        self.seed = seed if seed is not None else (sum(name.encode()) * 2654435761 + len(lens)) & 0x7FFFFFFF
        self._data = self._want = None

    @property
    def count(self):
        return len(self.lens)

    def off(self):
        o = np.zeros(self.count + 1, np.uint64)
        o[1:] = np.cumsum(self.lens)
        return o + np.uint64(self.start)

    def data(self):
        """the frames' bytes alone (off[0] ... off[count]); computed once, never changed"""
        if self._data is None:
            self._data = np.random.RandomState(self.seed).randint(0, 256, max(sum(self.lens), 1), dtype=np.uint8)[:sum(self.lens)]
            self._data.setflags(write=False)
        return self._data

    def frame(self, f):
        o = self.off() - np.uint64(self.start)
        return self.data()[int(o[f]):int(o[f + 1])].tobytes()

    def want(self):
        """XXH64 of every frame by the oracle's C (computed once)"""
        if self._want is None:
            from oracle import zko
            self._want = [zko.xxh64(self.frame(f)) for f in range(self.count)]
        return self._want

    def __repr__(self):
        return f"{self.kernel}:{self.name}"


def _ragged(u, n, seed):
    """n lengths of one to three steps with every kind of tail, none below a step"""
    r = np.random.RandomState(seed)
    return [int(u + 32 * r.randint(0, 2 * u // 32) + r.choice([0, 1, 3, 4, 7, 8, 12, 17, 24, 31])) for _ in range(n)]


def _by_class(lens):
    """zk_k_xxh64_follow's layout: the sixteen frames of wave w (consecutive in `lens`) at (w >> 3) * 128 + (w & 7) + 8 j; the places
    between them hold frames of 40 bytes, waves of their own"""
    at = [(w >> 3) * 128 + (w & 7) + 8 * j for w in range((len(lens) + 15) // 16) for j in range(16)][:len(lens)]
    out = [40] * (max(at) + 1)
    for i, x in zip(at, lens):
        out[i] = x
    return out


def batches(kernel):
    _, per, step = KERNELS[kernel]
    u = 32 * step
    out = []
    # shape(lens): `lens` lists a batch wave after wave (group after group).  The passes take consecutive frames; a wave of
    # zk_k_xxh64_follow takes every eighth frame of its 128, so for "follow" the list is laid out by class (_by_class) and model()'s
    # wave w is again the w-th sixteen of `lens`.  (Which follower runs is the plan's choice by count, not the batch's name: up to 32
    # frames go to zk_k_xxh64_follow1 -- the count_1 / _15 / _17 batches of either follower's list.)
    shape = _by_class if kernel == "follow" else list
    # every length of the list in one batch (a frame of 0 bytes in the first wave: least == 0 there, everything is leftover and tail)
    ll = edge_lengths(u)
    out.append(Batch("edge_lengths", kernel, shape(ll), start=1, align=1, facts=[(0, "least", 0), (0, "common", 0), ("all", "tails", set(range(32)) & {x & 31 for x in ll})]))
    # every tail of 0 ... 31 bytes behind one stripe: all of zk_xxh64_finish's 8 / 4 / 1-byte steps
    out.append(Batch("tails", kernel, shape([32 + t for t in range(32)]), start=4097, align=15, facts=[("all", "tails", set(range(32)))]))
    # waves (groups) of equal frames, one per length from U - 32 on: the batched loop on 0, 1, 1, ..., 2, 2 steps with and without leftovers
    eq = [x for x in ll if x >= u - 32]
    out.append(Batch("equal_waves", kernel, shape([x for x in eq for _ in range(per)]), start=0, align=8,
                     facts=[(w, "common", ((x >> 5) // step * step) if per > 1 else (x >> 10) * 32) for w, x in enumerate(eq)] +
                           [(w, "leftover_all", (x >> 5) - (((x >> 5) // step * step) if per > 1 else (x >> 10) * 32)) for w, x in enumerate(eq)]))
    if per > 1:
        # the shortest frame (a step and a byte) in the wave's first, middle and last lane group, its neighbours two to three steps long
        lens, facts = [], []
        for w, g in enumerate((0, per // 2 - 1 if per == 16 else 1, per - 1)):
            wl = [2 * u + 32 * (3 * j + 1) + (5 * j) % 32 for j in range(per)]
            wl[g] = u + 1
            lens += wl
            facts += [(w, "least", u >> 5), (w, "common", step), (w, "shortest", g), (w, "leftover_of_shortest", 0)]
        out.append(Batch("shortest_in_lane_group", kernel, shape(lens), start=4097, align=0, facts=facts))
        # least an exact multiple of U, longer neighbours: the batched loop runs, leftover stripes for some lanes only
        wl = [2 * u] + [2 * u + 32 * j + (7 * j) % 32 for j in range(1, per)]
        out.append(Batch("least_a_multiple", kernel, shape(wl[::-1] + wl), start=1, align=15,
                         facts=[(0, "common", 2 * step), (1, "common", 2 * step), (0, "leftover_zero_for", [per - 1]), (1, "leftover_zero_for", [0])]))
        # least == 0 among long frames: no batched step although every other frame has three
        wl = [3 * u - 1] * per
        wl[per // 2] = 0
        w2 = [3 * u - 1] * per
        w2[per - 1] = 31
        out.append(Batch("least_zero_among_long", kernel, shape(wl + w2), start=0, align=1, facts=[(0, "common", 0), (1, "common", 0), (0, "least", 0), (1, "least", 0)]))
    # counts of 1, 15, 17 and 65 modulo 16 (1, 3, 1, 1 modulo 4), and of 3 and 5 modulo 4: consecutive frames as they are, for the
    # followers too (a last wave of n - last * per frames is a fact of the passes' layout only)
    for n in (1, 15, 17, 65) + ((3, 5) if per == 4 else ()):
        lens = _ragged(u, n, 100 + n)
        last = (n - 1) // per
        out.append(Batch(f"count_{n}", kernel, lens, start=(0, 1, 4097)[n % 3], align=(0, 1, 8, 15)[n % 4],
                         facts=([(last, "frames", n - last * per)] if kernel != "follow" else []) + ([(0, "common_positive", True)] if per > 1 else [])))
    # groups mixing frames that begin on a 16-byte boundary with ragged ones, at every placement (the `aligned` / `any_ragged` load paths)
    mix = [u, u + 16, u + 1, 2 * u + 15, u + 32, u + 48, 2 * u, 2 * u + 16] + [2 * u + 16] * 4 + [u + 5, u + 11, u + 16, u]
    for start in (0, 1, 4097):
        for align in (0, 1, 8, 15):
            ml = shape(mix)
            out.append(Batch(f"mixed_alignment_{start}_{align}", kernel, ml, start=start, align=align,
                             facts=[("all", "aligned_frames", sorted(i for i in range(len(ml)) if (align + sum(ml[:i])) % 16 == 0))]))
    if kernel == "fed4":
        # the ring: groups whose frames have k chunks in common, k against the six under way; one frame of the group a chunk longer
        for k in FED_CHUNKS:
            uk = 1024 * k
            ll = edge_lengths(uk)
            lens = []
            for x in ll[5:]:
                lens += [x, x + 1024, x + 7, x]
            out.append(Batch(f"ring_{k}_chunks", kernel, shape(ll + lens), start=(0, 1, 4097)[k % 3], align=(0, 15, 8, 1)[k % 4],
                             facts=[((len(ll) + 3) // 4 + w, "common", (x >> 10) * 32) for w, x in enumerate(ll[5:])]))
    return out


def check_facts(b):
    """the batch's facts on model() alone"""
    m = model(b.kernel, b.lens)
    per = KERNELS[b.kernel][1]
    for w, name, value in b.facts:
        if name == "tails":
            assert value <= {t for x in m for t in x.tails}, (b, name)
        elif name == "aligned_frames":
            got = sorted(i for i in range(b.count) if (b.align + sum(b.lens[:i])) % 16 == 0)
            assert got == value and (b.align != 0 or 0 < len(got) < b.count), (b, name, got)
        elif name == "least":
            assert m[w].least == value, (b, w, name, m[w].least)
        elif name == "common":
            assert m[w].common == value, (b, w, name, m[w].common)
        elif name == "common_positive":
            assert m[w].common > 0, (b, w, name)
        elif name == "leftover_all":
            assert all(x == value for x in m[w].leftover), (b, w, name, m[w].leftover)
        elif name == "shortest":
            assert min(range(len(m[w].frames)), key=lambda j: b.lens[m[w].frames[j]]) == value, (b, w, name)
        elif name == "leftover_of_shortest":
            assert min(m[w].leftover) == value and max(m[w].leftover) > 0, (b, w, name)
        elif name == "leftover_zero_for":
            assert [j for j, x in enumerate(m[w].leftover) if x == 0] == value, (b, w, name, m[w].leftover)
        elif name == "frames":
            assert len(m[w].frames) == value and w == len(m) - 1, (b, w, name)
        else:
            raise KeyError(name)


def decoder_forms(b):
    """the decoder's view of a batch: [(name, status[], flag[], verified[])] -- frames without a checksum flag, frames whose status is not
    ZK_OK, frames a follower has verified (only for the kernels that take `skip`), whole waves / groups without a live frame, a single live
    frame that is the last one"""
    n, per = b.count, KERNELS[b.kernel][1]
    z = lambda: np.zeros(n, np.uint32)
    one = lambda: np.ones(n, np.uint32)
    forms = [("all_live", z(), one(), z())]
    st, fl, ve = z(), one(), z()
    st[1::5] = 20
    fl[2::5] = 0
    ve[3::5] = 1
    forms.append(("mixed", st, fl, ve))
    if n > per:
        st, fl, ve = z(), one(), z()
        st[:per:3] = 72; fl[1:per:3] = 0; ve[2:per:3] = 1      # the first wave (group) has no live frame
        if b.kernel not in ("wide", "fed4"):
            st[2:per:3] = 70
        forms.append(("dead_first_wave", st, fl, ve))
    st, fl, ve = z(), z(), z()
    fl[n - 1] = 1
    forms.append(("only_the_last", st, fl, ve))
    return forms


# ---------------------------------------------------------------------------------------------------------------- the emulated kernels
_LIB = None


class Event(C.Structure):
    _fields_ = [("step", C.c_uint32), ("frame", C.c_uint32), ("bytes", C.c_uint32), ("xcd", C.c_uint32), ("abort", C.c_uint32)]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(SIM, "libzk_xxh_sim.so")
        if not os.path.exists(so) or max(os.path.getmtime(p) for p in DEPS) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-attributes", "-o", so, DEPS[0]])
        l = C.CDLL(so)
        l.zk_xxh_sim_consts.restype = None
        l.zk_xxh_sim_consts.argtypes = [C.c_void_p]
        l.zk_xxh_sim_plan.restype = C.c_uint32
        l.zk_xxh_sim_plan.argtypes = [C.c_uint32, C.c_int, C.c_int]
        l.zk_xxh_sim_follow_plan.restype = C.c_uint32
        l.zk_xxh_sim_follow_plan.argtypes = [C.c_uint32]
        l.zk_xxh_sim_pass.restype = C.c_int
        l.zk_xxh_sim_pass.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 + [C.c_int]
        l.zk_xxh_sim_follow.restype = C.c_int
        l.zk_xxh_sim_follow.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p,
                                        C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        _LIB = l
    return _LIB


def consts():
    out = np.zeros(8, np.uint64)
    lib().zk_xxh_sim_consts(out.ctypes.data)
    return [int(x) for x in out]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _table(b, first):
    """the batch's offsets behind `first` entries the kernels must not read"""
    return np.concatenate([np.full(first, 0x7FFFFFFFFFFF0000, np.uint64), b.off()])


def sim_pass(kernel, b, infos=None, hashes=True, skip=None, descending=False, first=0, data=None):
    """one pass behind the executor under the emulator.  infos: (status, flag, checksum) uint32 arrays or None; skip: progress words or
    None.  -> (hashes or None, status or None); the hash slots hold POISON before."""
    data = np.ascontiguousarray(b.data() if data is None else data)
    off = _table(b, first)
    h = np.full(b.count, POISON, np.uint64) if hashes else None
    st = fl = ck = None
    if infos is not None:
        st, fl, ck = (np.ascontiguousarray(x, np.uint32).copy() for x in infos)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint64)
    rc = lib().zk_xxh_sim_pass(KERNELS[kernel][0], _ptr(data), data.size, b.align, _ptr(off), first, b.count, _ptr(st), _ptr(fl), _ptr(ck), _ptr(h), _ptr(sk), int(descending))
    assert rc == 0, rc
    return h, st


def pass_plan(count, choice, skip):
    """zk_xxh_plan -> the kernel's name"""
    p = lib().zk_xxh_sim_plan(count, choice, int(skip))
    name = PASSES[p & 255]
    assert KERNELS[name][1] == p >> 8
    return name


def follow_plan(count):
    """zk_xxh_follow_plan -> ('follow1' or 'follow', grid)"""
    p = lib().zk_xxh_sim_follow_plan(count)
    return ("follow1" if p & 1 else "follow"), p >> 8


# ---------------------------------------------------------------------------------------------------------------- the scripted executor
TICK = ZK_FOLLOW_PATIENCE // 4            # emulated clock per poll: a wave gives up on its sixth poll without news


def max_polls(events):
    """No wave polls more often than this: an event of step s is noticed at clock s * TICK at the latest (the script moves only at
    polls), and behind the last news the clock passes the patience after PATIENCE / TICK + 1 polls; + 1 for the poll that notices."""
    return max((e[0] for e in events), default=0) + ZK_FOLLOW_PATIENCE // TICK + 2


def sim_follow(b, infos, events, wg_xcd, descending=False, limit=None):
    """the follower zk_xxh_follow_plan takes for the batch against a script: events = [(step, frame, bytes, xcd, abort)], sorted by
    step here; wg_xcd[b]: the XCD of workgroup b.  -> (rc, progress words, polls per wave)"""
    _, grid = follow_plan(b.count)
    assert len(wg_xcd) == grid
    ev = sorted(events, key=lambda e: e[0])
    arr = (Event * max(len(ev), 1))(*[Event(*e) for e in ev])
    data, off = np.ascontiguousarray(b.data()), b.off()
    st, fl, ck = (np.ascontiguousarray(x, np.uint32) for x in infos)
    xc = np.ascontiguousarray(wg_xcd, np.uint32)
    prog, polls = np.zeros(b.count, np.uint64), np.zeros(grid, np.uint64)
    rc = lib().zk_xxh_sim_follow(_ptr(data), data.size, b.align, _ptr(off), 0, b.count, _ptr(st), _ptr(fl), _ptr(ck), C.addressof(arr), len(ev),
                                 _ptr(xc), TICK, max_polls(ev) if limit is None else limit, int(descending), _ptr(prog), _ptr(polls))
    assert rc in (0, 1), rc
    return rc, prog, [int(x) for x in polls]


# ---------------------------------------------------------------------------------------------------------------- jobs for tests/sim/xxh_san.cpp
def pack_job(b, kernel=None, infos=None, skip=None, first=0, events=None, wg_xcd=(), limit=None, expect_hash=None, expect_status=None, expect_progress=None):
    """one job of the sanitizer program's input file, all in 64-bit words: a header, the arrays, what to expect, the frames' bytes.
    kernel: a pass's name, or None for the follower of the plan (events / wg_xcd as sim_follow takes them)."""
    n = b.count
    u64 = lambda a, fill=0: np.full(n, fill, np.uint64) if a is None else np.array([int(x) for x in a], dtype=np.uint64)
    ev = sorted(events or [], key=lambda e: e[0])
    st, fl, ck = infos if infos is not None else (None, None, None)
    data = b.data()
    head = [0 if kernel else 1, KERNELS[kernel][0] if kernel else 0, first, n, b.align, int(infos is not None), int(skip is not None), len(ev), len(wg_xcd),
            TICK, (max_polls(ev) if limit is None else limit), data.size, int(expect_hash is not None)]
    words = [np.array(head, np.uint64), _table(b, first), u64(st), u64(fl), u64(ck), u64(skip), np.array([x for e in ev for x in e], np.uint64),
             np.array(list(wg_xcd), np.uint64), u64(expect_hash), u64(expect_status), u64(expect_progress)]
    return b"".join(w.astype("<u8").tobytes() for w in words) + data.tobytes() + b"\0" * (-data.size % 8)

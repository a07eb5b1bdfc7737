"""TEST INFRASTRUCTURE -- the archives of generated frames (tests/helpers/zstd_gen.py) that tests/test_gpu_generated_variants.py decodes on the
device, and the facts about them that its tests rest on.  Both live here so that tests/test_generated_frames.py can ask the same archives
on the CPU what the GPU tests take for granted: that libzstd 1.5.7 reads them as the generator's model does, that they reach the codes, depths
and group boundaries they are there for, and that the dense frames overflow a segment's hole records in the simulator.

Every frame is generated once per process (functools.lru_cache) and never changed.  A batch is a list of Frame; `archive` lays it out.

The block facts are the generator's own (generate(..., stats=True)); what is derived from them mirrors the device code:
  keys          zk_fse_share_pick (zk_decode.hip): per table PREDEF for Predefined_Mode, the block's own index for FSE_Compressed_Mode, and
                for Repeat_Mode the index of the last block of the frame with sequences that said anything else (zk_walk_frame's tab_def).
                A block with sequences and no RLE_Mode table is a candidate
  share_runs    the kernel's workgroups: aligned runs of 64 consecutive blocks of the batch, the first candidate's keys are the reference
                With a formatted dictionary (Frame.dict) a frame starts with the dictionary's entry in force for all three tables and the
                tree: its index is the batch's block count (zk_dict.h), which is what keys and huf_at then say
  huf_groups    zk_huf_group: groups of 16 consecutive blocks, a table of 2^depth cells per block with Huffman literals, a new pass of the
                pool whenever the next table does not fit"""
import collections
import functools

from helpers import zstd_gen
from oracle import zko

LONG_KW = dict(max_blocks=10, max_seq=4000, max_lit=100000)
TAIL_KW = dict(max_lit=1 << 17, max_ll=1 << 17, max_ml=1 << 17)
SHARED_KW = dict(shared_tables=True)
DENSE_KW = dict(dense=True, max_blocks=8)
KINDS = {"default": {}, "long": LONG_KW, "tail": TAIL_KW, "shared": SHARED_KW, "dense": DENSE_KW}

# the seeds the GPU tests use (fresh ranges: tests/test_generated_frames.py and tests/test_gpu_generated_frames.py use others)
DEFAULT_SEEDS = range(800000, 800600)
LONG_SEEDS = range(810000, 810060)
TAIL_SEEDS = range(820000, 820040)
SHARED_SEEDS = range(830000, 830024)
DENSE_SEEDS = (500000, 500001)                               # 32 512+ matches of 3 and 4 bytes in one block: more hole records than a segment's region holds
FILTER_FROM = 5000                                           # batch 1 of the fused kernel's tests: the first seeds from here on with own_blocks <= 1
AGGREGATE_FROM = 840000                                      # batch 2: frames with >= 3 own blocks, and frames with none

PREDEF = "predef"
Frame = collections.namedtuple("Frame", "seed kind comp data facts own feats dict", defaults=(None, None))   # dict: the name in DICTS, None without


@functools.lru_cache(maxsize=None)
def frame(seed, kind="default"):
    f, out, _, facts = zstd_gen.generate(seed, zko.xxh64, stats=True, **KINDS[kind])
    return Frame(seed, kind, f, out, facts, zstd_gen.own_blocks(facts))


def frames(seeds, kind="default"):
    return [frame(s, kind) for s in seeds]


def archive(batch):
    """-> (compressed bytes, [(compressed size, decoded size)], decoded bytes)"""
    return b"".join(f.comp for f in batch), [(len(f.comp), len(f.data)) for f in batch], b"".join(f.data for f in batch)


def filtered(n, start=FILTER_FROM, most_own=1):
    """the first n default frames from seed `start` on with at most `most_own` own blocks"""
    out, seed = [], start
    while len(out) < n:
        f = frame(seed)
        if f.own <= most_own: out.append(f)
        seed += 1
    return out


def aggregate(n_heavy=24, start=AGGREGATE_FROM):
    """n_heavy default frames with >= 3 own blocks each, between as many frames WITHOUT own blocks as make the batch's sum fit its frame count"""
    heavy, free, seed = [], [], start
    while len(heavy) < n_heavy or len(free) + len(heavy) < sum(f.own for f in heavy):
        f = frame(seed)
        if f.own >= 3 and len(heavy) < n_heavy: heavy.append(f)
        elif f.own == 0: free.append(f)
        seed += 1
    out = []
    for i, f in enumerate(free):                             # (interleaved: the heavy frames' blocks share workgroups with the others')
        out.append(f)
        if i < len(heavy): out.append(heavy[i])
    return out + heavy[len(free):]


def padded(batch, start=AGGREGATE_FROM, interleave=True):
    """the batch and as many default frames WITHOUT own blocks (from seed `start` on) as make the sum of own blocks fit the frame count:
    spread between the batch's frames, or all behind them"""
    free, seed = [], start
    while len(free) + len(batch) < sum(f.own for f in batch):
        f = frame(seed)
        if f.own == 0: free.append(f)
        seed += 1
    if not interleave: return list(batch) + free
    out = []
    for i, f in enumerate(batch):
        out.append(f)
        out += free[i * len(free) // len(batch):(i + 1) * len(free) // len(batch)]
    return out


# the batches of the fused entropy kernel's tests (tests/test_gpu_generated_variants.py, part c)
def batch_filtered():
    return filtered(800)


def batch_aggregate():
    return aggregate()


def batch_shared():
    return padded(frames(SHARED_SEEDS, "shared"), interleave=False)


def batch_huffman():
    """the shared_tables frames in reverse order (other group boundaries than batch_shared's) between frames without own blocks, and more
    of those behind them until the last group of 16 blocks has one to three"""
    out = padded(frames(reversed(SHARED_SEEDS), "shared"))
    seed = AGGREGATE_FROM + 5000
    while sum(len(f.facts) for f in out) % 16 not in (1, 2, 3):
        if frame(seed).own == 0: out.append(frame(seed))
        seed += 1
    return out


# ---------------------------------------------------------------------------------------------- dictionaries (make_dictionary) and frames against them
# what tests/test_gpu_generated_dict.py decodes; tests/test_generated_dict.py asks libzstd 1.5.7 about the same pairs on the CPU
DICTS = {
    # the routes' six: the content sizes at the edges, both weight forms, the accuracy logs at their ends, IDs of every field width
    "one_byte": dict(seed=101, content_size=1, weights="direct", alphabet=2, dict_id=0x1234),
    "seven": dict(seed=102, content_size=7, weights="fse", dict_id=200),
    "eight": dict(seed=103, content_size=8, weights="direct", depth=11, als={"of": 5, "ll": 5, "ml": 5}),
    "nine": dict(seed=104, content_size=9, weights="fse", alphabet=256, als={"of": 8, "ll": 9, "ml": 9}, reps=(9, 9, 1)),
    "few_kib": dict(seed=105, content_size=5000, weights="direct", dict_id=77, als={"of": 5, "ll": 9, "ml": 5}),
    "big": dict(seed=106, content_size=140000, weights="fse", depth=11, dict_id=0x89ABCDEF, als={"of": 8, "ll": 5, "ml": 9}, reps=(140000, 1, 140000)),
    # switching: two with one ID and nothing else in common, and a formatted one with ID 0
    "same_id_a": dict(seed=107, dict_id=4242, content_size=700),
    "same_id_b": dict(seed=108, dict_id=4242, content_size=3000),
    "id0": dict(seed=109, dict_id=0, content_size=600),
    # the large batch's: tables that cover every code, so that blocks of many frames repeat them
    "wide": dict(seed=110, dict_id=65000, content_size=3000, wide=True, als={"of": 6, "ll": 7, "ml": 8}),
}
ROUTE_DICTS = ("one_byte", "seven", "eight", "nine", "few_kib", "big")
DICT_SEEDS = {name: range(900000 + 1000 * i, 900000 + 1000 * i + 120) for i, name in enumerate(DICTS)}      # default frames per dictionary
DICT_SHARED_SEEDS = range(950000, 950090)                    # shared_tables frames against "few_kib": mostly (Repeat, Repeat, Repeat) on the dictionary's tables
BIG_DICT = "wide"


@functools.lru_cache(maxsize=None)
def dictionary(name):
    """-> (bytes, model) of DICTS[name]"""
    return zstd_gen.make_dictionary(**DICTS[name])


@functools.lru_cache(maxsize=None)
def dict_frame(name, seed, kind="default"):
    f, out, feats, facts = zstd_gen.generate(seed, zko.xxh64, stats=True, dictionary=dictionary(name)[1], **KINDS[kind])
    return Frame(seed, kind, f, out, facts, zstd_gen.own_blocks(facts), frozenset(feats), name)


def dict_frames(name, seeds=None, kind="default"):
    return [dict_frame(name, s, kind) for s in (DICT_SEEDS[name] if seeds is None else seeds)]


def dict_batch_big():
    """just past 4096 blocks: shared_tables frames and default frames against BIG_DICT in turn, until the count is there"""
    out, n = [], 0
    pool = [x for pair in zip(dict_frames(BIG_DICT, DICT_SHARED_SEEDS, "shared"), dict_frames(BIG_DICT) + dict_frames(BIG_DICT)) for x in pair]
    for f in pool:
        out.append(f); n += len(f.facts)
        if n > 4096: return out
    raise AssertionError("the pool has %d blocks only" % n)


def dict_batch_small():
    """frames of dict_batch_big, 4096 blocks or fewer: the other side of zk_launch_fse's threshold"""
    out, n = [], 0
    for f in dict_batch_big()[::-1]:
        if n + len(f.facts) > 2000: break
        out.append(f); n += len(f.facts)
    return out


def dict_batch_mixed():
    """default and shared_tables frames against BIG_DICT side by side"""
    d, s = dict_frames(BIG_DICT)[:60], dict_frames(BIG_DICT, DICT_SHARED_SEEDS[:6], "shared")
    return d[:30] + s[:3] + d[30:] + s[3:]


def dict_batch_fused():
    """the default frames of BIG_DICT that describe at most one set of tables each (the fused kernel's condition is on the sum)"""
    return [f for f in dict_frames(BIG_DICT) if f.own <= 1]


def dict_batch_sizes():
    """the frames of BIG_DICT without Frame_Content_Size: what they decode to is known from their sequences only"""
    return [f for f in dict_frames(BIG_DICT) + dict_frames(BIG_DICT, DICT_SHARED_SEEDS[:6], "shared") if {"fcs0", "windowed"} <= f.feats]


DAMAGED_DICTS = ("wide", "nine")


@functools.lru_cache(maxsize=None)
def dict_damaged(name):
    """the default frames of DICTS[name] with one to three flipped bits in every other frame or so:
    -> (the damaged bytes, [(compressed size, decoded size)], the frames that were hit, the undamaged frames' decoded bytes)"""
    import random
    comp, sizes, data = archive(dict_frames(name))
    bad, rng, at, hit = bytearray(comp), random.Random(len(comp)), 0, set()
    for i, (cs, _) in enumerate(sizes):
        if rng.random() < 0.5:
            hit.add(i)
            for _ in range(rng.randint(1, 3)):
                bad[at + rng.randrange(cs)] ^= 1 << rng.randrange(8)
        at += cs
    return bytes(bad), sizes, frozenset(hit), data


REFUSED_FLOOR = 1 / 3       # of the hit frames.  One to three flipped bits per hit frame: a flip in a header, a table description or a
                            # bitstream's last byte is mostly fatal, one in Raw literals or a Raw block never is (checksums are off)


@functools.lru_cache(maxsize=None)
def dict_damaged_verdicts(name):
    """per hit frame of dict_damaged(name): the oracle's bytes, or None where it refuses"""
    bad, sizes, hit, _ = dict_damaged(name)
    d = dictionary(name)[0]
    import numpy as np
    c = np.concatenate([[0], np.cumsum([s[0] for s in sizes])])
    out = {}
    for f in sorted(hit):
        try:
            o, used = zko.frame_decode(bad[int(c[f]):int(c[f + 1])], sizes[f][1] + 64, False, dictionary=d)
            out[f] = o if len(o) == sizes[f][1] and used == sizes[f][0] else None
        except zko.OracleError:
            out[f] = None
    return out


def dict_damaged_judge(name, out, st):
    """out, st: what a decoder under test made of dict_damaged(name) -- it refuses the frames the oracle refuses and yields its bytes otherwise"""
    bad, sizes, hit, data = dict_damaged(name)
    import numpy as np
    d = np.concatenate([[0], np.cumsum([s[1] for s in sizes])])
    want = dict_damaged_verdicts(name)
    for f in range(len(sizes)):
        lo, hi = int(d[f]), int(d[f + 1])
        if f not in hit:
            assert st[f] == 0 and out[lo:hi] == data[lo:hi], (name, f)
            continue
        assert (want[f] is not None) == (st[f] == 0), (name, f, int(st[f]))
        if want[f] is not None:
            assert out[lo:hi] == want[f], (name, f)
    assert sum(1 for f in hit if want[f] is None) >= REFUSED_FLOOR * len(hit)


def run_kinds(blocks):
    """per run of share_runs what its reference keys are: "dict" (all three the dictionary's entry), "dict+predef" (that entry and predefined
    tables, nothing else), "owned" (a block of the batch owns one), "predef" """
    n, out = len(blocks), []
    for r in share_runs(blocks):
        k = set(r.keys)
        out.append("owned" if any(x != PREDEF and x < n for x in k) else "dict" if k == {n} else "dict+predef" if k == {n, PREDEF} else "predef")
    return out


# ---------------------------------------------------------------------------------------------- what the device code makes of a batch
def blocks_of(batch):
    """the batch's blocks in the order of the engine's block records: dicts of the generator's facts + frame (index in the batch), at (index in
    the batch), keys (three of them, None without sequences), cand, huf_at (the defining block's index in the batch, None without Huffman).
    The dictionary's entry has the index len(result)."""
    out = []
    nblocks = sum(len(f.facts) for f in batch)
    for fi, f in enumerate(batch):
        base = len(out)
        start = nblocks if f.dict is not None and dictionary(f.dict)[1].formatted else None
        tab_def = [start, start, start]
        for b in f.facts:
            b = dict(b, frame=fi, at=len(out), keys=None, cand=False, huf_at=None)
            if b["type"] == "comp":
                if b["huf_def"] is not None: b["huf_at"] = nblocks if b["huf_def"] == "dict" else base + b["huf_def"]
                if b["modes"] is not None:
                    m = [(b["modes"] >> s) & 3 for s in (6, 4, 2)]
                    for t in range(3):
                        if m[t] != 3: tab_def[t] = b["at"]
                    b["keys"] = tuple(PREDEF if m[t] == 0 else tab_def[t] for t in range(3))
                    b["cand"] = 1 not in m
            out.append(b)
    return out


Run = collections.namedtuple("Run", "first ref keys share predef ref_before")


def share_runs(blocks):
    """per aligned run of 64 blocks that has a candidate: its first block, the first candidate, that one's keys, how many candidates of the
    run have the same keys, whether the keys are all predefined, whether one of them names a block before the run"""
    out = []
    for lo in range(0, len(blocks), 64):
        run = blocks[lo:lo + 64]
        ref = next((b for b in run if b["cand"]), None)
        if ref is None: continue
        k = ref["keys"]
        out.append(Run(lo, ref["at"], k, sum(1 for b in run if b["cand"] and b["keys"] == k), all(x == PREDEF for x in k),
                       any(x != PREDEF and x < lo for x in k)))
    return out


Group = collections.namedtuple("Group", "first depths passes streams")


def huf_groups(blocks, pool=4096):
    """per group of 16 blocks: the depths of its Huffman tables (a table per block with Huffman or Treeless literals), the passes a pool
    of `pool` cells takes for them, the stream counts that occur"""
    out = []
    for lo in range(0, len(blocks), 16):
        g = [b for b in blocks[lo:lo + 16] if b["type"] == "comp" and b["lit"] in ("huf", "treeless")]
        passes, acc = 1, 0
        for b in g:
            if acc + (1 << b["huf_depth"]) > pool: passes, acc = passes + 1, 0
            acc += 1 << b["huf_depth"]
        out.append(Group(lo, [b["huf_depth"] for b in g], passes, {b["streams"] for b in g}))
    return out


def treeless_reach(blocks):
    """-> (Treeless blocks whose tree was described in another group of 16, ... in another run of 64)"""
    t = [b for b in blocks if b["type"] == "comp" and b["lit"] == "treeless"]
    return sum(1 for b in t if b["huf_at"] // 16 != b["at"] // 16), sum(1 for b in t if b["huf_at"] // 64 != b["at"] // 64)

"""The Huffman half of zk_k_entropy_frame (zk_huf_group<4096, true>, zeekstd_amd/csrc/zk_decode.hip) on trees that are pinned block by block
(tests/helpers/huf_frames.py): groups of 16 blocks whose tables take many passes of the pool, with the two waves in step through an LDS
word at every pass.  Every output byte and every per-frame status against the oracle, under ZK_CHOICE_ENTROPY = 2, into a buffer of 0xA5
with 64 guard bytes on both sides.  A batch's frames lie back to back in the output: what lies before and behind a frame's bytes is the
guard or a neighbour's bytes, and every neighbour of a refused frame is compared byte for byte.

  pressure   a frame of 17 and one of 64 blocks, every block its own tree of depth 11 (2 048 cells: two tables per pass, eight passes per
             group), 4-stream and 1-stream literals, direct and FSE-compressed weights; 81 blocks: a last group of 1
  mixed      trees of depth 5, 8 and 11 in turn: passes split in the middle of a group; 51 blocks: a last group of 3
  treeless   Treeless blocks whose tree was described in an earlier pass of the same group, and in an earlier group; 31 blocks: a last group of 15
  damaged    a damaged tree description in block 0, in block 15 and in block 16 of a frame of 32 blocks (the first pass of a group, its
             last, the next group's first), one kind each: a weight of 15, weights whose sum leaves no power of two for the last symbol
             (both in a direct description), an accuracy log of 20 in an FSE-compressed one; good frames of 16 blocks between them:
             the oracle's status for the three, the others exact
  own        this engine's archive, level 1: 512 blocks of 4 KiB (eight workgroups of 64; 32 frames of 64 KiB, the only frames the encoder
             cuts that small), eight frames of 256 KiB and two frames of 2 MiB -- one batch at a time, and submitted on both contexts at once
  beside     1 024 frames of 512 KiB of this engine's, submitted on both contexts at once: the shape for which zk_exec_plan pads the executor
             to four workgroups per CU beside the other batch's zk_k_entropy_frame (the second batch; the first has no neighbour yet and
             runs at five).  The device offers no read-back of a launch's LDS: the verdict itself is pinned in tests/test_dec_plan_beside.py,
             the size it rests on in tests/test_entropy_budget.py; here both launches must give every byte

Damaged inputs that libzstd accepts and the format oracle refuses: 0 of 3 (the CPU test below asks both about each)."""
import functools

import numpy as np
import pytest

from conftest import offsets_from_frames
from helpers import huf_frames as HF
from helpers.dev_decode import dev as _dev, upload as _upload
from oracle import zko
from oracle import libzstd_ref as Z

gpu = pytest.mark.gpu
POISON, GUARD = 0xA5, 64
POOL = 4096                                                  # ZK_ENT_POOL
FORMS = ("direct", "fse")


def _specs(name):
    if name == "pressure17": return [(11, 4, FORMS[i & 1]) for i in range(17)]
    if name == "pressure64": return [(11, (1, 4)[i & 1], FORMS[(i >> 1) & 1]) for i in range(64)]
    if name == "mixed": return [((5, 8, 11)[i % 3], (4, 1)[i % 2], FORMS[(i // 3) & 1]) for i in range(51)]
    if name == "treeless":                                   # trees in blocks 0 and 4; 1 ... 3 and 5 ... 30 use them
        return [(11, 4, "direct") if i in (0, 4) else (None, (4, 1)[i % 2], None) for i in range(31)]
    if name == "good16": return [((9, 10, 6)[i % 3], 4, FORMS[i & 1]) for i in range(16)]
    if name == "bad32": return [(9, 4, "direct") for _ in range(32)]
    if name == "bad32_fse16": return [(9, 4, "fse" if i == 16 else "direct") for i in range(32)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _frame(name, seed):
    return HF.frame(seed, _specs(name))


DAMAGE = {0: "weight15", 15: "sum", 16: "fse_log"}           # block of the frame -> what is done to its tree description


@functools.lru_cache(maxsize=None)
def _damaged_frame(block):
    """a frame of 32 blocks with the tree description of `block` damaged as DAMAGE says"""
    kind = DAMAGE[block]
    f, data, desc_at = _frame("bad32_fse16" if kind == "fse_log" else "bad32", 9100 + block)
    bad = bytearray(f)
    at = desc_at[block]
    if kind == "fse_log":
        assert 2 <= bad[at] < 128, "an FSE-compressed description"
        bad[at + 1] |= 0x0F                                  # Accuracy_Log = 15 + 5; weights allow 6
    else:
        assert bad[at] >= 128, "a direct description"
        if kind == "weight15": bad[at + 1] |= 0xF0
        else: bad[at + 1] ^= 0x10                            # the first symbol's weight +- 1: the others' sum no longer leaves a power of two
    return bytes(bad), data, desc_at


@functools.lru_cache(maxsize=None)
def _batch(name):
    """-> [(frame bytes, decoded bytes or None for a damaged frame)]"""
    if name == "pressure": return [_frame("pressure17", 9001)[:2], _frame("pressure64", 9002)[:2]]
    if name == "mixed": return [_frame("mixed", 9003)[:2]]
    if name == "treeless": return [_frame("treeless", 9004)[:2]]
    if name == "damaged":
        out = []
        for i, b in enumerate((0, 15, 16)):
            out += [_frame("good16", 9200 + i)[:2], (_damaged_frame(b)[0], None)]
        return out + [_frame("good16", 9203)[:2]]
    raise KeyError(name)


def _passes(specs, first=0):
    """per group of 16 blocks of a batch whose blocks start at index `first`: the passes zk_huf_group takes with POOL cells"""
    depth, depths = None, []
    for d, _, _ in specs:
        depth = d if d is not None else depth
        depths.append(depth)
    out = []
    for lo in range(-(first % 16), len(depths), 16):
        p, acc = 1, 0
        for d in depths[max(lo, 0):lo + 16]:
            if acc + (1 << d) > POOL: p, acc = p + 1, 0
            acc += 1 << d
        out.append(p)
    return out


def _oracle(frame_bytes, n):
    """-> (bytes, 0) or (None, the oracle's error code)"""
    try:
        o, used = zko.frame_decode(frame_bytes, n + 64, True)
        assert used == len(frame_bytes)
        return o, 0
    except zko.OracleError as e:
        return None, e.code


# ------------------------------------------------------------------------------------------------ the inputs, on the CPU
def test_the_frames_are_what_the_tests_take_them_for():
    """the oracle (and libzstd, where the box has one) reads every good frame as the model wrote it; the passes are the ones the cases are
    named for; the three damaged frames are refused by both"""
    lz = Z.load("system") is not None
    for name in ("pressure", "mixed", "treeless", "damaged"):
        for f, data in _batch(name):
            if data is None: continue
            assert _oracle(f, len(data)) == (data, 0), name
            if lz: assert Z.decode_stream(f, len(data)) == data, name
    assert _passes(_specs("pressure17")) == [8, 1]
    assert _passes(_specs("pressure64"), first=17) == [8, 8, 8, 8, 1], "eight passes in every whole group, a last group of one block"
    mixed = _passes(_specs("mixed"))
    assert all(p >= 4 for p in mixed[:3]) and len(_specs("mixed")) % 16 == 3
    assert _passes(_specs("treeless")) == [8, 8] and len(_specs("treeless")) % 16 == 15
    lax = 0
    for b in (0, 15, 16):
        f, data, _ = _damaged_frame(b)
        assert _oracle(f, len(data)) == (None, 20), b
        if lz and Z.decode_stream_verdict(f)[1] == "end": lax += 1
    assert lax == 0, "inputs libzstd accepts and the oracle refuses"


# ------------------------------------------------------------------------------------------------ on the device
def _decode(engine, frames, verify=True):
    """the batch under ZK_CHOICE_ENTROPY = 2 -> (return code, decoded bytes, statuses); the guards are checked here"""
    import torch
    comp = b"".join(f for f, _ in frames)
    sizes = []
    for f, data in frames:
        sizes.append((len(f), int.from_bytes(f[6:10], "little")))            # Frame_Content_Size (huf_frames writes four bytes of it)
        assert data is None or len(data) == sizes[-1][1]
    c, d = offsets_from_frames(sizes)
    d_comp, csize, d_c, d_d = _upload(comp, c, d)
    total = int(d[-1])
    buf = torch.full((GUARD + total + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    d_st = torch.full((len(frames),), -1, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    engine.set_kernel_choice(reset=0)
    try:
        engine.set_kernel_choice(entropy=2)
        rc = engine.decode_frames_dev(d_comp, csize, d_c, d_d, 0, len(frames), buf[GUARD:], total, verify, d_st)
        assert engine.entropy_fused(), "ZK_CHOICE_ENTROPY = 2: zk_k_entropy_frame"
    finally:
        engine.set_kernel_choice(reset=0)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == POISON).all() and (got[GUARD + total:] == POISON).all(), "bytes outside the output written"
    return rc, got[GUARD:GUARD + total], d_st.cpu().numpy(), d


@gpu
@pytest.mark.parametrize("name", ["pressure", "mixed", "treeless"])
def test_trees_that_take_several_passes(engine, name):
    frames = _batch(name)
    rc, got, st, d = _decode(engine, frames)
    assert rc == 0 and not st.any(), (rc, st)
    for i, (f, data) in enumerate(frames):
        assert got[int(d[i]):int(d[i + 1])].tobytes() == data == _oracle(f, len(data))[0], (name, i)


@gpu
def test_damaged_tree_descriptions(engine):
    frames = _batch("damaged")
    rc, got, st, d = _decode(engine, frames)
    want = [_oracle(f, int(d[i + 1] - d[i])) for i, (f, _) in enumerate(frames)]
    assert [int(x) for x in st] == [code for _, code in want] == [0, 20] * 3 + [0]
    assert rc == -20
    for i, (o, code) in enumerate(want):
        if code == 0:                                        # the neighbours of a refused frame: its output may hold anything, theirs is exact
            assert got[int(d[i]):int(d[i + 1])].tobytes() == o == frames[i][1], i


def _own(engine):
    """written by this engine's encoder at level 1, checksummed: eight workgroups' worth of 4 KiB blocks (the encoder cuts those for frames
    below 128 KiB only -- zke_block_max -- so 32 frames of 64 KiB, four frames per workgroup of 64 blocks), eight frames of 256 KiB (16 blocks
    of 16 KiB each) and two frames of 2 MiB (64 blocks of 32 KiB)"""
    from helpers import in_flight as IF
    parts = [(32, 64 << 10, 0xF0), (8, 256 << 10, 0xF1), (2, 2 << 20, 0xF2)]
    comp, sizes, want = b"", [], []
    for n, fs, seed in parts:
        data = zko.gen_chunks(n * fs, seed)
        c, f = engine.encode_frames(data, fs, 1, True)
        assert len(f) == n
        comp += c; sizes += list(f); want += [data[i * fs:(i + 1) * fs] for i in range(n)]
    return IF._batch("own_passes", comp, sizes, want)


@gpu
def test_own_archive_one_batch_at_a_time(engine):
    from helpers import in_flight as IF
    batch = _own(engine)
    engine.set_kernel_choice(reset=0)
    try:
        engine.set_kernel_choice(entropy=2)
        rc, s = IF.decode_sync(engine, batch)
        assert engine.entropy_fused()
    finally:
        engine.set_kernel_choice(reset=0)
    assert rc == 0
    s.check(rc, "one batch at a time")
    assert s.out[:s.total].cpu().numpy().tobytes() == b"".join(_oracle(batch.comp[int(batch.c[i]):int(batch.c[i + 1])], len(w))[0] for i, w in enumerate(batch.want))


@gpu
def test_own_archive_on_both_contexts(engine):
    from helpers import in_flight as IF
    batch = _own(engine)
    first, second = IF.Staged(batch), IF.Staged(batch)
    engine.set_kernel_choice(reset=0)
    engine.set_kernel_choice(entropy=2)
    with IF.Flight(engine) as fl:                            # (leaving it puts the kernel choice back)
        fl.reach("both", first, second)
        for slot in (0, 1):
            rc, st = fl.wait(slot, "both contexts busy")
            assert rc == 0 and not st.any()
            assert engine.entropy_fused()


@gpu
def test_long_frames_beside_another_batch(engine):
    """1 024 frames of 512 KiB (64 distinct ones, sixteen times over) on both contexts at once under ZK_CHOICE_ENTROPY = 2: 256-lane tiles, long
    frames, the fused kernel, and for the second batch a neighbour in flight -- zk_exec_plan's four-per-CU launch beside the first batch's five"""
    from helpers import in_flight as IF
    batch = IF.engine_made(engine, 64, 512 << 10, 0xF3, repeat=16)
    assert len(batch.want) == 1024 and int(batch.d[-1]) == 1024 * IF.FOLLOW_MIN
    first, second = IF.Staged(batch), IF.Staged(batch)
    engine.set_kernel_choice(reset=0)
    engine.set_kernel_choice(entropy=2)
    with IF.Flight(engine) as fl:                            # (leaving it puts the kernel choice back)
        fl.reach("both", first, second)
        for slot in (0, 1):
            rc, st = fl.wait(slot, "long frames, both contexts busy")
            assert rc == 0 and not st.any()
            assert engine.entropy_fused()

"""Generated frames (tests/helpers/zstd_gen.py: what neither libzstd's encoder nor this engine's writes) under the decode kernels that
tests/test_gpu_generated_frames.py does not pin:

  a  every pinned variant of tests/test_gpu_kernel_choice.py and tests/test_gpu_exec_seg.py
  b  the executor in segments over every segment size and fill kernel, the frames it gives up on included
  c  the fused entropy kernel (zk_k_entropy_frame), which a batch gets by a COUNT (blocks that define a table <= frames), on batches of
     foreign frames that meet that count -- against the two kernels side by side, and damaged against the oracle

The archives and what the tests take for granted about them are tests/helpers/gen_batches.py's; every frame is generated once per process.
Expected bytes are the generator's model, which libzstd 1.5.7 confirms on the CPU for these very seeds (tests/test_generated_frames.py:
test_new_keywords_mean_what_libzstd_says, test_the_gpu_tests_seeds_reach_what_they_are_for, test_dense_frames_overflow_their_segments).
Every decode verifies checksums (but the damaged one) into a poisoned buffer; every status must be 0."""
import functools

import numpy as np
import pytest

from conftest import offsets_from_frames
from helpers import gen_batches as G
from helpers.dev_decode import decode as _decode, dev as _dev, upload as _upload
from oracle import zko
from test_gpu_exec_seg import VARIANTS as SEG_VARIANTS
from test_gpu_kernel_choice import VARIANTS as KERNEL_VARIANTS

pytestmark = pytest.mark.gpu

ALL_VARIANTS = {**KERNEL_VARIANTS, **SEG_VARIANTS}
assert len(ALL_VARIANTS) == len(KERNEL_VARIANTS) + len(SEG_VARIANTS) == 18
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _archive(name):
    """-> (compressed bytes + 8 of padding, compressed offsets, decoded offsets, decoded bytes)"""
    batch = {"default": lambda: G.frames(G.DEFAULT_SEEDS), "long": lambda: G.frames(G.LONG_SEEDS, "long"), "tail": lambda: G.frames(G.TAIL_SEEDS, "tail"),
             "dense0": lambda: G.frames(G.DENSE_SEEDS[:1], "dense"), "dense1": lambda: G.frames(G.DENSE_SEEDS[1:], "dense"),
             # redone and ordinary frames side by side in one launch
             "segments": lambda: G.frames(G.LONG_SEEDS[:12], "long") + G.frames(G.DENSE_SEEDS[:1], "dense") + G.frames(G.TAIL_SEEDS[:12], "tail")
                                 + G.frames(G.DENSE_SEEDS[1:], "dense") + G.frames(G.DEFAULT_SEEDS[:40])}[name]()
    comp, frames, data = G.archive(batch)
    c, d = offsets_from_frames(frames)
    return comp + b"\0" * 8, c, d, data


def _decode_host(engine, arch, first=0, count=None, verify=True):
    """zk_decode_frames as Engine.decode_frames calls it, into a poisoned buffer -> (bytes, statuses)"""
    import zeekstd_amd as zk
    comp, c, d, _ = arch
    buf = np.frombuffer(comp, np.uint8)
    if count is None:
        count = len(c) - 1 - first
    n = int(d[first + count] - d[first])
    out = np.full(max(n, 1), POISON, np.uint8)
    st = np.full(count, -1, np.int32)
    rc = zk.lib.zk_decode_frames(engine._h, buf.ctypes.data, buf.size, c.ctypes.data, d.ctypes.data, first, count, out.ctypes.data, n, int(verify), st.ctypes.data)
    assert rc > -1000, rc
    return out[:n].tobytes(), st


def _check(engine, arch, first=0, count=None, what=None):
    out, st = _decode_host(engine, arch, first, count)
    d, data = arch[2], arch[3]
    bad = np.flatnonzero(st)
    assert len(bad) == 0, (what, bad[:5], st[bad[:5]])
    count = len(d) - 1 - first if count is None else count
    assert out == data[int(d[first]):int(d[first + count])], what


# ------------------------------------------------------------------------------------------------ a: every pinned variant
@pytest.fixture(params=list(ALL_VARIANTS), ids=list(ALL_VARIANTS))
def pinned(request, engine):
    engine.set_kernel_choice(reset=0)
    engine.set_kernel_choice(**ALL_VARIANTS[request.param])
    yield engine
    engine.set_kernel_choice(reset=0)


def test_generated_frames_under_every_variant(pinned, request):
    """600 default frames (sizes of 0 and 1 ... 31 bytes among them: less than one XXH64 stripe), 60 frames with long blocks and 40 with
    literal runs and matches of up to a block's size, each archive whole; then sub-ranges of 1 ... 64 frames, which a host-pointer call
    takes down the small path unless the variant says otherwise (small_path=2: its entropy roles as two kernels).
    Under the xxh64=4 variants how many frames the waves beside the executor verify is printed, not asserted: it is the dispatcher's
    habit, and what they leave is verified behind the executor (tests/test_gpu_kernel_choice.py, test_checksums_beside_the_executor)."""
    sizes = np.diff(_archive("default")[2].astype(np.int64))
    assert (sizes == 0).any() and ((sizes > 0) & (sizes < 32)).any()
    for name in ("default", "long", "tail"):
        _check(pinned, _archive(name), what=name)
        if ALL_VARIANTS[request.node.callspec.id].get("xxh64") == 4:
            print(name, "frames verified beside the executor:", pinned.checksums_followed(), "of", len(_archive(name)[1]) - 1)
    arch = _archive("default")
    for first, count in ((0, 1), (17, 2), (100, 31), (333, 64), (599, 1)):
        assert int(arch[2][first + count] - arch[2][first]) <= 4 << 20, "a request the small path takes"
        _check(pinned, arch, first, count, what=(first, count))
    _check(pinned, _archive("tail"), 5, 3, what="tail, three frames")


# ------------------------------------------------------------------------------------------------ b: the executor in segments
SEG_SWEEP = [(kib, fill) for kib in (1, 4, 32, 0) for fill in (1, 2, 3)]


@pytest.mark.parametrize("seg_kib,seg_fill", SEG_SWEEP, ids=["seg%d_fill%d" % x for x in SEG_SWEEP])
def test_generated_frames_in_segments(engine, seg_kib, seg_fill):
    """Segments of 1 / 4 / 32 / 128 KiB under each fill kernel (zk_k_exec_fill<1024> / <256> / zk_k_exec_fill_lds): the long-block frames
    and the frames with block-long matches (segments cut at Raw, RLE and empty blocks, repeat offsets carried across the cuts with
    Literals_Length 0, matches that span many segments), each dense frame alone, and one batch with dense and ordinary frames side by side.
    The dense frames (32 512+ matches of 3 and 4 bytes in a block) are the GIVE-UP path: a segment's region of out/4 + 8 hole records is
    too small for them, the frame is marked ZK_E_SEG_OVERFLOW and zk_k_exec<REDO> executes it again -- with segments of 1 ... 32 KiB;
    at 128 KiB such a frame is one segment and nothing overflows.  The device offers no read-back of "was redone": what ties these
    inputs to that path is the simulator's count for the same seeds, tests/test_generated_frames.py,
    test_dense_frames_overflow_their_segments."""
    engine.set_kernel_choice(reset=0)
    try:
        engine.set_kernel_choice(exec_seg=2, seg_kib=seg_kib, seg_fill=seg_fill, small_path=1)
        for name in ("long", "tail", "dense0", "dense1", "segments"):
            _check(engine, _archive(name), what=name)
    finally:
        engine.set_kernel_choice(reset=0)


def test_generated_frame_list_in_segments(engine):
    """zk_decode_frame_list_dev over the mixed batch with a shuffled id list that has repeats, segments of 4 KiB: `ids` and `out_off` in
    zk_k_exec_seg and the fill kernels, and in the executor that redoes the dense frames"""
    import torch
    comp, c, d, data = _archive("segments")
    nf = len(c) - 1
    rng = np.random.default_rng(12)
    ids = np.concatenate([rng.permutation(nf), rng.integers(0, nf, 20)]).astype(np.uint32)
    rng.shuffle(ids)
    dense_at = [12, 25]                                      # where _archive("segments") puts the dense frames
    assert all(int(d[i + 1] - d[i]) > 90000 for i in dense_at) and sum(int(np.count_nonzero(ids == i)) for i in dense_at) >= 2
    sizes = (d[ids.astype(np.int64) + 1] - d[ids.astype(np.int64)]).astype(np.uint64)
    off = np.zeros(len(ids) + 1, np.uint64); off[1:] = np.cumsum(sizes)
    d_comp, csize, d_c, d_d = _upload(comp[:-8], c, d)
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(_dev())
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(_dev())
    total = int(off[-1])
    engine.set_kernel_choice(reset=0)
    try:
        engine.set_kernel_choice(exec_seg=2, seg_kib=4)
        d_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=_dev())
        d_st = torch.full((len(ids),), -1, dtype=torch.int32, device=_dev())
        assert engine.decode_frame_list_dev(d_comp, csize, d_c, d_d, d_ids, d_off, len(ids), d_out, total, True, d_st) == 0
    finally:
        engine.set_kernel_choice(reset=0)
    assert int(d_st.abs().sum().item()) == 0
    out = d_out[:total].cpu().numpy().tobytes()
    for i, f in enumerate(ids):
        assert out[int(off[i]):int(off[i + 1])] == data[int(d[f]):int(d[f + 1])], (i, int(f))


# ------------------------------------------------------------------------------------------------ c: the fused entropy kernel
@functools.lru_cache(maxsize=None)
def _batch(name):
    batch = getattr(G, "batch_" + name)()
    comp, frames, data = G.archive(batch)
    c, d = offsets_from_frames(frames)
    return batch, G.blocks_of(batch), comp, c, d, data


def _fused_and_pair(engine, comp, c, d, data):
    """the batch under entropy=1 and entropy=2: which kernel ran, equal return codes and statuses, all of them 0, both outputs the model's"""
    arch = _upload(comp, c, d)
    nf, total = len(c) - 1, len(data)
    want = np.frombuffer(data, np.uint8)
    res = {}
    for setting in (1, 2):
        rc, out, st, fused = _decode(engine, setting, arch, nf, total, poison=POISON)
        assert fused == (setting == 2), "entropy=%d: the fused kernel %s" % (setting, "ran" if fused else "declined the batch")
        res[setting] = (rc, st)
        bad = np.flatnonzero(st)
        assert rc == 0 and len(bad) == 0, (setting, rc, bad[:5], st[bad[:5]])
        assert np.array_equal(out[:total].cpu().numpy(), want), setting
    assert res[1][0] == res[2][0] and np.array_equal(res[1][1], res[2][1])


def test_fused_kernel_on_frames_with_at_most_one_own_block(engine):
    """800 default frames with own_blocks <= 1 (every table mode, Raw / RLE / empty blocks, Treeless and 1-stream literals): per workgroup
    a mixed key per table, most lanes left to the quad pass behind the kernel, RLE_Mode blocks refused as candidates"""
    batch, blocks, comp, c, d, data = _batch("filtered")
    assert len(batch) == 800 and max(f.own for f in batch) <= 1
    assert sum(f.own for f in batch) <= len(batch)
    assert len({b["modes"] for b in blocks if b.get("modes") is not None}) >= 20
    assert any(b["keys"] is not None and not b["cand"] for b in blocks), "RLE_Mode blocks among them"
    _fused_and_pair(engine, comp, c, d, data)


def test_fused_kernel_on_a_batch_that_qualifies_in_aggregate(engine):
    """frames with three and more own blocks between frames with none: the count admits the batch, no frame of it is the encoder's shape"""
    batch, blocks, comp, c, d, data = _batch("aggregate")
    assert max(f.own for f in batch) >= 3
    assert sum(f.own for f in batch) <= len(batch)
    _fused_and_pair(engine, comp, c, d, data)


def test_fused_kernel_on_shared_tables(engine):
    """shared_tables frames (16 ... 80 blocks behind one description of all three tables): workgroups whose reference is shared by 8 and
    more lanes (the walk runs, the lanes that do not match are the quad pass's), references that lie in an earlier workgroup, and
    workgroups that leave at once because fewer than ZK_FSEP_MIN_SHARE = 8 lanes share a reference that is not predefined"""
    batch, blocks, comp, c, d, data = _batch("shared")
    assert sum(f.own for f in batch) <= len(batch)
    runs = G.share_runs(blocks)
    assert any(r.share >= 8 and not r.predef for r in runs)
    assert any(r.share >= 8 and not r.predef and r.share < sum(1 for b in blocks[r.first:r.first + 64] if b["keys"] is not None) for r in runs), "lanes that do not match"
    assert any(r.ref_before and r.share >= 8 for r in runs)
    assert any(not r.predef and r.share < 8 for r in runs)
    _fused_and_pair(engine, comp, c, d, data)


def test_fused_kernel_huffman_half(engine):
    """zk_huf_group<4096, true>: groups of 16 blocks with three and more trees of depth 11 (a pool of 4096 cells takes them in several
    passes, two waves in step through an LDS word), Treeless blocks whose tree was described in another group and in another workgroup,
    1-stream next to 4-stream literals, a last group of one to three blocks (the shadow lanes)"""
    batch, blocks, comp, c, d, data = _batch("huffman")
    assert sum(f.own for f in batch) <= len(batch)
    groups = G.huf_groups(blocks, pool=4096)
    assert any(g.depths.count(11) >= 3 and g.passes > 1 for g in groups)
    assert max(g.passes for g in groups) > max(g.passes for g in G.huf_groups(blocks, pool=8192)), "a pool of twice the size would need fewer passes"
    other_group, other_run = G.treeless_reach(blocks)
    assert other_group > 0 and other_run > 0
    assert any(g.streams >= {1, 4} for g in groups)
    assert len(blocks) % 16 in (1, 2, 3)
    _fused_and_pair(engine, comp, c, d, data)


def test_fused_kernel_on_damaged_frames_against_the_oracle(engine):
    """one to three flipped bits in about 150 of the 800 frames, checksums not verified: under both settings a frame is refused exactly
    where the oracle refuses it, and accepted frames carry the oracle's bytes.  (Differential; no damaged input is meant to fault.)"""
    batch, blocks, comp, c, d, data = _batch("filtered")
    rng = np.random.default_rng(31)
    bad = bytearray(comp)
    hit = sorted(int(x) for x in rng.choice(len(batch), 150, replace=False))
    for f in hit:
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(int(c[f]), int(c[f + 1])))] ^= 1 << int(rng.integers(0, 8))
    verdict = {}
    for f in hit:
        n = int(d[f + 1] - d[f])
        try:
            o, used = zko.frame_decode(bytes(bad[int(c[f]):int(c[f + 1])]), n + 64, False)
            verdict[f] = o if len(o) == n and used == int(c[f + 1] - c[f]) else None
        except zko.OracleError:
            verdict[f] = None
    assert sum(v is None for v in verdict.values()) > 30 and sum(v is not None for v in verdict.values()) > 10
    arch = _upload(bytes(bad), c, d)
    res = {}
    for setting in (1, 2):
        rc, out, st, fused = _decode(engine, setting, arch, len(batch), len(data), poison=POISON, verify=False)
        assert fused == (setting == 2)
        res[setting] = st
        got = out[:len(data)].cpu().numpy().tobytes()
        for f in range(len(batch)):
            lo, hi = int(d[f]), int(d[f + 1])
            want = verdict.get(f, data[lo:hi])
            assert (want is not None) == (st[f] == 0), (setting, f, int(st[f]))
            if want is not None:
                assert got[lo:hi] == want, (setting, f)
    assert np.array_equal(res[1] == 0, res[2] == 0)

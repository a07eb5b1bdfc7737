"""Frames no encoder here writes (tests/helpers/zstd_gen.py: every choice RFC 8878 leaves open drawn at random -- header forms, block types,
literal modes and header sizes, Treeless literals, the four modes per sequence table with random FSE distributions, repeat codes with and without
Literals_Length 0) through the real libzstd 1.5.7, the oracle and the kernels' lane code on the CPU (tests/sim/zk_sim.cpp, all three sequence
walks).  libzstd decides what a frame means; the generator's own model, the oracle and the lane code have to agree with it.  The kernels themselves:
tests/test_gpu_generated_frames.py.  (The goldens are what libzstd's encoder emits; this is the rest of the format.)"""
import collections

import pytest

from conftest import sim_decode
from helpers import gen_batches as G
from helpers import zstd_gen
from oracle import zko
from oracle import libzstd_ref as Z

WANTED = {"raw", "rle", "compressed", "single", "windowed", "fcs0", "fcs1", "fcs2", "fcs3", "checksum", "did_field", "unused_bit", "lit_raw", "lit_rle", "lit_huf", "lit_treeless",
          "lit_hdr1", "lit_hdr2", "lit_hdr3", "huf_streams1", "huf_streams4", "huf_fmt0", "huf_fmt1", "huf_fmt2", "huf_fmt3", "huf_weights_direct", "huf_weights_fse", "fse_lowprob",
          "nseq_form1", "nseq_form2", "off_new", "rep_idx0", "rep_idx1", "rep_idx2", "rep_idx3"} | {"%s_mode%d" % (t, m) for t in ("ll", "of", "ml") for m in range(4)}


def test_generated_frames_mean_what_libzstd_says():
    ref = "1.5.7" if Z.load("1.5.7") is not None else "system"
    if Z.load(ref) is None:
        pytest.skip("no libzstd in the image")
    seen = collections.Counter()
    for seed in range(1500):
        f, out, feats = zstd_gen.generate(seed, zko.xxh64)
        got, state = Z.decode_stream_verdict(f, ref)
        assert state == "end" and got == out, (seed, state, len(got), len(out), sorted(feats))
        o, used = zko.frame_decode(f, len(out) + 64, True)
        assert used == len(f) and o == out, (seed, sorted(feats))
        seen.update(feats)
    assert not WANTED - set(seen), WANTED - set(seen)


@pytest.mark.parametrize("quad", [False, True, 2])
def test_generated_frames_through_the_lane_code(quad):
    for seed in range(600):
        f, out, feats = zstd_gen.generate(seed, zko.xxh64)
        rc, o, st = sim_decode(f, [(len(f), len(out))], quad=quad)
        assert rc == 0 and o == out, (seed, rc, sorted(feats))


def test_generated_frames_through_the_executor_in_segments():
    """several "workgroups" per frame (zk_k_seg_prep / zk_k_exec_seg / zk_k_exec_fill): segments of one block or a few, of a few hundred
    bytes (a segment per block: every offset across a block's first byte is a hole), fill rounds of 3 ... 1024 lanes"""
    for seed in range(600):
        f, out, feats = zstd_gen.generate(seed, zko.xxh64)
        seg = ((131072, 64, 2), (1 + seed % 5000, 3 + seed % 200, 2), (65536, 1024, 1))[seed % 3]
        rc, o, st = sim_decode(f, [(len(f), len(out))], seg=seg)
        assert rc == 0 and o == out, (seed, rc, seg, sorted(feats))


def test_generated_frames_side_by_side_in_one_archive():
    """many of them in one call: the block records of different frames sit side by side, Repeat / Treeless reach back inside their own frame only"""
    frames, comp, data = [], bytearray(), bytearray()
    for seed in range(2000, 2300):
        f, out, _ = zstd_gen.generate(seed, zko.xxh64)
        frames.append((len(f), len(out))); comp += f; data += out
    for quad in (False, 2):
        rc, o, st = sim_decode(bytes(comp), frames, quad=quad)
        assert rc == 0 and not st.any() and o == bytes(data)


def test_generated_frames_with_long_blocks():
    """thousands of sequences per block, literal sections of tens of KiB (4-stream Huffman with the wide header forms), ten blocks per frame"""
    ref = "1.5.7" if Z.load("1.5.7") is not None else "system"
    for seed in range(150):
        f, out, feats = zstd_gen.generate(100000 + seed, zko.xxh64, max_blocks=10, max_seq=4000, max_lit=100000)
        if Z.load(ref) is not None:
            assert Z.decode_stream_verdict(f, ref) == (out, "end"), seed
        o, used = zko.frame_decode(f, len(out) + 64, True)
        assert used == len(f) and o == out, seed
        for quad in (False, True, 2):
            rc, so, st = sim_decode(f, [(len(f), len(out))], quad=quad)
            assert rc == 0 and so == out, (seed, quad)
        rc, so, st = sim_decode(f, [(len(f), len(out))], seg=(131072, 256, 1))
        assert rc == 0 and so == out, seed
        # the executor in segments (several workgroups per frame): segments of 128 KiB and of a few hundred bytes
        for seg in ((131072, 64, 2), (700 + seed % 3000, 16, 2)):
            rc, so, st = sim_decode(f, [(len(f), len(out))], seg=seg)
            assert rc == 0 and so == out, (seed, seg)


def test_generated_frames_against_a_prefix():
    """the same against a raw-content prefix (ZSTD_DCtx_refPrefix): offsets reach across the frame's first byte into it, within the window"""
    ref = "1.5.7" if Z.load("1.5.7") is not None else "system"
    into = 0
    for seed in range(500):
        prefix = zko.gen_text(1 + (seed * 7919) % 90000, seed % 7)
        f, out, feats = zstd_gen.generate(300000 + seed, zko.xxh64, prefix=prefix)
        if Z.load(ref) is not None:
            assert Z.decode_stream(f, -1, ref, prefix=prefix, window_log_max=31) == out, seed
        o, used = zko.frame_decode(f, len(out) + 64, True, prefix=prefix)
        assert used == len(f) and o == out, seed
        rc, so, st = sim_decode(f, [(len(f), len(out))], prefix=prefix, quad=(False, True, 2)[seed % 3])
        assert rc == 0 and so == out, seed
        into += "off_into_prefix" in feats
    assert into > 100


def test_generated_frames_with_more_than_0x7F00_sequences_in_a_block():
    """the three-byte Number_of_Sequences: 32 512 ... 38 000 matches of three or four bytes back to back (the densest a block can be)"""
    ref = "1.5.7" if Z.load("1.5.7") is not None else "system"
    for seed in range(4):
        f, out, feats = zstd_gen.generate(500000 + seed, zko.xxh64, dense=True, max_blocks=8)
        assert "nseq_form3" in feats
        if Z.load(ref) is not None:
            assert Z.decode_stream_verdict(f, ref) == (out, "end"), seed
        o, used = zko.frame_decode(f, len(out) + 64, True)
        assert used == len(f) and o == out, seed
        for quad in (False, True, 2):
            rc, so, st = sim_decode(f, [(len(f), len(out))], quad=quad)
            assert rc == 0 and so == out, (seed, quad)



@pytest.mark.parametrize("quad", [False, 2])
def test_damaged_generated_frames_the_lane_code_against_the_oracle(quad):
    """one to three flipped bits per hit frame, checksums not verified: the lane code refuses exactly the frames the oracle refuses and yields its
    bytes otherwise (tests/test_gpu_generated_frames.py does this with the kernels)"""
    import numpy as np
    frames, comp, data = [], bytearray(), bytearray()
    for seed in range(20000, 20400):
        f, out, _ = zstd_gen.generate(seed, zko.xxh64)
        frames.append((len(f), len(out))); comp += f; data += out
    c = np.concatenate([[0], np.cumsum([f[0] for f in frames])]); d = np.concatenate([[0], np.cumsum([f[1] for f in frames])])
    rng = np.random.default_rng(9)
    bad = bytearray(comp)
    hit = set()
    for _ in range(300):
        i = int(rng.integers(0, len(bad)))
        bad[i] ^= 1 << int(rng.integers(0, 8))
        hit.add(int(np.searchsorted(c, i, side="right")) - 1)
    # checksum verification off: the simulator's checksum pass is separate (sim_decode runs the format checks only)
    rc, out, st = sim_decode(bytes(bad), frames, quad=quad)
    refused = 0
    for f in range(len(frames)):
        lo, hi = int(d[f]), int(d[f + 1])
        if f not in hit:
            assert st[f] == 0 and out[lo:hi] == bytes(data[lo:hi]), f
            continue
        try:
            o, used = zko.frame_decode(bytes(bad[int(c[f]):int(c[f + 1])]), hi - lo + 64, False)
            ok = len(o) == hi - lo and used == int(c[f + 1] - c[f])
        except zko.OracleError:
            ok = False
        assert ok == (st[f] == 0), (f, int(st[f]), ok)
        if ok:
            assert out[lo:hi] == o, f
        refused += not ok
    assert refused > 50


# ---- the keywords behind tests/test_gpu_generated_variants.py, on the very seeds it decodes (tests/helpers/gen_batches.py)
def test_default_arguments_keep_their_bytes():
    """every draw of the new keywords sits behind its keyword: a default frame's bytes are what they were (XXH64 of the first 200 seeds' frames,
    recorded before the keywords existed), and stats=True changes nothing but the return value"""
    h = zko.xxh64(b"".join(zstd_gen.generate(seed, zko.xxh64)[0] for seed in range(200)))
    assert h == 0xA102EF72F9DCAE2E
    for seed in (0, 7, 123):
        assert zstd_gen.generate(seed, zko.xxh64, stats=True)[:3] == zstd_gen.generate(seed, zko.xxh64)


@pytest.mark.parametrize("kind,seeds", [("shared", G.SHARED_SEEDS), ("tail", G.TAIL_SEEDS)], ids=["shared_tables", "max_ll_max_ml"])
def test_new_keywords_mean_what_libzstd_says(kind, seeds):
    """shared_tables and max_ll / max_ml through libzstd 1.5.7 (the judge), the oracle, the lane code in all three sequence walks and the
    executor in segments"""
    ref = "1.5.7" if Z.load("1.5.7") is not None else "system"
    if Z.load(ref) is None:
        pytest.skip("no libzstd in the image")
    for f in G.frames(seeds, kind):
        assert Z.decode_stream_verdict(f.comp, ref) == (f.data, "end"), f.seed
        o, used = zko.frame_decode(f.comp, len(f.data) + 64, True)
        assert used == len(f.comp) and o == f.data, f.seed
        for quad in (False, True, 2):
            rc, so, st = sim_decode(f.comp, [(len(f.comp), len(f.data))], quad=quad)
            assert rc == 0 and so == f.data, (f.seed, quad)
        for seg in ((131072, 64, 2), (1 + f.seed % 5000, 3 + f.seed % 200, 2), (65536, 1024, 1), (131072, 256, 1), (700 + f.seed % 3000, 16, 2)):
            rc, so, st = sim_decode(f.comp, [(len(f.comp), len(f.data))], seg=seg)
            assert rc == 0 and so == f.data, (f.seed, seg)
        assert len(f.facts) >= (16 if kind == "shared" else 1)


def test_the_gpu_tests_seeds_reach_what_they_are_for():
    """what the generator could not draw before, on the seeds the GPU tests use: every Literals_Length code 0 ... 35 and every Match_Length
    code 0 ... 52 (the ones with 11 ... 16 extra bits among them), a match of more than 65 538 bytes at offset 1, a literal run of 65 536 and
    more, Huffman trees of depth 11, Treeless literals whose tree was described in another group of 16 blocks of the batch"""
    tail = G.blocks_of(G.frames(G.TAIL_SEEDS, "tail"))
    ll, ml = set(), set()
    for b in tail:
        ll |= b.get("ll_codes", set()); ml |= b.get("ml_codes", set())
    for b in G.blocks_of(G.frames(G.SHARED_SEEDS, "shared")):
        ll |= b.get("ll_codes", set()); ml |= b.get("ml_codes", set())
    assert ll == set(range(36)), set(range(36)) - ll
    assert ml == set(range(53)), set(range(53)) - ml
    assert max(b.get("max_ml_off1", 0) for b in tail) > 65538
    assert max(b.get("max_ll", 0) for b in tail) >= 65536
    for name in ("shared", "huffman"):
        blocks = G.blocks_of(getattr(G, "batch_" + name)())
        assert any(g.depths.count(11) >= 3 for g in G.huf_groups(blocks)), name
        other_group, other_run = G.treeless_reach(blocks)
        assert other_group > 0 and other_run > 0, name


def test_block_facts_against_the_device_walk():
    """the facts a GPU test computes its premises from are the generator's own account (generate(..., stats=True)); the block walker of
    tests/helpers/enc_inputs.py reads the same block types, literal types and sizes, Huffman depths, sequence counts and modes bytes back
    from the frame's BYTES wherever it knows the header forms, and the same count of own blocks by zk_device.h's rule,
    (m ^ (m >> 1)) & 0x54 on the modes byte"""
    from helpers import enc_inputs
    seen = 0
    for f in G.frames(G.DEFAULT_SEEDS[:300]):
        try:
            walked = enc_inputs.walk_frame(f.comp)
        except AssertionError:
            continue                                         # Treeless literals, FSE-compressed weights, RLE_Mode tables: not that walker's
        assert [b["type"] for b in walked] == [b["type"] for b in f.facts], f.seed
        for w, b in zip(walked, f.facts):
            if w["type"] == "comp":
                assert (w["nseq"], w["modes"], w["nlit"], w["lit"]) == (b["nseq"], b["modes"], b["nlit"], b["lit"]), f.seed
                if w["lit"] == "huf":
                    assert w["huf_depth"] == b["huf_depth"], f.seed
        assert f.own == sum(1 for w in walked if w.get("modes") and (w["modes"] ^ (w["modes"] >> 1)) & 0x54)
        seen += 1
    assert seen > 60


def test_dense_frames_overflow_their_segments():
    """The premise of tests/test_gpu_generated_variants.py, test_generated_frames_in_segments: the dense frames it decodes have more hole
    records than a segment's region of out/4 + 8 holds (cap_shift = 2, the device's), with segments of 32 KiB and of 1 KiB -- the frame is
    given up and executed again by the frame executor (the simulator counts it), and the bytes are the model's.  A frame that is ONE
    segment of 128 KiB does not overflow."""
    import ctypes as C
    from conftest import sim_lib
    a = (C.c_uint64 * 4)()
    for f in G.frames(G.DENSE_SEEDS, "dense"):
        for seg_bytes, redone in ((32768, True), (1024, True), (131072, False)):
            sim_lib().zk_sim_seg_stats(a, 1)
            rc, out, st = sim_decode(f.comp, [(len(f.comp), len(f.data))], seg=(seg_bytes, 64, 2))
            assert rc == 0 and not st.any() and out == f.data, (f.seed, seg_bytes)
            sim_lib().zk_sim_seg_stats(a, 1)
            assert (a[3] > 0) == redone, (f.seed, seg_bytes, list(a))


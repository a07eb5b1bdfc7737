"""Dictionaries nobody trained and frames no encoder writes against them (tests/helpers/zstd_gen.py: make_dictionary, generate(dictionary=))
on the CPU.  libzstd 1.5.7 decides what a (dictionary, frame) pair means (ZSTD_decompress_usingDict) and which damaged dictionaries load
(ZSTD_DCtx_loadDictionary); the generator's model, the oracle (zko.frame_decode(dictionary=)), zk_dict_create and the kernels' lane code
(tests/sim/zk_sim_dict.cpp) have to agree with it.  The batches tests/test_gpu_generated_dict.py decodes on the device are judged here
on the very seeds it uses, and the facts it takes for granted about them are asserted (tests/helpers/gen_batches.py).
(tests/test_dict.py and tests/test_sim_dict.py: one dictionary libzstd trained, and what its encoder writes against it.)"""
import collections
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import gen_batches as G
from helpers import libzstd_dict, sim_dict, zstd_gen
from oracle import zko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a few dozen dictionaries: thirty as the seed draws them, the rest with one draw pinned to an edge each
DICT_KW = [dict(seed=s) for s in range(30)] + [
    dict(seed=30, dict_id=0), dict(seed=31, content_size=1), dict(seed=32, content_size=7), dict(seed=33, content_size=8),
    dict(seed=34, content_size=9), dict(seed=35, content_size=150000, reps=(150000, 150000, 1)), dict(seed=36, alphabet=2, weights="direct"),
    dict(seed=37, alphabet=256, weights="fse"), dict(seed=38, depth=11, weights="direct"), dict(seed=39, als={"of": 5, "ll": 5, "ml": 5}),
    dict(seed=40, als={"of": 8, "ll": 9, "ml": 9}), dict(seed=41, alphabet=2, weights="fse", reps=(1, 1, 1))]
FRAMES_PER_DICT = 24                                         # 42 x 24: about a thousand frames

WANTED = ({"dict_treeless_first_1stream", "dict_treeless_first_4streams", "dict_table_after_redefine", "dict_first_comp_not_block0",
           "off_into_dict", "off_dict_first_byte", "match_straddles_frame_start", "did_width1", "did_width2", "did_width4", "did_absent"}
          | {"dict_rep_first_idx%d" % i for i in range(4)} | {"dict_%s_repeat" % t for t in ("ll", "of", "ml")}
          | {"dict_%s_repeat_%s_mode%d" % (t, o, m) for t in ("ll", "of", "ml") for o in ("ll", "of", "ml") if o != t for m in (0, 1, 2)})


@pytest.fixture(scope="module")
def judge():
    j = libzstd_dict.judge()
    if j is None:
        pytest.skip("libzstd 1.5.7 is not in this image")
    yield j
    j.close()


_PAIRS = {}


def pairs(i):
    """dictionary i of DICT_KW and its frames, made once: (bytes, model, [(frame, decoded, features)])"""
    if i not in _PAIRS:
        d, m = zstd_gen.make_dictionary(**DICT_KW[i])
        _PAIRS[i] = (d, m, [zstd_gen.generate(1000000 + 1000 * i + k, zko.xxh64, dictionary=m) for k in range(FRAMES_PER_DICT)])
    return _PAIRS[i]


def test_the_dictionaries_reach_what_they_are_for():
    """what make_dictionary draws, over DICT_KW: IDs for every width of the Dictionary_ID field and 0, both forms of weights, alphabets of 2
    and of 256 symbols, a tree of depth 11, every table's accuracy log at both ends, "less than 1" probabilities and absent symbols in
    every table, the content sizes at the edges, repeat offsets of 1, of the content size, equal ones"""
    ms = [pairs(i)[1] for i in range(len(DICT_KW))]
    ids = [m.id for m in ms]
    assert 0 in ids and any(0 < x < 256 for x in ids) and any(256 <= x < 65536 for x in ids) and any(x >= 65536 for x in ids)
    assert {m.huf_form for m in ms} == {"direct", "fse"}
    assert {2, 256} <= {len(m.huf.code) for m in ms} and 11 in {m.huf.maxbits for m in ms} and 1 in {m.huf.maxbits for m in ms}
    for t, lo, hi, nsym in (("of", 5, 8, 32), ("ml", 5, 9, 53), ("ll", 5, 9, 36)):
        assert {lo, hi} <= {m.tables[t][1] for m in ms}, t
        assert any(-1 in m.norms[t] for m in ms) and any(0 in m.norms[t] or len(m.norms[t]) < nsym for m in ms), t
    sizes = {len(m.content) for m in ms}
    assert {1, 7, 8, 9} <= sizes and any(100 <= x < 1000 for x in sizes) and any(1024 <= x <= 8192 for x in sizes) and any(x > 1 << 17 for x in sizes)
    assert any(1 in m.rep for m in ms) and any(len(m.content) in m.rep and len(m.content) > 1 for m in ms)
    assert any(len(set(m.rep)) < 3 and max(m.rep) > 1 for m in ms)
    # each description's length feeds the image zk_dict_block re-orders: many values of each
    for name in ("huf", "of", "ml", "ll"):
        assert len({m.spans[name][1] for m in ms}) >= 8, name


def test_generated_pairs_mean_what_libzstd_says(judge):
    """libzstd is the judge: the generator's model and the oracle agree with ZSTD_decompress_usingDict byte for byte, and the draws reach
    every feature named"""
    seen = collections.Counter()
    for i in range(len(DICT_KW)):
        d, m, frames = pairs(i)
        assert judge.load_dictionary(d) == 0, DICT_KW[i]
        for k, (f, out, feats) in enumerate(frames):
            assert judge.using_dict(f, len(out) + 64, d) == out, (DICT_KW[i], k, sorted(feats))
            o, used = zko.frame_decode(f, len(out) + 64, True, dictionary=d)
            assert used == len(f) and o == out, (DICT_KW[i], k, sorted(feats))
            seen.update(feats)
    assert not WANTED - set(seen), WANTED - set(seen)


def test_raw_content_and_wrong_dictionaries(judge):
    """anything that is not a formatted dictionary lends its bytes only; a frame that names another ID than the loaded one is refused (32)"""
    d, m = zstd_gen.raw_dictionary(zko.gen_text(3000, 5))
    for k in range(40):
        f, out, feats = zstd_gen.generate(2000000 + k, zko.xxh64, dictionary=m)
        assert judge.using_dict(f, len(out) + 64, d) == out, k
        assert zko.frame_decode(f, len(out) + 64, True, dictionary=d) == (out, len(f)), k
        assert sim_dict.decode(f, [(len(f), len(out))], d)[1] == out, k
    da, ma, fa = pairs(5)
    db, mb, fb = pairs(9)
    assert ma.id != mb.id and ma.id and mb.id
    for f, out, feats in fa:
        named = "did_absent" not in feats
        got = judge.using_dict(f, len(out) + 64, db)
        assert (got == -32) == named, sorted(feats)
        if named:
            with pytest.raises(zko.OracleError) as e:
                zko.frame_decode(f, len(out) + 64, True, dictionary=db)
            assert e.value.code == 32
            assert sim_dict.decode(f, [(len(f), len(out))], db)[2][0] == 32


def test_zk_dict_create_reports_the_generators_id_and_content_offset():
    for i in range(len(DICT_KW)):
        d, m, _ = pairs(i)
        h = zk.Dictionary(d)
        assert (h.id, h.content_offset) == (m.id, m.content_offset), DICT_KW[i]
        assert zko.dict_check(d) == (m.id, m.content_offset), DICT_KW[i]
    for name in G.DICTS:
        d, m = G.dictionary(name)
        h = zk.Dictionary(d)
        assert (h.id, h.content_offset) == (m.id, m.content_offset), name


def damaged_dictionaries(d, m, rng):
    """(what was done, bytes): cuts, a repeat offset of 0 and of content size + 1 in each place, a flipped bit in each description"""
    at, n = m.spans["rep"][0], len(m.content)
    for cut in (7, 8, 9, m.spans["huf"][0] + 1, m.spans["of"][0], m.spans["of"][0] + 1, m.spans["ml"][0], m.spans["ml"][0] + 1, m.spans["ll"][0],
                m.spans["ll"][0] + 1, at, at + 5, at + 11, at + 12, m.content_offset + max(m.rep) - 1):
        yield "cut at %d" % cut, d[:cut]
    for k in range(3):
        for v in (0, n + 1, 0xFFFFFFFF):
            yield "offset %d = %d" % (k, v), d[:at + 4 * k] + struct.pack("<I", v) + d[at + 4 * k + 4:]
    for name in ("huf", "of", "ml", "ll"):
        lo, ln = m.spans[name]
        for _ in range(6):
            i, bit = lo + rng.randrange(ln), rng.randrange(8)
            yield "%s: bit %d of byte %d" % (name, bit, i - lo), d[:i] + bytes([d[i] ^ (1 << bit)]) + d[i + 1:]


def test_damaged_generated_dictionaries_get_libzstds_verdict(judge):
    """zk_dict_create refuses (-30) exactly what ZSTD_DCtx_loadDictionary refuses (with whatever code: it reports a dictionary it cannot
    digest as a failed allocation), and so does the oracle"""
    import random
    rng = random.Random(11)
    refused = loaded = 0
    for i in range(len(DICT_KW)):
        d, m, frames = pairs(i)
        for what, bad in damaged_dictionaries(d, m, rng):
            want = 30 if judge.load_dictionary(bad) else 0
            h = C.c_void_p()
            buf = (C.c_uint8 * max(len(bad), 1)).from_buffer_copy(bad.ljust(1, b"\0"))
            rc = zk.lib.zk_dict_create(buf, len(bad), C.byref(h))
            assert rc == -want and bool(h.value) == (rc == 0), (DICT_KW[i], what, rc, want)
            if rc == 0:
                zk.lib.zk_dict_free(h)
            try:
                zko.dict_check(bad); ok = True
            except zko.OracleError as e:
                assert e.code == 30
                ok = False
            assert ok == (want == 0), (DICT_KW[i], what, want)
            refused += want != 0; loaded += want == 0
    assert refused > 300 and loaded > 100, (refused, loaded)


def test_a_tree_without_two_leaves_of_weight_1_is_refused(judge):
    """The weights (2, 2) describe the tree of (1, 1), and the lane code builds a table from them; HUF_readStats wants the symbols of
    weight 1 two at least and even in number, so libzstd loads no such dictionary -- and zk_dict_create did (found by seed 17 of DICT_KW,
    "huf: bit 4 of byte 29")."""
    d, m, _ = pairs(36)                                      # two symbols, direct weights: the one weight written is a 1
    lo, ln = m.spans["huf"]
    sym = min(m.huf.code)
    i = lo + 1 + sym // 2
    assert (d[i] >> (0 if sym & 1 else 4)) & 15 == 1
    bad = d[:i] + bytes([d[i] ^ (3 << (0 if sym & 1 else 4))]) + d[i + 1:]
    assert judge.load_dictionary(bad) != 0
    h = C.c_void_p()
    assert zk.lib.zk_dict_create((C.c_uint8 * len(bad)).from_buffer_copy(bad), len(bad), C.byref(h)) == -30 and not h.value
    with pytest.raises(zko.OracleError):
        zko.dict_check(bad)


def test_where_zk_dict_create_is_stricter_than_libzstd(judge):
    """The one damaged description known on which the verdicts part (a campaign over 150 further dictionaries found four of its kind and
    nothing else): the written weights alone sum to 2^11, so the implied last weight is 12 and the tree 12 bits deep.  RFC 8878 4.2.1
    allows 11; libzstd's table has room for 12 (HUF_TABLELOG_MAX) and it loads the dictionary.  The kernels' tables hold 2^11 cells:
    zk_dict_create and the oracle refuse, as they refuse such a tree in a frame."""
    d, m = zstd_gen.make_dictionary(1022)
    lo, ln = m.spans["huf"]
    assert m.huf_form == "direct" and m.huf.maxbits == 11
    bad = d[:lo + 22] + bytes([d[lo + 22] ^ 1]) + d[lo + 23:]           # weight 4 -> 5
    n = bad[lo] - 127
    w = [(bad[lo + 1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
    assert sum(1 << (x - 1) for x in w if x) == 1 << 11
    assert judge.load_dictionary(bad) == 0
    h = C.c_void_p()
    assert zk.lib.zk_dict_create((C.c_uint8 * len(bad)).from_buffer_copy(bad), len(bad), C.byref(h)) == -30 and not h.value
    with pytest.raises(zko.OracleError):
        zko.dict_check(bad)


def test_generated_pairs_through_the_lane_code():
    """tests/sim/zk_sim_dict.cpp: every frame alone, and a dictionary's frames side by side in one call (the dictionary's block entry sits
    behind the blocks of all of them)"""
    for i in range(len(DICT_KW)):
        d, m, frames = pairs(i)
        for k, (f, out, feats) in enumerate(frames):
            rc, o, st = sim_dict.decode(f, [(len(f), len(out))], d)
            assert rc == 0 and st[0] == 0 and o == out, (DICT_KW[i], k, int(st[0]), sorted(feats))
        rc, o, st = sim_dict.decode(b"".join(f for f, _, _ in frames), [(len(f), len(out)) for f, out, _ in frames], d)
        assert rc == 0 and not st.any() and o == b"".join(out for _, out, _ in frames), (DICT_KW[i], np.flatnonzero(st)[:5])


# ---------------------------------------------------------------------------------------------- damaged frames
@pytest.mark.parametrize("name", G.DAMAGED_DICTS)
def test_damaged_generated_frames_the_lane_code_against_the_oracle(name):
    """one to three flipped bits per hit frame, checksums not verified: the lane code with the dictionary refuses exactly the frames the
    oracle with the dictionary refuses, and yields its bytes otherwise (tests/test_gpu_generated_dict.py does this with the kernels)"""
    bad, sizes, hit, _ = G.dict_damaged(name)
    assert len(hit) > 40
    want = G.dict_damaged_verdicts(name)
    assert sum(1 for f in hit if want[f] is None) >= G.REFUSED_FLOOR * len(hit)        # the oracle alone clears the floor
    rc, out, st = sim_dict.decode(bad, sizes, G.dictionary(name)[0])
    assert rc == 0
    G.dict_damaged_judge(name, out, st)


def _sanitizer_build(tmp_path, cc, src, exe):
    if shutil.which(cc[0]) is None:
        pytest.skip("no " + cc[0])
    r = subprocess.run(cc + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for %s here" % cc[0])
    assert r.returncode == 0, r.stderr[-2000:]


def _case_file(path, sizes, comp, data=None):
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQ", len(sizes), len(comp), len(data) if data is not None else sum(s[1] for s in sizes)))
        for c, d in sizes:
            f.write(struct.pack("<QQ", c, d))
        f.write(comp)
        if data is not None:
            f.write(data)


def test_lane_code_with_a_dictionary_under_sanitizers(tmp_path):
    """tests/sim/dict_fuzz.cpp, a program of its own under AddressSanitizer + UBSan, every buffer an exact-size heap allocation: the very
    damaged bytes of the test above (its statuses must be the shared library's), then the same frames damaged further and, every fourth
    round, against a damaged dictionary; and undamaged frames of the dictionaries at the content-size edges"""
    exe = str(tmp_path / "dict_fuzz")
    _sanitizer_build(tmp_path, ["g++", "-std=c++17"], os.path.join(ROOT, "tests", "sim", "dict_fuzz.cpp"), exe)
    first = True

    def run(tag, dictionary, sizes, comp, iters):
        nonlocal first
        case, dpath = str(tmp_path / (tag + ".bin")), str(tmp_path / (tag + ".dict"))
        _case_file(case, sizes, comp)
        with open(dpath, "wb") as f:
            f.write(dictionary)
        r = subprocess.run([exe, case, dpath, str(iters), "5"], capture_output=True, text=True, timeout=600)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (tag, r.stdout[-300:], r.stderr[-3000:])
        return [int(x) for x in r.stdout.splitlines()[0].split()[1:]]
    for name in G.DAMAGED_DICTS:
        bad, sizes, hit, _ = G.dict_damaged(name)
        d = G.dictionary(name)[0]
        assert run(name, d, sizes, bad, 40) == list(sim_dict.decode(bad, sizes, d)[2]), name
    for name in ("one_byte", "seven", "eight", "big"):
        comp, sizes, _ = G.archive(G.dict_frames(name)[:40])
        assert not any(run(name, G.dictionary(name)[0], sizes, comp, 60)), name


def test_oracle_with_a_dictionary_under_sanitizers(tmp_path):
    """tests/sim/oracle_fuzz.c with a dictionary argument: the checker reads damaged frames against a dictionary, and damaged dictionaries,
    without leaving its buffers (exact-size heap copies, no padding)"""
    exe = str(tmp_path / "oracle_fuzz")
    _sanitizer_build(tmp_path, ["gcc", "-w"], os.path.join(ROOT, "tests", "sim", "oracle_fuzz.c"), exe)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    first = True
    for name in ("one_byte", "nine", "wide", "big"):
        comp, sizes, data = G.archive(G.dict_frames(name)[:40])
        case, dpath = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".dict"))
        _case_file(case, sizes, comp, data)
        with open(dpath, "wb") as f:
            f.write(G.dictionary(name)[0])
        r = subprocess.run([exe, case, "60", "3", dpath], capture_output=True, text=True, timeout=600, env=env)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (name, r.stdout[-300:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------- the GPU tests' batches (tests/helpers/gen_batches.py)
def gpu_frames():
    """every (dictionary name, Frame) tests/test_gpu_generated_dict.py decodes"""
    seen = {}
    for name in G.DICTS:
        if name != G.BIG_DICT:
            for f in G.dict_frames(name):
                seen[(name, f.kind, f.seed)] = f
    for batch in (G.dict_batch_big(), G.dict_batch_small(), G.dict_batch_mixed(), G.dict_batch_fused(), G.dict_batch_sizes()):
        for f in batch:
            seen[(f.dict, f.kind, f.seed)] = f
    return seen


def test_the_gpu_tests_frames_mean_what_libzstd_says(judge):
    """the expectation of the GPU tests is the generator's model: confirmed here for their seeds by libzstd, the oracle and the lane code"""
    by = collections.defaultdict(list)
    for (name, _, _), f in gpu_frames().items():
        by[name].append(f)
    assert set(by) == set(G.DICTS)
    for name, batch in by.items():
        d = G.dictionary(name)[0]
        for f in batch:
            assert judge.using_dict(f.comp, len(f.data) + 64, d) == f.data, (name, f.kind, f.seed)
            assert zko.frame_decode(f.comp, len(f.data) + 64, True, dictionary=d) == (f.data, len(f.comp)), (name, f.kind, f.seed)
        comp, sizes, data = G.archive(batch)
        rc, o, st = sim_dict.decode(comp, sizes, d)
        assert rc == 0 and not st.any() and o == data, (name, np.flatnonzero(st)[:5])


def test_premises_of_the_gpu_batches():
    """what tests/test_gpu_generated_dict.py takes for granted about its batches"""
    big = G.dict_batch_big()
    blocks = G.blocks_of(big)
    n = len(blocks)
    assert n > 4096 and n - len(big[-1].facts) <= 4096                    # just past zk_launch_fse's threshold: one frame fewer is not
    kinds = collections.Counter(G.run_kinds(blocks))
    assert kinds["dict"] >= 4 and kinds["dict+predef"] >= 1 and kinds["owned"] >= 4, kinds
    small = G.dict_batch_small()
    assert 1000 < sum(len(f.facts) for f in small) <= 4096 and {f.kind for f in small} == {"default", "shared"}
    # blocks_of understands the dictionary's key: a frame's first block with sequences that says Repeat_Mode has it, and so has Treeless
    # behind no tree of the frame's own; nothing in a frame written without a dictionary has
    first = [next((b for b in blocks if b["frame"] == fi and b["type"] == "comp" and b["modes"] is not None), None) for fi in range(len(big))]
    assert sum(1 for b in first if b and b["keys"] == (n, n, n)) > 20
    for b in first:
        if b:
            m = [(b["modes"] >> s) & 3 for s in (6, 4, 2)]
            assert all((k == n) == (mode == 3) for k, mode in zip(b["keys"], m)), b
    assert sum(1 for b in blocks if b["huf_at"] == n) > 20 and all(b["lit"] == "treeless" for b in blocks if b["huf_at"] == n)
    plain = G.blocks_of(G.frames(G.DEFAULT_SEEDS[:50]))
    assert not any(b["huf_at"] == len(plain) or (b["keys"] and len(plain) in b["keys"]) for b in plain)
    # the fused kernel's condition: blocks that define a table <= frames
    fused = G.dict_batch_fused()
    assert len(fused) >= 40 and sum(f.own for f in fused) <= len(fused) and any(f.own for f in fused)
    assert any(b["keys"] == (len(G.blocks_of(fused)),) * 3 for b in G.blocks_of(fused))
    # the size batch: no frame states its size
    sizes = G.dict_batch_sizes()
    assert len(sizes) >= 30 and {f.kind for f in sizes} == {"default", "shared"}
    for f in sizes:
        from helpers import dict_fixtures
        assert dict_fixtures.frame_facts(f.comp)["fcs"] is None, f.seed
    assert any("off_into_dict" in f.feats for f in sizes) and any(any(k.startswith("dict_") and k.endswith("_repeat") for k in f.feats) for f in sizes)
    # every route dictionary's frames reach into it and start from its state; all four widths of the ID field occur over the routes
    feats = collections.Counter()
    for name in G.ROUTE_DICTS:
        own = collections.Counter(x for f in G.dict_frames(name) for x in f.feats)
        assert own["off_into_dict"] and own["dict_ll_repeat"] + own["dict_of_repeat"] + own["dict_ml_repeat"] > 20, name
        assert own["dict_treeless_first_1stream"] + own["dict_treeless_first_4streams"], name
        feats.update(own)
    assert not {x for x in WANTED if not x.endswith("mode1")} - set(feats), WANTED - set(feats)

"""Encoding against a dictionary, the part that runs without a GPU: what zk_cdict_create builds from a dictionary and the rules
zk_encode_frames_dict* chooses a frame's tables by (zeekstd_amd/csrc/zk_enc_dict.h through tests/sim/zk_enc_dict_sim.cpp), and
zk_compress_bound_dict.  The decoder's lane code for the same descriptions and a restatement of the rules in Python
(tests/helpers/enc_dict_sim.py) are what they are held against.  tests/test_gpu_encode_dict.py has the frames."""
import os
import random
import shutil
import subprocess

import pytest

from helpers import enc_dict_sim as S
from helpers import zstd_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20

# generated dictionaries (tests/helpers/zstd_gen.make_dictionary, the keywords of tests/test_generated_dict.py): as the seed draws them, and
# with one draw pinned to an edge each -- sparse trees and tables among them
DICT_KW = [dict(seed=s) for s in range(30)] + [
    dict(seed=30, dict_id=0), dict(seed=31, content_size=1), dict(seed=36, alphabet=2, weights="direct"), dict(seed=37, alphabet=256, weights="fse"),
    dict(seed=38, depth=11, weights="direct"), dict(seed=39, als={"of": 5, "ll": 5, "ml": 5}), dict(seed=40, als={"of": 8, "ll": 9, "ml": 9}),
    dict(seed=41, alphabet=2, weights="fse", reps=(1, 1, 1)), dict(seed=42, wide=True)]
TABLES = (("ll", S.LL), ("of", S.OF), ("ml", S.ML))


@pytest.fixture(scope="module")
def dicts():
    """[(name, bytes, model or None)]: the fixture's three and the generated ones"""
    out = [(k, v, None) for k, v in S.fixture_dicts().items()]
    for kw in DICT_KW:
        d, m = zstd_gen.make_dictionary(**kw)
        out.append((str(kw), d, m))
    return out


def test_raw_content_has_no_tables(dicts):
    assert S.build(dict((n, d) for n, d, _ in dicts)["raw"]) is None
    assert S.build(b"") is None and S.build(b"abc") is None


def test_huffman_code_has_the_decoders_lengths_and_round_trips(dicts):
    """the code built from a dictionary assigns exactly the lengths zk_huf_read_weights derives (maxbits + 1 - weight, none without a
    weight), and literals written with it as zk_k_enc_dict_lits writes them come back through zk_huf_fill_table's table"""
    rng = random.Random(7)
    depths, alphabets = set(), set()
    for name, d, m in dicts:
        b = S.build(d)
        if b is None:
            continue
        w, n, mb = S.decoder_weights(d)
        assert b["maxbits"] == mb, name
        assert b["len"] == [mb + 1 - x if x else 0 for x in w], name
        if m is not None:
            assert {s for s in range(256) if b["len"][s]} == set(m.huf.code), name
        # a prefix code that fills the code space
        assert sum(1 << (mb - l) for l in b["len"] if l) == 1 << mb, name
        alphabet = [s for s in range(256) if b["len"][s]]
        depths.add(mb); alphabets.add(len(alphabet))
        for nl in (1, 2, 3, 255, 256, 1000):
            lits = bytes(rng.choice(alphabet) for _ in range(nl))
            assert S.huf_roundtrip(d, lits) == 0, (name, nl)
        missing = [s for s in range(256) if not b["len"][s]]
        if missing:
            assert S.huf_roundtrip(d, bytes([alphabet[0], missing[0]])) == -2, name
    assert {1, 11} <= depths and {2, 256} <= alphabets          # the generator's edges were reached


def test_fse_tables_round_trip_through_the_decoders_table(dicts):
    """a compression table built from the dictionary's description, walked as zk_k_enc_entropy's chain wave walks it, decodes through
    zk_fse_build's table for the same description; a code without a probability has no cost"""
    rng = random.Random(11)
    sparse = 0
    for name, d, m in dicts:
        b = S.build(d)
        if b is None:
            continue
        for key, t in TABLES:
            legal = [c for c in range(64) if b["cost"][t][c] != S.COST_NONE]
            if m is not None:
                norm, al = m.norms[key], m.tables[key][1]
                assert b["al"][t] == al, (name, key)
                assert legal == [c for c, x in enumerate(norm) if x != 0], (name, key)
                assert [b["cost"][t][c] for c in legal] == [S.sym_cost(norm[c], al) for c in legal], (name, key)
                sparse += len(legal) < S.NSYM[t]
            for n in (1, 2, 3, 50, 2000):
                syms = [rng.choice(legal) for _ in range(n)]
                assert S.fse_roundtrip(d, t, syms) == 0, (name, key, n)
            absent = [c for c in range(S.NSYM[t]) if c not in legal]
            if absent:
                assert S.fse_roundtrip(d, t, [legal[0], absent[0]]) == -2, (name, key)
    assert sparse >= 10


def test_symbol_costs():
    assert S.sym_cost(0, 6) == S.COST_NONE == S.lib().zk_enc_dict_sim_sym_cost(0, 6)
    for al in range(5, 10):
        for norm in [-1] + list(range(1, (1 << al) + 1)):
            got = S.lib().zk_enc_dict_sim_sym_cost(norm, al)
            assert got == S.sym_cost(norm, al), (norm, al)
            import math
            assert abs(got / 256 - (al - math.log2(max(norm, 1)))) < 2 / 256, (norm, al)


def test_legality_and_choice_against_brute_force(dicts):
    """per table: the dictionary's is refused exactly when a counted code has no probability in it, the frame's own exists exactly under
    the other routes' conditions, and the pick is the minimum of the legal costs"""
    rng = random.Random(13)
    picks, refused = {S.PREDEF: 0, S.OWN: 0, S.DICT: 0}, 0
    for name, d, m in dicts:
        b = S.build(d)
        if b is None:
            continue
        for key, t in TABLES:
            legal = [c for c in range(64) if b["cost"][t][c] != S.COST_NONE]
            top = 28 if t == S.OF else S.NSYM[t]            # (the matcher produces no offset code the predefined table lacks)
            for trial in range(12):
                nseq = rng.choice([1, 2, 10, 255, 256, 257, 3000, 20000])
                pool = legal if trial % 3 else list(range(top))
                pool = [c for c in pool if c < top] or [0]
                fav = rng.sample(pool, min(len(pool), rng.randint(1, 6)))
                hist = [0] * 64
                for _ in range(nseq):
                    hist[rng.choice(fav) if rng.random() < 0.8 else rng.choice(pool)] += 1
                nblk = rng.randint(1, 9)
                got, costs, dlen = S.choose(hist, t, nseq, nblk, b["cost"][t], b["al"][t])
                norm, al = S.PREDEF_NORMS[t]
                c_predef = S.table_cost(hist, [S.sym_cost(x, al) for x in norm]) + S.overhead(0, al, nblk)
                c_dict = S.table_cost(hist, b["cost"][t])
                assert costs[0] == c_predef, (name, key, trial)
                assert (costs[2] == S.NOT_LEGAL) == (c_dict is None), (name, key, trial)
                if c_dict is not None:
                    c_dict += S.overhead(0, b["al"][t], nblk)
                    assert costs[2] == c_dict
                else:
                    refused += 1
                own = costs[1] != S.NOT_LEGAL
                assert own == (nseq >= S.FSE_MIN_SEQ and sum(1 for x in hist if x) >= 2 and 0 < dlen <= S.DESC_CAP), (name, key, trial, nseq, dlen)
                assert got == S.pick(c_predef, costs[1] if own else None, c_dict), (name, key, trial, costs)
                assert costs[got] == min(c for c in costs if c != S.NOT_LEGAL)
                picks[got] += 1
    assert min(picks.values()) > 20 and refused > 20, (picks, refused)


def test_ties_go_to_the_other_routes_choice():
    P = S.lib().zk_enc_dict_sim_pick
    assert P(100, 0, 0, 1, 100) == S.PREDEF and P(100, 0, 0, 1, 99) == S.DICT and P(100, 0, 0, 0, 1) == S.PREDEF
    assert P(100, 1, 100, 1, 100) == S.OWN and P(99, 1, 100, 1, 99) == S.PREDEF and P(100, 1, 100, 1, 99) == S.DICT
    assert P(100, 1, 101, 1, 100) == S.PREDEF and P(100, 1, 90, 0, 1) == S.OWN


def test_dictionary_id_field_width():
    for i, w in ((0, 0), (1, 1), (255, 1), (256, 2), (65535, 2), (65536, 4), ((1 << 32) - 1, 4)):
        got = S.lib().zk_enc_dict_sim_id_width(i)
        assert got & 0xFF == w == S.id_width(i), i
        assert got >> 8 == {0: 0, 1: 1, 2: 2, 4: 3}[w], i            # Dictionary_ID_Flag


def test_treeless_section_size_and_header():
    # one stream below 256 literals: 3-byte header, no jump table
    sz, z, head = S.treeless_size(255, [801, 5, 5, 5])
    assert (sz, z) == (3 + 101, [101, 0, 0, 0])
    v = int.from_bytes(head[:3], "little")
    assert (v & 3, (v >> 2) & 3, (v >> 4) & 0x3FF, v >> 14) == (3, 0, 255, 101)
    # four streams above: jump table of 6 bytes, sizes of 10 / 14 / 18 bits
    sz, z, head = S.treeless_size(256, [7, 8, 9, 15])
    assert (sz, z) == (3 + 6 + 1 + 2 + 2 + 2, [1, 2, 2, 2])
    v = int.from_bytes(head[:3], "little")
    assert (v & 3, (v >> 2) & 3, (v >> 4) & 0x3FF, v >> 14) == (3, 1, 256, 13)
    sz, z, head = S.treeless_size(5000, [8000] * 4)
    v = int.from_bytes(head[:4], "little")
    assert sz == 4 + 6 + 4 * 1001 and (v & 3, (v >> 2) & 3, (v >> 4) & 0x3FFF, v >> 18) == (3, 2, 5000, 6 + 4004)
    sz, z, head = S.treeless_size(20000, [30000] * 4)
    v = int.from_bytes(head[:5], "little")
    assert sz == 5 + 6 + 4 * 3751 and (v & 3, (v >> 2) & 3, (v >> 4) & 0x3FFFF, v >> 22) == (3, 3, 20000, 6 + 15004)
    # what the format has no header for
    assert S.treeless_size(1000, [3000] * 4)[0] == 0           # 1506 bytes do not fit a 10-bit size
    assert S.treeless_size(200000, [65536 * 8] * 4)[0] == 0    # a stream of 64 KiB


def test_bound_is_the_plain_bound_plus_four_bytes_per_frame():
    import zeekstd_amd as zk
    for fs in (1, 1024, 1025, 2 * MIB, 1 << 31, (1 << 32) - 1):
        for n in sorted({0, 1, fs - 1, fs, fs + 1, (1 << 32) - 1, 1 << 32, 1 << 40}):
            frames = 1 if n == 0 else -(-n // fs)
            assert int(zk.lib.zk_compress_bound_dict(n, fs)) == int(zk.lib.zk_compress_bound(n, fs)) + 4 * frames, (n, fs)
    for n in (0, 1, 1 << 32):
        assert int(zk.lib.zk_compress_bound_dict(n, 0)) == 0


def test_entry_points_under_sanitizers(tmp_path, dicts):
    """the same entry points under AddressSanitizer + UBSan from a program of its own (tests/sim/enc_dict_san.cpp): the fixture's three
    dictionaries and a few generated ones"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dictsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(ROOT, "tests", "sim", "enc_dict_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    first = True
    for i, (name, d, m) in enumerate(dicts[:3] + dicts[3::5]):
        path = str(tmp_path / ("d%d" % i))
        with open(path, "wb") as f:
            f.write(d)
        r = subprocess.run([exe, path, str(i)], capture_output=True, text=True, timeout=300)
        if first and r.returncode != 0 and "AddressSanitizer" in r.stderr and "ERROR: AddressSanitizer:" not in r.stderr:
            pytest.skip("the sanitizer runtime cannot start here")
        first = False
        assert r.returncode == 0, (name, r.stdout[-300:], r.stderr[-3000:])

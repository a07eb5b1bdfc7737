"""Encoding against a zstd dictionary on the device (zk_cdict, zk_encode_frames_dict[_dev]; zeekstd_amd/csrc/zk_enc_dict.h has the rules,
tests/test_enc_dict_rules.py checks them on the CPU).  Every encoded frame goes to three judges -- libzstd 1.5.7 (ZSTD_decompress_usingDict), the
oracle (zko.frame_decode(dictionary=)) and the engine's own decoder with Engine.set_dictionary through zk_decode_frames_dev -- and the system's
libzstd must accept it too; what a frame says about itself is read back from its bytes (dict_fixtures.frame_facts).
No input here is meant to provoke a fault."""
import ctypes as C
import functools

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import dict_fixtures as df
from helpers import enc_dict_sim as S
from helpers import in_flight as IF
from helpers import libzstd_dict, zstd_gen
from helpers.dev_decode import dev as _dev, upload as _upload
from oracle import libzstd_ref
from oracle import zko

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
WINDOW = 57280                                               # ZKE_WINDOW: the matcher's ring
DICTS = S.fixture_dicts()
TRAINED_ID = 1368370104


@pytest.fixture(scope="module")
def judge():
    j = libzstd_dict.judge()
    if j is None:
        pytest.skip("libzstd 1.5.7 is not in this image")
    yield j
    j.close()


@pytest.fixture(scope="module")
def system_zstd():
    z = libzstd_ref.load("system")
    if z is None:
        pytest.skip("no system libzstd")
    z.ZSTD_decompress_usingDict.restype = C.c_size_t
    z.ZSTD_decompress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    z.ZSTD_createDCtx.restype = C.c_void_p
    dctx = C.c_void_p(z.ZSTD_createDCtx())

    def decode(frame, cap, dictionary):
        out = C.create_string_buffer(max(cap, 1))
        n = z.ZSTD_decompress_usingDict(dctx, out, cap, bytes(frame), len(frame), bytes(dictionary), len(dictionary))
        return None if z.ZSTD_isError(n) else out.raw[:n]
    return decode


@functools.lru_cache(maxsize=None)
def cdict_of(engine, key):
    """one EncodeDictionary per dictionary and session (made once, used by any number of calls)"""
    return zk.EncodeDictionary(engine, zk.Dictionary(_DICT_BYTES[key]))


_DICT_BYTES = dict(DICTS)


def cd(engine, d, key=None):
    key = key or ("anon%d" % (zko.xxh64(d) & 0xFFFFFFFF))
    _DICT_BYTES.setdefault(key, d)
    return cdict_of(engine, key)


def split(comp, pairs):
    out, at = [], 0
    for c, _ in pairs:
        out.append(comp[at:at + c]); at += c
    assert at == len(comp)
    return out


def three_judges(engine, judge, system_zstd, data, comp, pairs, dictionary, frame_size):
    """every frame decodes to its slice of the input under libzstd 1.5.7, the oracle, the system's libzstd and the engine's own decoder"""
    import torch
    frames = split(comp, pairs)
    at = 0
    for f, (c, d) in zip(frames, pairs):
        want = data[at:at + d]; at += d
        assert judge.using_dict(f, d + 64, dictionary) == want, ("libzstd 1.5.7", len(frames), c, d)
        assert zko.frame_decode(f, d + 64, True, dictionary=dictionary) == (want, len(f)), ("oracle", c, d)
        assert system_zstd(f, d + 64, dictionary) == want, ("system libzstd", c, d)
    assert at == len(data)
    c_off = np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).astype(np.uint64)
    d_off = np.concatenate([[0], np.cumsum([p[1] for p in pairs])]).astype(np.uint64)
    engine.set_dictionary(zk.Dictionary(dictionary))
    try:
        arch = _upload(comp, c_off, d_off)
        out = torch.full((len(data) + 64,), 0x5A, dtype=torch.uint8, device=_dev())
        st = torch.full((len(pairs),), -1, dtype=torch.int32, device=_dev())
        rc = engine.decode_frames_dev(arch[0], arch[1], arch[2], arch[3], 0, len(pairs), out, len(data), True, st)
        torch.cuda.synchronize()
        assert rc == 0 and not st.cpu().numpy().any()
        assert out[:len(data)].cpu().numpy().tobytes() == data
    finally:
        engine.set_dictionary(None)
    return frames


def facts_of(frames):
    return [df.frame_facts(f) for f in frames]


def assert_block_rules(facts):
    """no block after a frame's first is Treeless; no table goes back to the dictionary's (Repeat_Mode before any definition is the
    dictionary's, so: a table in FSE_Compressed_Mode is never followed, in the same frame, by a state the dictionary's table would need --
    which here means every table's mode sequence is either Predefined throughout, Repeat throughout, or Compressed once and Repeat after)"""
    for ff in facts:
        per_table = [[], [], []]
        for i, (bt, lt, modes) in enumerate(ff["blocks"]):
            if bt == 2:
                assert not (i and lt == 3), ff["blocks"]
                if modes:
                    for t in range(3): per_table[t].append(modes[t])
        for seq in per_table:
            if not seq: continue
            assert 1 not in seq                                          # (RLE_Mode is never written)
            if seq[0] == 0: assert set(seq) == {0}, seq
            elif seq[0] == 3: assert set(seq) == {3}, seq            # the dictionary's table, every block
            else: assert seq[0] == 2 and set(seq[1:]) <= {3}, seq    # the frame's own, defined once


def dict_tables_used(ff):
    """a frame says Repeat_Mode for a table before any block defined one"""
    for bt, lt, modes in ff["blocks"]:
        if bt == 2 and modes:
            return 3 in modes
    return False


# ---------------------------------------------------------------------------------------------- raw-content dictionary
@pytest.mark.parametrize("level", [1, 2, 3, 9])
@pytest.mark.parametrize("checksum", [False, True])
def test_raw_content_dictionary_is_the_prefix_route(engine, judge, system_zstd, level, checksum):
    raw = DICTS["raw"]
    data = df.records(41, 30000)
    fs = 7000
    comp, pairs = engine.encode_frames(data, fs, level, checksum, dictionary=cd(engine, raw, "raw"))
    comp_p, pairs_p = engine.encode_frames(data, fs, level, checksum, prefix=raw)
    assert (comp, pairs) == (comp_p, pairs_p)
    twin = b"".join(zko.frame_encode(data[o:o + fs], level, checksum, prefix=raw) for o in range(0, len(data), fs))
    assert comp == twin
    frames = three_judges(engine, judge, system_zstd, data, comp, pairs, raw, fs)
    for ff in facts_of(frames):
        assert ff["dict_id"] is None and ff["checksum"] == checksum
    assert cd(engine, raw, "raw").id == 0


# ---------------------------------------------------------------------------------------------- trained dictionary
@pytest.mark.parametrize("fs", [0, 1, 255, 256, 1024, 4096, 4097, 40000])
def test_trained_dictionary(engine, judge, system_zstd, fs):
    d = DICTS["trained"]
    nf = 1 if fs == 0 else 3 if fs >= 40000 else 12
    data = df.records(9000 + fs, nf * fs - (fs // 3 if fs > 2 else 0)) if fs else b""
    frame_size = fs or 1024
    c = cd(engine, d, "trained")
    assert c.id == TRAINED_ID
    comp, pairs = engine.encode_frames(data, frame_size, 1, True, dictionary=c)
    assert [p[1] for p in pairs] == ([len(data[o:o + frame_size]) for o in range(0, len(data), frame_size)] or [0])
    frames = three_judges(engine, judge, system_zstd, data, comp, pairs, d, frame_size)
    facts = facts_of(frames)
    for ff in facts:
        assert ff["dict_id"] == TRAINED_ID and ff["checksum"]
    assert_block_rules(facts)
    if fs == 0:
        assert len(frames) == 1 and len(frames[0]) == 9 + 4 + 4          # the empty frame carries the 4-byte field (and its checksum)
    if fs in (256, 1024, 4096):
        # the reference shows it is reachable: the fixture's libzstd-made frames on this generator are (2, 3, (3, 3, 3))
        assert any(ff["blocks"][0][:2] == (2, 3) for ff in facts), [ff["blocks"][0] for ff in facts]
        assert any(dict_tables_used(ff) for ff in facts), [ff["blocks"][0] for ff in facts]
    if fs == 4097:
        assert all(len(ff["blocks"]) == 2 for ff in facts[:-1])
    if fs == 40000:
        assert all(len(ff["blocks"]) >= 3 for ff in facts[:-1])
    # the same bytes from HBM to HBM
    assert dev_encode(engine, data, frame_size, 1, True, c).payload() == comp


def test_patched_dictionary_decodes_the_same(engine, judge, system_zstd):
    """repeat offsets 24 / 57 / 131: the encoder emits no repeat code before a sequence of the same block, so they are irrelevant"""
    data = df.records(77, 20000)
    comp, pairs = engine.encode_frames(data, 1024, 1, False, dictionary=cd(engine, DICTS["patched"], "patched"))
    comp_t, pairs_t = engine.encode_frames(data, 1024, 1, False, dictionary=cd(engine, DICTS["trained"], "trained"))
    assert comp == comp_t and pairs == pairs_t
    three_judges(engine, judge, system_zstd, data, comp, pairs, DICTS["patched"], 1024)


# ---------------------------------------------------------------------------------------------- generated dictionaries: fallbacks
def _generated(**kw):
    d, m = zstd_gen.make_dictionary(**kw)
    return d, m, S.build(d)


def test_tree_without_a_literal_falls_back(engine, judge, system_zstd):
    """a tree of two symbols: the first block's literals are not all in it, so no frame is Treeless; all decode"""
    d, m, b = _generated(seed=36, alphabet=2, weights="direct", content_size=3000)
    data = df.records(5, 6000)
    assert any(not b["len"][x] for x in data[:1024])
    comp, pairs = engine.encode_frames(data, 1024, 1, True, dictionary=cd(engine, d))
    frames = three_judges(engine, judge, system_zstd, data, comp, pairs, d, 1024)
    for ff in facts_of(frames):
        assert all(lt != 3 for bt, lt, modes in ff["blocks"]) and ff["dict_id"] == (m.id or None)


def test_tables_without_a_needed_code_fall_back(engine, judge, system_zstd):
    """sparse tables (accuracy logs of 5: at most 31 codes each; seeds whose tables lack codes): a table that lacks a code the frame uses is
    not taken -- read back: every Repeat_Mode-first table has a cost for every code, which the three judges confirm by decoding"""
    data = df.records(6, 12000) + bytes(3000) + df.records(7, 3000)
    seen_repeat = seen_fallback = 0
    for kw in (dict(seed=39, als={"of": 5, "ll": 5, "ml": 5}), dict(seed=3), dict(seed=11), dict(seed=42, wide=True, content_size=2000)):
        d, m, b = _generated(**kw)
        comp, pairs = engine.encode_frames(data, 3000, 1, False, dictionary=cd(engine, d))
        frames = three_judges(engine, judge, system_zstd, data, comp, pairs, d, 3000)
        facts = facts_of(frames)
        assert_block_rules(facts)
        for ff in facts:
            first = next((modes for bt, lt, modes in ff["blocks"] if bt == 2 and modes), None)
            if first:
                seen_repeat += 3 in first
                seen_fallback += any(x != 3 for x in first)
    assert seen_fallback >= 1


def test_noise_and_runs(engine, judge, system_zstd):
    d = DICTS["trained"]
    c = cd(engine, d, "trained")
    for data, fs, want_type in ((df.noise(9, 5000), 1024, 0), (b"\x07" * 5000, 1024, 1), (b"Q", 1024, None)):
        comp, pairs = engine.encode_frames(data, fs, 1, True, dictionary=c)
        frames = three_judges(engine, judge, system_zstd, data, comp, pairs, d, fs)
        for ff in facts_of(frames):
            assert ff["dict_id"] == TRAINED_ID
            if want_type is not None:
                assert all(bt == want_type for bt, lt, modes in ff["blocks"]), ff["blocks"]


# ---------------------------------------------------------------------------------------------- content boundaries
def _wrap(content, seed=50, dict_id=4242):
    """a formatted dictionary around `content`: a generated dictionary's header (wide tables) in front of it"""
    d, m = zstd_gen.make_dictionary(seed=seed, dict_id=dict_id, wide=True, content_size=8, reps=(1, 1, 1))
    return d[:m.content_offset] + content


@pytest.mark.parametrize("level", [1, 3])
def test_content_longer_than_the_ring(engine, judge, system_zstd, level):
    """more than 57 280 bytes of records as content: the long-distance table over the content runs; frames repeat records from its far end"""
    content = df.records(60, 90000)
    assert len(content) > WINDOW
    d = _wrap(content)
    data = content[1000:9000] + df.records(61, 4000) + content[200:3000]
    comp, pairs = engine.encode_frames(data, 5000, level, True, dictionary=cd(engine, d))
    comp_p, pairs_p = engine.encode_frames(data, 5000, level, True, prefix=content)
    frames = three_judges(engine, judge, system_zstd, data, comp, pairs, d, 5000)
    assert all(ff["dict_id"] == 4242 for ff in facts_of(frames))
    # the matcher is the prefix route's: the same long-distance matches (the tables differ -- recorded, not gated: they are nobody's training)
    assert len(pairs) == len(pairs_p)
    print("level %d: dictionary route %d bytes, prefix route %d + %d ID bytes, input %d" % (level, len(comp), len(comp_p), 2 * len(pairs), len(data)))
    assert len(comp_p) < len(data) // 2                                  # the far end of the content was reached (by both: one matcher)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_content_of_a_few_bytes(engine, judge, system_zstd, n):
    d = _wrap(b"{\"i"[:n], seed=51, dict_id=77)
    data = df.records(62, 5000)
    comp, pairs = engine.encode_frames(data, 1500, 1, True, dictionary=cd(engine, d))
    frames = three_judges(engine, judge, system_zstd, data, comp, pairs, d, 1500)
    assert all(ff["dict_id"] == 77 for ff in facts_of(frames))


# ---------------------------------------------------------------------------------------------- ratio
LIBZSTD_DICT_RATIO = {256: 3.073, 512: 3.626, 1024: 3.944}           # libzstd 1.5.7, level 1, the trained dictionary (measured on the CPU)


@pytest.mark.parametrize("fs", [256, 512, 1024])
def test_ratio_beats_the_prefix_route(engine, fs):
    d = DICTS["trained"]
    content = d[135:]
    data = df.records(9000 + fs, 32 << 10)
    nf = -(-len(data) // fs)
    for level in (1, 3):
        comp, pairs = engine.encode_frames(data, fs, level, False, dictionary=cd(engine, d, "trained"))
        comp_p, _ = engine.encode_frames(data, fs, level, False, prefix=content)
        comp_n, _ = engine.encode_frames(data, fs, level, False)
        print("fs %d level %d: dictionary %d prefix %d (+ %d ID bytes) plain %d input %d: ratio %.3f / %.3f / %.3f, libzstd 1.5.7 with the dictionary %.3f"
              % (fs, level, len(comp), len(comp_p), 4 * nf, len(comp_n), len(data), len(data) / len(comp), len(data) / len(comp_p),
                 len(data) / len(comp_n), LIBZSTD_DICT_RATIO[fs]))
        assert len(comp) < len(comp_p) + 4 * nf, (fs, level, len(comp), len(comp_p), nf)


# ---------------------------------------------------------------------------------------------- slices
def test_bytes_do_not_depend_on_the_staging_slices(engine):
    d = DICTS["trained"]
    c = cd(engine, d, "trained")
    data = df.records(90, 40 * 1024)
    rec = ((len(d) - 135) & ~3) + 1024                                  # one [content tail | frame] record: the tail is a multiple of 4
    want = None
    try:
        for slices in (1, 2, 7):
            per = -(-40 // slices)
            kib = -(-per * rec // 1024)
            assert -(-40 // ((kib * 1024) // rec)) == slices
            engine.set_kernel_choice(enc_dict_slice_kib=kib)
            got = (engine.encode_frames(data, 1024, 1, True, dictionary=c), engine.encode_frames(data, 1024, 3, True, dictionary=c))
            want = want or got
            assert got == want, slices
        engine.set_kernel_choice(enc_dict_slice_kib=1)                  # less than one record: a frame at a time
        assert (engine.encode_frames(data, 1024, 1, True, dictionary=c), engine.encode_frames(data, 1024, 3, True, dictionary=c)) == want
    finally:
        engine.set_kernel_choice(reset=0)


# ---------------------------------------------------------------------------------------------- destinations
class Encoded:
    def payload(self):
        return self.all[self.lead:self.lead + self.written].tobytes()


def dev_encode(engine, data, frame_size, level, checksum, cdict, cap=None, lead=5):
    """one zk_encode_frames_dict_dev call into a poisoned tensor (tests/test_gpu_encode_bound.py's pattern)"""
    import torch
    n = len(data)
    nf = max(1, -(-n // frame_size))
    cap = int(zk.lib.zk_compress_bound_dict(n, frame_size)) if cap is None else cap
    buf = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    src = torch.zeros(n + 64, dtype=torch.uint8, device=_dev())
    if n:
        src[:n] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(_dev())
    d_cs = torch.zeros(nf, dtype=torch.int32, device=_dev())
    d_ds = torch.zeros(nf, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    r = Encoded()
    r.rc, r.nf, r.written, r.lead, r.cap = 0, 0, 0, lead, cap
    try:
        r.nf, r.written = engine.encode_frames_dict_dev(src.data_ptr(), n, frame_size, level, checksum, cdict, buf.data_ptr() + lead, cap, d_cs, d_ds)
    except zk.ZkError as ex:
        r.rc = ex.code
    torch.cuda.synchronize()
    r.all = buf.cpu().numpy()
    r.c_sizes = d_cs.cpu().numpy().astype(np.int64)
    assert bytes(src[:n].cpu().numpy()) == data, "the source is the caller's: untouched"
    return r


def test_destinations_at_the_bound_at_the_size_and_one_below(engine):
    d = DICTS["trained"]
    c = cd(engine, d, "trained")
    for data, fs in ((df.records(95, 20000), 1024), (df.noise(96, 3000), 700), (b"", 512)):
        want, pairs = engine.encode_frames(data, fs, 1, True, dictionary=c)
        r = dev_encode(engine, data, fs, 1, True, c)
        assert r.rc == 0 and r.payload() == want and r.written <= r.cap and int(r.c_sizes.sum()) == r.written
        outside = np.concatenate([r.all[:r.lead], r.all[r.lead + r.written:]])
        assert (outside == POISON).all()
        r = dev_encode(engine, data, fs, 1, True, c, cap=len(want))
        assert r.rc == 0 and r.payload() == want
        assert (np.concatenate([r.all[:r.lead], r.all[r.lead + r.written:]]) == POISON).all()
        r = dev_encode(engine, data, fs, 1, True, c, cap=len(want) - 1)
        assert r.rc == -70 and (r.all == POISON).all()
        # the engine is whole after the refusal
        assert engine.encode_frames(data, fs, 1, True, dictionary=c) == (want, pairs)
    # noise at the bound: raw blocks plus the largest field is what the four bytes per frame are for
    data = df.noise(97, 2048)
    r = dev_encode(engine, data, 1, 1, True, c)
    assert r.rc == 0 and r.written <= r.cap


def test_arguments(engine):
    import torch
    src = torch.zeros(128, dtype=torch.uint8, device=_dev())
    dst = torch.full((4096,), POISON, dtype=torch.uint8, device=_dev())
    with pytest.raises(zk.ZkError) as ex:
        engine.encode_frames_dict_dev(src.data_ptr(), 64, 32, 1, False, None, dst.data_ptr(), 4096)
    assert ex.value.code == -2003
    assert (dst.cpu().numpy() == POISON).all()


# ---------------------------------------------------------------------------------------------- two dictionaries
def test_two_dictionaries_alternately(engine, judge):
    da = DICTS["trained"]
    db, mb = zstd_gen.make_dictionary(seed=42, wide=True, content_size=4000, dict_id=99)
    ca, cb = cd(engine, da, "trained"), cd(engine, db)
    assert (ca.id, cb.id) == (TRAINED_ID, 99)
    data = df.records(98, 6000)
    for i in range(4):
        mine, other, c = (da, db, ca) if i % 2 == 0 else (db, da, cb)
        comp, pairs = engine.encode_frames(data, 1500, 1, True, dictionary=c)
        at = 0
        for f, (cs, ds) in zip(split(comp, pairs), pairs):
            assert judge.using_dict(f, ds + 64, mine) == data[at:at + ds]
            assert judge.using_dict(f, ds + 64, other) == -32
            at += ds
    # the routes without a dictionary are what they were, whatever objects exist
    assert engine.encode_frames(data, 1500, 1, True)[0] == b"".join(zko.frame_encode(data[o:o + 1500], 1, True) for o in range(0, 6000, 1500))


# ---------------------------------------------------------------------------------------------- in flight
@pytest.mark.parametrize("state", IF.STATES)
def test_served_while_batches_are_in_flight(engine, state):
    """the table above zk_decode_submit_dev: zk_cdict_create / _free / _id, zk_encode_frames_dict[_dev] and the two setters of the handles are
    served in all three busy states"""
    import io
    from zeekstd_amd import EncodeOptions, FrameSizePolicy
    d = DICTS["trained"]
    data = df.records(99, 9000)
    want = engine.encode_frames(data, 1024, 1, True, dictionary=cd(engine, d, "trained"))
    big = IF.engine_made(engine, 20, 640 << 10, 0x6400, repeat=8)
    with IF.Flight(engine) as fl:
        fl.reach(state, big)
        c = zk.EncodeDictionary(engine, zk.Dictionary(d))
        assert c.id == TRAINED_ID
        assert engine.encode_frames(data, 1024, 1, True, dictionary=c) == want
        r = dev_encode(engine, data, 1024, 1, True, c)
        assert r.rc == 0 and r.payload() == want[0]
        raw = EncodeOptions().engine(engine).frame_size_policy(FrameSizePolicy.Uncompressed(1024)).compression_level(1).checksum_flag(True).into_raw_encoder()
        raw.set_dictionary(c)
        buf = bytearray(4096)
        assert raw.compress(data[:1024], buf).in_progress() == 1024
        p = raw.end_frame(buf)
        assert p.data_left() == 0 and bytes(buf[:p.out_progress()]) == want[0][:want[1][0][0]]
        sink = io.BytesIO()
        enc = EncodeOptions().engine(engine).frame_size_policy(FrameSizePolicy.Uncompressed(1024)).compression_level(1).checksum_flag(True).into_encoder(sink)
        enc.set_dictionary(c)
        enc.compress(data); enc.end_frame(); enc.flush()
        assert sink.getvalue() == want[0]
        del raw, enc
        c.close()
        assert set(fl.live) == IF.BUSY[state]
        fl.wait_all()

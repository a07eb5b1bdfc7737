"""zk_train_dictionary[_dev] on the GPU (include/zeekstd_amd.h; zeekstd_amd/csrc/zk_train.hip, zk_train.h): the content against the numpy model
of the rule (tests/helpers/train_model.py), the choice between segment lengths and the report against independent encodes of the samples, the
trained dictionary at work on frames it has not seen, the refused calls, and training while decode batches are in flight.  The reference has
no trainer; the fixture's dictionary (libzstd 1.5.7, ZDICT_trainFromBuffer over the same samples) is what the result is measured against.

test_held_out_frames measures the result against the fixture's dictionary through the same engine call; the figures are in MEASURED below and
in profiles/dict_train_probe.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import dict_fixtures as df
from helpers import enc_dict_sim as S
from helpers import in_flight as IF
from helpers import libzstd_dict
from helpers import train_model as M
from helpers.dev_decode import dev as _dev, upload as _upload
from oracle import zko
from conftest import GOLDENS

pytestmark = pytest.mark.gpu

CAP = 16384
ARG = -2003
# test_held_out_frames, bytes of the 120 frames at level 1 through Engine.encode_frame_list: no dictionary / the fixture's content as a raw
# dictionary / the fixture's formatted dictionary (the reference) / the trained content alone / the trained dictionary.  MARGIN: the measured
# excess of the last over the reference, rounded up to the next whole percent; the output is deterministic, so it only guards later changes.
MEASURED = {"none": 43077, "fixture_raw": 25894, "fixture": 20254, "trained_raw": 25786, "trained": 19728}
MARGIN_PERCENT = -2          # measured: -2.60 % (the trained dictionary is the smaller)


@functools.lru_cache(maxsize=None)
def samples():
    s = M.fixture_samples()
    return s, M.join(s)


@functools.lru_cache(maxsize=None)
def model_content(k):
    s, (data, off) = samples()
    hp = M.hashes(data, off, 8, 20)
    return M.select(data, hp, M.count(hp, 20), k, 8, M.content_cap(CAP))


def encoded_total(engine, sample_list, dictionary=None, level=1):
    data, off = M.join(sample_list)
    cd = zk.EncodeDictionary(engine, zk.Dictionary(dictionary)) if dictionary else None
    try:
        comp, pairs = engine.encode_frame_list(data, off, level, False, dictionary=cd)
    finally:
        if cd is not None:
            cd.close()
    assert len(comp) == sum(p[0] for p in pairs)
    return len(comp), comp, pairs


def on_device(sample_list, lead=0):
    import torch
    data, off = M.join(sample_list)
    buf = np.concatenate([np.full(lead, 0xEE, np.uint8), data])
    return (torch.from_numpy(buf.copy()).to(_dev()) if buf.size else torch.zeros(1, dtype=torch.uint8, device=_dev()),
            torch.from_numpy((off + np.uint64(lead)).view(np.int64).copy()).to(_dev()), len(sample_list))


def test_pinned_k_equals_the_model_and_itself(engine):
    """k = 256 at 16 KiB over the fixture's samples: the content is the model's, byte for byte; a second call and the device entry point (its
    list starting at 37) give the same bytes; the report's fields agree with the model and with independent encodes of the samples"""
    s, (data, off) = samples()
    segs, want = model_content(256)
    got, rep = engine.train_dictionary(data, off, CAP, k=256, raw_content=True, report=True)
    assert got == want and len(got) == M.content_cap(CAP) == 62 * 256
    assert engine.train_dictionary(s, None, CAP, k=256, raw_content=True) == got
    d_buf, d_off, count = on_device(s, lead=37)
    got_dev, rep_dev = engine.train_dictionary_dev(d_buf, d_off, count, CAP, k=256, raw_content=True, report=True)
    assert got_dev == got and rep_dev == rep
    with_, _, _ = encoded_total(engine, s, got)
    without, _, _ = encoded_total(engine, s)
    assert rep == {"k_chosen": 256, "segments": len(segs), "content_bytes": len(got), "header_bytes": 0, "sample_bytes": len(data),
                   "compressed_with": with_, "compressed_without": without}
    assert with_ < without
    assert zk.Dictionary(got).id == 0 and zk.Dictionary.train(engine, s, None, CAP, k=256, raw_content=True).content_offset == 0
    # the formatted result: the same content behind a header, the same report but for the header's bytes; identical across calls and entry points
    full, frep = engine.train_dictionary(data, off, CAP, k=256, report=True)
    h = zk.Dictionary(full)
    assert 20 < h.content_offset <= 512 and full[h.content_offset:] == got and len(full) <= CAP
    assert frep == dict(rep, header_bytes=h.content_offset)
    assert h.id == 32768 + zko.xxh64(got) % ((1 << 31) - 65536)
    assert engine.train_dictionary(s, None, CAP, k=256) == full
    assert engine.train_dictionary_dev(d_buf, d_off, count, CAP, k=256, report=True) == (full, frep)
    # a caller's ID: in the bytes, and in the frames encoded with the dictionary
    mine = engine.train_dictionary(s, None, CAP, k=256, dict_id=0x12345)
    assert mine == full[:4] + (0x12345).to_bytes(4, "little") + full[8:] and zk.Dictionary(mine).id == 0x12345
    _, comp, pairs = encoded_total(engine, s[:5], mine)
    assert df.frame_facts(comp[:pairs[0][0]])["dict_id"] == 0x12345


def test_k_zero_keeps_the_candidate_that_encodes_the_samples_smallest(engine):
    s, _ = samples()
    got, rep = engine.train_dictionary(s, None, CAP, raw_content=True, report=True)
    ks = M.candidates(CAP)
    assert ks == [64, 128, 256, 512]
    totals = [encoded_total(engine, s, model_content(k)[1])[0] for k in ks]
    best = min(range(4), key=lambda i: (totals[i], ks[i]))
    assert rep["k_chosen"] == ks[best] and rep["compressed_with"] == totals[best] and got == model_content(ks[best])[1], (totals, rep)
    assert len(set(totals)) > 1


def test_samples_above_the_trial_limit_are_tried_on_every_jth(engine):
    """ZK_CHOICE_TRAIN_TRIAL_KIB = 64 puts the 64 MiB rule under the fixture's 1.7 MB: the content is still selected from all samples, the
    candidates are judged and the report's totals counted on samples 0, j, 2 j, ... for the smallest j that totals at most 64 KiB, and the
    tables are those samples' -- the header differs from the one all samples give, the content does not unless k does"""
    s, (data, off) = samples()
    sizes = [len(x) for x in s]
    j = M.trial_stride(sizes, 64 << 10)
    assert j > 2 and sum(sizes[::j]) <= 64 << 10 < sum(sizes[::j - 1])
    tried = s[::j]
    ks = M.candidates(CAP)
    totals = [encoded_total(engine, tried, model_content(k)[1])[0] for k in ks]
    best = min(range(4), key=lambda i: (totals[i], ks[i]))
    whole = engine.train_dictionary(s, None, CAP, k=ks[best])
    d_buf, d_off, count = on_device(s, lead=5)
    try:
        engine.set_kernel_choice(train_trial_kib=64)
        got, rep = engine.train_dictionary(s, None, CAP, report=True)
        assert engine.train_dictionary_dev(d_buf, d_off, count, CAP, report=True) == (got, rep)
        raw = engine.train_dictionary(s, None, CAP, raw_content=True)
    finally:
        engine.set_kernel_choice(reset=0)
    h = zk.Dictionary(got)
    assert rep["k_chosen"] == ks[best] and rep["compressed_with"] == totals[best] and rep["compressed_without"] == encoded_total(engine, tried)[0]
    assert rep["sample_bytes"] == len(data) and got[h.content_offset:] == raw == model_content(ks[best])[1]
    assert whole[zk.Dictionary(whole).content_offset:] == raw and whole[8:zk.Dictionary(whole).content_offset] != got[8:h.content_offset]
    assert engine.train_dictionary(s, None, CAP, k=ks[best]) == whole              # the key is back at its default
    judge = libzstd_dict.judge()
    if judge is not None:
        assert judge.load_dictionary(got) == 0
        judge.close()


def test_held_out_frames(engine):
    """120 frames the trainer has not seen, through Engine.encode_frame_list(dictionary=) at level 1"""
    s, _ = samples()
    trained = engine.train_dictionary(s, None, CAP)
    trained_raw = engine.train_dictionary(s, None, CAP, raw_content=True)
    assert trained[zk.Dictionary(trained).content_offset:] == trained_raw
    held = M.held_out()
    assert len(held) == 120 and sum(map(len, held)) == 71680
    fixture = S.fixture_dicts()["trained"]
    fixture_raw = fixture[zk.Dictionary(fixture).content_offset:]
    total, comp, pairs = encoded_total(engine, held, trained)
    got = {"none": encoded_total(engine, held)[0], "fixture_raw": encoded_total(engine, held, fixture_raw)[0],
           "fixture": encoded_total(engine, held, fixture)[0], "trained_raw": encoded_total(engine, held, trained_raw)[0], "trained": total}
    print("\nheld-out totals:", got, "excess over the reference: %.2f %%" % (100.0 * (total - got["fixture"]) / got["fixture"]))
    # the frames decode to their input: the engine with the dictionary set, the oracle, libzstd 1.5.7 where it is here
    import torch
    data, off = M.join(held)
    c_off = np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).astype(np.uint64)
    engine.set_dictionary(zk.Dictionary(trained))
    try:
        arch = _upload(comp, c_off, off)
        out = torch.full((len(data) + 64,), 0x5A, dtype=torch.uint8, device=_dev())
        st = torch.full((len(pairs),), -1, dtype=torch.int32, device=_dev())
        rc = engine.decode_frames_dev(arch[0], arch[1], arch[2], arch[3], 0, len(pairs), out, len(data), True, st)
        torch.cuda.synchronize()
        assert rc == 0 and not st.cpu().numpy().any() and out[:len(data)].cpu().numpy().tobytes() == data.tobytes()
    finally:
        engine.set_dictionary(None)
    judge = libzstd_dict.judge()
    for i, (c, d) in enumerate(pairs):
        f = comp[int(c_off[i]):int(c_off[i + 1])]
        assert zko.frame_decode(f, d + 64, True, dictionary=trained) == (held[i], len(f)), i
        if judge is not None:
            assert judge.using_dict(f, d + 64, trained) == held[i], i
    if judge is not None:
        assert judge.load_dictionary(trained) == 0
        judge.close()
    assert got["trained"] < got["trained_raw"] < got["none"]
    assert got == MEASURED, got
    assert 100 * (got["trained"] - got["fixture"]) <= MARGIN_PERCENT * got["fixture"]


def _refused(engine, sample_list, cap=CAP, offsets=None, **kw):
    """the host call and the device call: ZK_ERR_ARGUMENT from both, the destination, `written` and the report as they were"""
    data, off = M.join(sample_list)
    if offsets is not None:
        off = np.asarray(offsets, np.uint64)
    par = zk.TrainParams(kw.get("k", 0), kw.get("d", 0), kw.get("f", 0), 0, 0, kw.get("flags", 1))
    import torch
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)])).to(_dev())
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(_dev())
    torch.cuda.synchronize()
    for host in (True, False):
        out = np.full(max(cap, 1) + 64, 0xA5, np.uint8)
        wr, rep = C.c_size_t(0xABCD), zk.TrainReport(7, 7, 7, 7, 7, 7, 7)
        if host:
            rc = zk.lib.zk_train_dictionary(engine._h, data.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(par), out.ctypes.data, cap, C.byref(wr), C.byref(rep))
        else:
            rc = zk.lib.zk_train_dictionary_dev(engine._h, d_data.data_ptr(), d_off.data_ptr(), len(off) - 1, C.byref(par), out.ctypes.data, cap, C.byref(wr),
                                                C.byref(rep), None)
        assert rc == ARG, (host, rc, kw)
        assert (out == 0xA5).all() and wr.value == 0xABCD and rep.k_chosen == 7 and rep.compressed_without == 7, (host, kw)


def test_refused_calls_write_nothing(engine):
    good = [df.records(300 + i, 200) for i in range(12)]
    _refused(engine, [], offsets=[0])                                       # count == 0
    _refused(engine, good, cap=1023)
    _refused(engine, good, offsets=[0, 200, 150] + [200 * i for i in range(2, 12)])     # a decreasing list
    for kw in ({"d": 7}, {"d": 4}, {"f": 9}, {"f": 25}, {"k": 15}, {"k": 4097}, {"k": 512, "cap": 2047}, {"flags": 2}, {"flags": 3}):
        kw = dict(kw)
        _refused(engine, good, cap=kw.pop("cap", CAP), **kw)
    _refused(engine, [df.records(i, 8) for i in range(7)] + [b"1234567"] * 5)           # seven samples of d bytes
    _refused(engine, [df.records(i, 8) for i in range(8)], d=0, offsets=[0] + [8 * i + 7 for i in range(8)])      # ... the first of only 7
    # a sample above a frame's largest size (2^30): decided from the offsets, before anything runs
    _refused(engine, good, offsets=[0] + [200 * i for i in range(1, 12)] + [2200 + (1 << 30) + 1])
    # more samples than a call has frames: another code, decided before the list is read (the arrays here hold 13 offsets)
    data, off = M.join(good)
    out, wr = np.full(CAP, 0xA5, np.uint8), C.c_size_t(0xABCD)
    par = zk.TrainParams(0, 0, 0, 0, 0, 0)
    assert zk.lib.zk_train_dictionary(engine._h, data.ctypes.data, off.ctypes.data, 0x08000001, C.byref(par), out.ctypes.data, CAP, C.byref(wr), None) == -1002
    assert (out == 0xA5).all() and wr.value == 0xABCD
    # 2^32 bytes in all: decided from the offsets, nothing is read
    _refused(engine, good, offsets=[0] + [200 * i for i in range(1, 12)] + [1 << 32])


def test_edges(engine):
    """noise; eight samples of exactly d bytes (with k above their 64 bytes no segment fits: the samples' tail); empty samples and a list that starts above 0; d = 6 and a
    small table: every result is the model's and a dictionary zk_dict_create takes"""
    noise = [df.noise(500 + i, 300) for i in range(40)]
    got = engine.train_dictionary(noise, None, 2048, k=64, raw_content=True)
    assert got == M.train(noise, 2048, 64)[1] and len(got) == 1536 and zk.Dictionary(got).id == 0
    full = engine.train_dictionary(noise, None, 2048, k=64)
    assert full[zk.Dictionary(full).content_offset:] == got
    judge = libzstd_dict.judge()
    if judge is not None:
        assert judge.load_dictionary(got) == 0 and judge.load_dictionary(full) == 0
        judge.close()
    tiny = [bytes([65 + i]) * 8 for i in range(8)]
    assert M.train(tiny, 1024, 64) == ([0], b"".join(tiny)) and M.train(tiny, 1024, 128) == ([], b"".join(tiny))
    got, rep = engine.train_dictionary(tiny, None, 1024, raw_content=True, report=True)            # k = 64 takes the one segment there is
    assert got == b"".join(tiny) and rep["segments"] == 1 and rep["k_chosen"] == 64 and rep["content_bytes"] == 64
    got, rep = engine.train_dictionary(tiny, None, 1024, k=128, raw_content=True, report=True)     # no segment of 128 bytes: the samples' tail
    assert got == b"".join(tiny) and rep["segments"] == 0 and rep["k_chosen"] == 128 and rep["content_bytes"] == 64
    full = engine.train_dictionary(tiny, None, 1024)
    assert full[zk.Dictionary(full).content_offset:] == got
    case = M.cases()["short_samples_d6"]
    buf, off = case.buffers()
    want = M.train(case.samples, 1536, 32, d=6, f=10)[1]
    assert engine.train_dictionary(np.frombuffer(buf, np.uint8), off, 1536, k=32, d=6, f=10, raw_content=True) == want
    d_buf, d_off, count = on_device(case.samples, lead=case.lead)
    assert engine.train_dictionary_dev(d_buf, d_off, count, 1536, k=32, d=6, f=10, raw_content=True) == want


@pytest.mark.parametrize("state", IF.STATES)
def test_training_while_batches_are_in_flight(engine, state):
    """served in all three states with the bytes it has when idle; the batches' results are what they are without it (Flight checks them
    bit for bit); an encode and a decode of a golden archive before and after are identical"""
    s = [df.records(700 + i, 300 + 7 * i) for i in range(64)]
    g = next(x for x in GOLDENS if x.name == "text_l1_64k")
    c, d = g.offsets()

    def around():
        enc = engine.encode_frames(g.input()[:200000], 65536, 1, True)
        out, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, verify=True)
        assert not st.any()
        return enc, out
    before = around()
    idle = engine.train_dictionary(s, None, 4096, report=True)
    d_buf, d_off, count = on_device(s)
    with IF.Flight(engine) as fl:
        fl.reach(state, IF.Staged(IF.long_()), IF.Staged(IF.long_()))
        assert engine.train_dictionary(s, None, 4096, report=True) == idle
        assert engine.train_dictionary_dev(d_buf, d_off, count, 4096, report=True) == idle
        assert set(fl.live) == IF.BUSY[state]
        fl.wait_all()
    assert around() == before

"""Frames of caller-given sizes in one call (zk_encode_frame_list[_dev]).  The contract that makes it checkable: frame i is byte for byte the
frame the existing route makes of those bytes alone -- on the plain and prefix routes the twin's zko.frame_encode, on the dictionary route the
single-frame zk_encode_frames_dict_dev call.  The list is tests/helpers/enc_list_inputs.py's: sizes at the encoder's own edges, shuffled.
No input here is meant to provoke a fault."""
import functools

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import dict_fixtures as df
from helpers import enc_dict_sim as S
from helpers import enc_list_inputs as E
from helpers import in_flight as IF
from helpers import libzstd_dict
from helpers.dev_decode import dev as _dev, upload as _upload
from oracle import zko

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
DICTS = S.fixture_dicts()
LEVELS = [1, 2, 3, 9]
ERR_ARGUMENT, ERR_FRAME_INDEX = -2003, -1002


def sizes_of(off):
    return [int(off[i + 1] - off[i]) for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def twin(level, checksum, prefix_key=None):
    data, off = E.edge_list()
    return tuple(zko.frame_encode(f, level, checksum, prefix=PREFIXES[prefix_key] if prefix_key else None) for f in E.frames_of(data, off))


PREFIXES = {3: b"abc", 1000: zko.gen_text(1000, 31), 200000: zko.gen_text(200000, 9)}


class Encoded:
    def payload(self):
        return self.all[self.lead:self.lead + self.written].tobytes()

    def frames(self):
        out, at = [], self.lead
        for c in self.c_sizes:
            out.append(self.all[at:at + int(c)].tobytes()); at += int(c)
        return out


def dev_encode(engine, data, off, level, checksum, prefix=None, cdict=None, cap=None, lead=5):
    """one zk_encode_frame_list_dev call into a poisoned tensor; data[off[0]:off[-1]] is what the frames cover"""
    import torch
    count = len(off) - 1
    n = int(off[count] - off[0]) if count else 0
    cap = int(zk.lib.zk_compress_bound_list(n, count, int(cdict is not None))) if cap is None else cap
    buf = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=_dev())
    if len(data):
        src[:len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(_dev())
    d_off = torch.from_numpy(np.asarray(off, np.uint64).view(np.int64).copy()).to(_dev())
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).to(_dev()) if prefix else None
    d_cs = torch.full((max(count, 1),), -1, dtype=torch.int32, device=_dev())
    d_ds = torch.full((max(count, 1),), -1, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    r = Encoded()
    r.rc, r.written, r.lead, r.cap = 0, 0, lead, cap
    try:
        r.written = engine.encode_frame_list_dev(src, d_off, count, level, checksum, buf.data_ptr() + lead, cap, d_cs, d_ds,
                                                 d_prefix=d_pre, prefix_len=len(prefix) if prefix else 0, dictionary=cdict)
    except zk.ZkError as ex:
        r.rc = ex.code
    torch.cuda.synchronize()
    r.all = buf.cpu().numpy()
    r.c_sizes = d_cs.cpu().numpy().astype(np.int64)[:count]
    r.d_sizes = d_ds.cpu().numpy().astype(np.int64)[:count]
    assert bytes(src[:len(data)].cpu().numpy()) == data, "the source is the caller's: untouched"
    return r


def assert_whole(r, want_frames, off):
    assert r.rc == 0
    assert r.d_sizes.tolist() == sizes_of(off)
    assert r.c_sizes.tolist() == [len(f) for f in want_frames]
    assert r.written == sum(len(f) for f in want_frames) == int(r.c_sizes.sum())
    got = r.frames()
    for i, (g, w) in enumerate(zip(got, want_frames)):
        assert g == w, (i, sizes_of(off)[i], len(g), len(w))
    outside = np.concatenate([r.all[:r.lead], r.all[r.lead + r.written:]])
    assert (outside == POISON).all()


# ---------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("level", LEVELS)
def test_identity_plain(engine, level, checksum):
    data, off = E.edge_list()
    assert_whole(dev_encode(engine, data, off, level, checksum), twin(level, checksum), off)


@pytest.mark.parametrize("plen", [3, 1000, 200000])
@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("level", LEVELS)
def test_identity_prefix(engine, level, checksum, plen):
    data, off = E.edge_list()
    assert_whole(dev_encode(engine, data, off, level, checksum, prefix=PREFIXES[plen]), twin(level, checksum, plen), off)


def test_first_offset_need_not_be_zero(engine):
    data, off = E.edge_list(lead=1237)
    assert int(off[0]) == 1237
    assert_whole(dev_encode(engine, data, off, 3, True), twin(3, True), off)


@functools.lru_cache(maxsize=None)
def cdict_of(engine, key):
    return zk.EncodeDictionary(engine, zk.Dictionary(DICTS[key]))


def dict_list():
    """records for the dictionary route: the edge list's frames up to the window as record text, and the large ones as they are"""
    data, off = E.edge_list()
    parts = [df.records(300 + i, len(f)) if 0 < len(f) <= 4097 else f for i, f in enumerate(E.frames_of(data, off))]
    return b"".join(parts), off


def single_dict_frame(engine, frame, level, checksum, cdict):
    """the existing route on these bytes alone: zk_encode_frames_dict_dev with n = size, frame_size = max(size, 1)"""
    import torch
    n = len(frame)
    cap = int(zk.lib.zk_compress_bound_dict(n, max(n, 1)))
    src = torch.zeros(n + 64, dtype=torch.uint8, device=_dev())
    if n:
        src[:n] = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(_dev())
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device=_dev())
    nf, wr = engine.encode_frames_dict_dev(src, n, max(n, 1), level, checksum, cdict, dst, cap)
    assert nf == 1
    return dst[:wr].cpu().numpy().tobytes()


@pytest.mark.parametrize("key", ["trained", "raw"])
@pytest.mark.parametrize("level", LEVELS)
def test_identity_dictionary(engine, level, key):
    import torch
    judge = libzstd_dict.judge()
    if judge is None:
        pytest.skip("libzstd 1.5.7 is not in this image")
    d = DICTS[key]
    c = cdict_of(engine, key)
    data, off = dict_list()
    checksum = level != 2
    want = [single_dict_frame(engine, f, level, checksum, c) for f in E.frames_of(data, off)]
    r = dev_encode(engine, data, off, level, checksum, cdict=c)
    assert_whole(r, want, off)
    for f, g in zip(E.frames_of(data, off), r.frames()):
        assert judge.using_dict(g, len(f) + 64, d) == f
    judge.close()
    # the engine decodes the whole output with the dictionary set, with `off` as d_off
    c_off = np.concatenate([[0], np.cumsum(r.c_sizes)]).astype(np.uint64)
    engine.set_dictionary(zk.Dictionary(d))
    try:
        arch = _upload(r.payload(), c_off, off)
        out = torch.full((len(data) + 64,), 0x5A, dtype=torch.uint8, device=_dev())
        st = torch.full((len(off) - 1,), -1, dtype=torch.int32, device=_dev())
        rc = engine.decode_frames_dev(arch[0], arch[1], arch[2], arch[3], 0, len(off) - 1, out, len(data), True, st)
        torch.cuda.synchronize()
        assert rc == 0 and not st.cpu().numpy().any()
        assert out[:len(data)].cpu().numpy().tobytes() == data
    finally:
        engine.set_dictionary(None)


# ---------------------------------------------------------------------------------------------- equal sizes
@pytest.mark.parametrize("level,fs,n", [(1, 1000, 10000), (3, 4097, 4097 * 5), (3, 70000, 210000), (2, 300000, 600000)])
def test_equal_sizes_are_the_uniform_route(engine, level, fs, n):
    data = zko.gen_text(n, 77)
    off = np.arange(0, n + 1, fs, dtype=np.uint64)
    assert int(off[-1]) == n
    want, pairs = engine.encode_frames(data, fs, level, True)
    r = dev_encode(engine, data, off, level, True)
    assert r.rc == 0 and r.payload() == want
    assert list(zip(r.c_sizes.tolist(), r.d_sizes.tolist())) == pairs
    c = cdict_of(engine, "trained")
    want, pairs = engine.encode_frames(data, fs, level, True, dictionary=c)
    r = dev_encode(engine, data, off, level, True, cdict=c)
    assert r.rc == 0 and r.payload() == want


# ---------------------------------------------------------------------------------------------- the plan, host or device
def test_plan_pin_gives_the_same_bytes(engine):
    """ZK_CHOICE_ENC_PLAN 1 (records written on the host and uploaded) and 2 (made on the device from the offsets): the same frames, on
    every route, with far history and without, and with a first offset that is not 0"""
    data, off = E.edge_list(lead=64)
    ddata, doff = dict_list()
    sdata, soff = E.small_list(8, count=2500, hi=1500)
    c = cdict_of(engine, "trained")
    got = {}
    try:
        for plan in (1, 2):
            engine.set_kernel_choice(enc_plan=plan)
            assert_whole(dev_encode(engine, data, off, 1, True), twin(1, True), off)
            assert_whole(dev_encode(engine, data, off, 3, True), twin(3, True), off)
            assert_whole(dev_encode(engine, data, off, 2, False, prefix=PREFIXES[200000]), twin(2, False, 200000), off)
            assert_whole(dev_encode(engine, data, off, 9, True, prefix=PREFIXES[3]), twin(9, True, 3), off)
            got[plan] = [dev_encode(engine, ddata, doff, 3, True, cdict=c), dev_encode(engine, sdata, soff, 1, True), dev_encode(engine, sdata, soff, 1, False, cdict=c)]
            assert all(r.rc == 0 for r in got[plan])
        for a, b in zip(got[1], got[2]):
            assert a.payload() == b.payload() and a.c_sizes.tolist() == b.c_sizes.tolist() and a.d_sizes.tolist() == b.d_sizes.tolist()
        assert got[2][1].frames() == [zko.frame_encode(f, 1, True) for f in E.frames_of(sdata, soff)]
        # a refused list under the device plan: its sums were made from the offsets as they came, and are dropped
        engine.set_kernel_choice(enc_plan=2)
        r = dev_encode(engine, data, np.array([0, 100, 99, 200], np.uint64), 1, True, cap=8192)
        assert r.rc == ERR_ARGUMENT and (r.all == POISON).all()
        assert_whole(dev_encode(engine, data, off, 3, True), twin(3, True), off)
    finally:
        engine.set_kernel_choice(reset=0)


# ---------------------------------------------------------------------------------------------- slices
def test_bytes_do_not_depend_on_the_slices(engine):
    """dense scratch of 64 KiB: every frame beyond the window exceeds a slice (never less than a frame); staged dictionary records of 1 KiB:
    a frame at a time"""
    data, off = E.edge_list()
    ddata, doff = dict_list()
    c = cdict_of(engine, "trained")
    try:
        engine.set_kernel_choice(enc_dense_slice_kib=64)
        assert_whole(dev_encode(engine, data, off, 3, True), twin(3, True), off)
        assert_whole(dev_encode(engine, data, off, 9, False), twin(9, False), off)
        engine.set_kernel_choice(reset=0)
        want = dev_encode(engine, ddata, doff, 1, True, cdict=c)
        want3 = dev_encode(engine, ddata, doff, 3, True, cdict=c)
        for kib in (1, 300):
            engine.set_kernel_choice(enc_dict_slice_kib=kib)
            assert dev_encode(engine, ddata, doff, 1, True, cdict=c).payload() == want.payload()
            assert dev_encode(engine, ddata, doff, 3, True, cdict=c).payload() == want3.payload()
    finally:
        engine.set_kernel_choice(reset=0)


# ---------------------------------------------------------------------------------------------- destinations
def test_destinations(engine):
    data, off = E.edge_list()
    want = twin(2, True)
    total = sum(len(f) for f in want)
    assert_whole(dev_encode(engine, data, off, 2, True), want, off)                     # at the bound: nothing past `written` is touched
    assert_whole(dev_encode(engine, data, off, 2, True, cap=total), want, off)
    r = dev_encode(engine, data, off, 2, True, cap=total - 1)
    assert r.rc == -70 and (r.all == POISON).all()
    for lead in (1, 3, 7):                                                              # odd addresses
        assert_whole(dev_encode(engine, data, off, 2, True, lead=lead), want, off)
    # the engine is whole after the refusal
    assert_whole(dev_encode(engine, data, off, 2, True), want, off)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(engine):
    data = zko.gen_text(4096, 3)
    c = cdict_of(engine, "trained")
    # (these offsets may claim sizes nobody allocated: the list is checked before anything is read)
    for off, kw, code in (([0, 100, 99, 200], {}, ERR_ARGUMENT),
                          ([0, 100, 100 + 0x40000001], {}, ERR_ARGUMENT),
                          ([0, 100, 200], dict(prefix=b"abcdef", cdict=c), ERR_ARGUMENT)):
        r = dev_encode(engine, data, np.array(off, np.uint64), 1, True, cap=8192, **kw)
        assert r.rc == code and (r.all == POISON).all() and (r.c_sizes == -1).all() and (r.d_sizes == -1).all(), off
    import torch
    dst = torch.full((4096,), POISON, dtype=torch.uint8, device=_dev())
    with pytest.raises(zk.ZkError) as ex:
        engine.encode_frame_list_dev(None, None, 0x08000001, 1, False, dst, 4096)      # decided before the list is read: there is none
    assert ex.value.code == ERR_FRAME_INDEX
    assert engine.encode_frame_list_dev(None, None, 0, 1, False, dst, 4096) == 0        # count == 0: nothing written
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == POISON).all()
    with pytest.raises(zk.ZkError) as ex:
        engine.encode_frame_list(data, [0, 100, 99], 1)
    assert ex.value.code == ERR_ARGUMENT
    assert engine.encode_frame_list(data, [5], 1) == (b"", [])
    # a list of one empty frame: the frame n == 0 makes
    for checksum in (False, True):
        r = dev_encode(engine, data, np.array([17, 17], np.uint64), 1, checksum)
        assert_whole(r, [zko.frame_encode(b"", 1, checksum)], np.array([17, 17], np.uint64))
        assert r.payload() == engine.encode_frames(b"", 1024, 1, checksum)[0]


# ---------------------------------------------------------------------------------------------- host route
@pytest.mark.parametrize("level", [1, 3])
def test_host_route_gives_the_same_bytes(engine, level):
    data, off = E.edge_list(lead=333)
    comp, pairs = engine.encode_frame_list(data, off, level, True)
    assert comp == b"".join(twin(level, True)) and pairs == [(len(f), s) for f, s in zip(twin(level, True), sizes_of(off))]
    comp, pairs = engine.encode_frame_list(data, off, level, False, prefix=PREFIXES[200000])
    assert comp == b"".join(twin(level, False, 200000))
    ddata, doff = dict_list()
    c = cdict_of(engine, "trained")
    comp, pairs = engine.encode_frame_list(ddata, doff, level, True, dictionary=c)
    r = dev_encode(engine, ddata, doff, level, True, cdict=c)
    assert comp == r.payload() and [p[0] for p in pairs] == r.c_sizes.tolist()
    # small records, many of them
    sdata, soff = E.small_list(5, count=300)
    comp, pairs = engine.encode_frame_list(sdata, soff, level, True)
    assert comp == b"".join(zko.frame_encode(f, level, True) for f in E.frames_of(sdata, soff))


# ---------------------------------------------------------------------------------------------- in flight
@pytest.mark.parametrize("state", IF.STATES)
def test_served_while_batches_are_in_flight(engine, state):
    """the table above zk_decode_submit_dev: zk_encode_frame_list[_dev] are served in all three busy states"""
    sdata, soff = E.small_list(11, count=60)
    want = [zko.frame_encode(f, 1, True) for f in E.frames_of(sdata, soff)]
    big = IF.engine_made(engine, 20, 640 << 10, 0x6400, repeat=8)
    with IF.Flight(engine) as fl:
        fl.reach(state, big)
        assert engine.encode_frame_list(sdata, soff, 1, True)[0] == b"".join(want)
        assert_whole(dev_encode(engine, sdata, soff, 1, True), want, soff)
        assert set(fl.live) == IF.BUSY[state]
        fl.wait_all()

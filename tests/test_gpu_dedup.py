"""zk_dedup_frames[_dev] and zk_encode_dedup[_dev] on the GPU (include/zeekstd_amd.h; zeekstd_amd/csrc/zk_dedup.hip, zk_dedup.h): ref, uniq and
ids against the model of the rule (tests/helpers/dedup_model.py: a dict from bytes to first index) entry by entry on the input list the
emulator tests share -- under every ZK_CHOICE_DEDUP_KEY_BITS of the list, from source pointers 0, 1, 3 and 7 bytes off a 256-byte boundary
--, the host-pointer call, NULL outputs, refused calls, the deduplicating encode against zk_encode_frame_list_dev on every unique frame
alone on the plain, prefix and dictionary routes in one slice and in slices of 1 KiB, tight destinations, the round trip through
zk_decode_frame_list_dev, and both calls while decode batches are in flight."""
import ctypes as C

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import cdc_model as CM
from helpers import dedup_model as M
from helpers import enc_dict_sim as S
from helpers import in_flight as IF
from helpers.dev_decode import dev as _dev

pytestmark = pytest.mark.gpu

CASES = M.cases()
POISON, GUARD = 0xA5, 4096
POISON32 = 0x5A5A5A5A
TOO_SMALL, ARG, TOO_MANY = -70, -2003, -1002
MISALIGN = dict(zip(M.KEY_BITS, (0, 1, 3, 7)))


def _i64(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).to(_dev())


def _put(c, misalign=0):
    """the case's allocation on the device, `misalign` bytes into a tensor of exactly that size (torch's allocations start on 256 bytes)
    -> (tensor, the pointer off[] counts from, device offsets)"""
    import torch
    t = torch.zeros(max(len(c.buf) + misalign, 1), dtype=torch.uint8, device=_dev())
    if len(c.buf):
        t[misalign:] = torch.from_numpy(c.buf.copy()).to(_dev())
    return t, t.data_ptr() + misalign, _i64(c.off)


def _poisoned(n):
    import torch
    return torch.full((n + 8,), POISON32, dtype=torch.int32, device=_dev())


def dev_map(engine, c, bits=0, misalign=0):
    import torch
    t, p, d_off = _put(c, misalign)
    ref, ids, uniq = (_poisoned(c.count) for _ in range(3))
    nu = C.c_uint32(12345)
    torch.cuda.synchronize()
    try:
        engine.set_kernel_choice(dedup_key_bits=bits)
        rc = zk.lib.zk_dedup_frames_dev(engine._h, p, d_off.data_ptr(), c.count, ref.data_ptr(), ids.data_ptr(), uniq.data_ptr(), C.byref(nu), None)
    finally:
        engine.set_kernel_choice(dedup_key_bits=0)
    torch.cuda.synchronize()
    return rc, nu.value, [x.cpu().numpy().view(np.uint32) for x in (ref, ids, uniq)]


def assert_map(c, nu, ref, ids, uniq, padded=True):
    want_ref, want_uniq, want_ids = c.model()
    assert nu == len(want_uniq), (nu, len(want_uniq))
    for name, got, want in (("ref", ref, want_ref), ("ids", ids, want_ids), ("uniq", uniq, want_uniq)):
        bad = np.nonzero(got[:len(want)] != want)[0]
        assert bad.size == 0, (name, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
        if padded:
            assert (got[len(want):] == POISON32).all(), name


@pytest.mark.parametrize("bits", M.KEY_BITS)
@pytest.mark.parametrize("name", list(CASES))
def test_map_equals_the_model(engine, name, bits):
    """zk_dedup_frames_dev under every key width: the same three arrays, nothing written behind them"""
    c = CASES[name]
    rc, nu, (ref, ids, uniq) = dev_map(engine, c, bits, MISALIGN[bits])
    assert rc == 0
    assert_map(c, nu, ref, ids, uniq)


@pytest.mark.parametrize("name", list(CASES))
def test_host_call_equals_the_model(engine, name):
    c = CASES[name]
    ref, ids, uniq = engine.dedup_frames(c.buf, c.off)
    assert ref.dtype == ids.dtype == uniq.dtype == np.uint32
    assert_map(c, len(uniq), ref, ids, uniq, padded=False)
    if name in ("edges", "far_pairs"):
        try:
            engine.set_kernel_choice(dedup_key_bits=4)
            ref, ids, uniq = engine.dedup_frames(c.buf, c.off)
        finally:
            engine.set_kernel_choice(dedup_key_bits=0)
        assert_map(c, len(uniq), ref, ids, uniq, padded=False)


def test_null_outputs_and_python_device_call(engine):
    import torch
    c = CASES["enc_mix"]
    want_ref, want_uniq, want_ids = c.model()
    t, p, d_off = _put(c, 3)
    assert engine.dedup_frames_dev(p, d_off, c.count) == len(want_uniq)
    for which in range(3):
        arrs = [None, None, None]
        arrs[which] = _poisoned(c.count)
        assert engine.dedup_frames_dev(p, d_off, c.count, *arrs) == len(want_uniq)
        torch.cuda.synchronize()
        want = (want_ref, want_ids, want_uniq)[which]
        got = arrs[which].cpu().numpy().view(np.uint32)
        assert (got[:len(want)] == want).all() and (got[len(want):] == POISON32).all()
    nu = C.c_uint32(7)
    assert zk.lib.zk_dedup_frames_dev(engine._h, None, None, 0, None, None, None, C.byref(nu), None) == 0 and nu.value == 0
    nu = C.c_uint32(7)
    assert zk.lib.zk_dedup_frames(engine._h, None, None, 0, None, None, None, C.byref(nu)) == 0 and nu.value == 0
    assert zk.lib.zk_dedup_frames_dev(engine._h, p, d_off.data_ptr(), c.count, None, None, None, None, None) == ARG


def test_refused_calls_write_nothing(engine):
    """a decreasing list, a frame above ZK_SEEKABLE_MAX_FRAME_SIZE, more frames than ZK_SEEKABLE_MAX_FRAMES: the code of
    zk_encode_frame_list_dev, and the poisoned arrays and destination as they were"""
    import torch
    c = CASES["enc_mix"]
    t, p, _ = _put(c)
    falling = c.off.copy()
    falling[5] = falling[4] - 1
    oversize = np.array([0, 10, 10 + 0x40000001, 20 + 0x40000001], np.uint64)
    dst = torch.full((1 << 16,), POISON, dtype=torch.uint8, device=_dev())
    for off, count, want in ((falling, c.count, ARG), (oversize, 3, ARG), (c.off, 0x08000001, TOO_MANY)):
        d_off = _i64(off)
        arrs = [_poisoned(c.count) for _ in range(5)]
        nu, wr = C.c_uint32(12345), C.c_uint64(12345)
        torch.cuda.synchronize()
        rc = zk.lib.zk_dedup_frames_dev(engine._h, p, d_off.data_ptr(), count, arrs[0].data_ptr(), arrs[1].data_ptr(), arrs[2].data_ptr(), C.byref(nu), None)
        assert rc == want and nu.value == 0
        rc = zk.lib.zk_encode_dedup_dev(engine._h, p, d_off.data_ptr(), count, 1, 0, None, 0, None, dst.data_ptr(), 1 << 16, arrs[1].data_ptr(), arrs[2].data_ptr(),
                                        arrs[3].data_ptr(), arrs[4].data_ptr(), C.byref(nu), C.byref(wr), None)
        torch.cuda.synchronize()
        assert rc == want and nu.value == 0 and wr.value == 12345
        for a in arrs:
            assert (a.cpu().numpy().view(np.uint32) == POISON32).all()
        assert (dst.cpu().numpy() == POISON).all()
        host = [np.full(c.count, POISON32, np.uint32) for _ in range(5)]
        hdst = np.full(1 << 16, POISON, np.uint8)
        assert zk.lib.zk_dedup_frames(engine._h, c.buf.ctypes.data, off.ctypes.data, count, host[0].ctypes.data, host[1].ctypes.data, host[2].ctypes.data, C.byref(nu)) == want
        assert zk.lib.zk_encode_dedup(engine._h, c.buf.ctypes.data, off.ctypes.data, count, 1, 0, None, 0, None, hdst.ctypes.data, 1 << 16, host[1].ctypes.data,
                                      host[2].ctypes.data, host[3].ctypes.data, host[4].ctypes.data, C.byref(nu), C.byref(wr)) == want
        assert all((a == POISON32).all() for a in host) and (hdst == POISON).all()


def test_kernel_choice_ranges(engine):
    for key, bad in (("dedup_key_bits", (-1, 65)), ("dedup_slice_kib", (-1, (1 << 22) + 1))):
        for v in bad:
            with pytest.raises(zk.ZkError):
                engine.set_kernel_choice(**{key: v})
    engine.set_kernel_choice(dedup_key_bits=64, dedup_slice_kib=1 << 22)
    engine.set_kernel_choice(reset=0)


def test_kernel_times_name_the_map(engine):
    c = CASES["enc_mix"]
    zk.lib.zk_engine_set_profiling(engine._h, 1)
    try:
        rc, nu, _ = dev_map(engine, c)
        times = engine.kernel_times()
    finally:
        zk.lib.zk_engine_set_profiling(engine._h, 0)
    assert rc == 0
    assert {"zk_k_dedup_hash", "zk_k_dedup_insert", "zk_k_dedup_verify", "zk_k_dedup_verify_long", "zk_k_dedup_compact"} <= set(times), times


# ---------------------------------------------------------------------------------------------- each distinct frame encoded once
class Enc:
    pass


PREFIX = CM.word_text(21, 3000).tobytes()


def dev_encode_list(engine, data, off, level, checksum, prefix=None, cdict=None):
    """zk_encode_frame_list_dev on the given offsets -> (payload, c_sizes, d_sizes)"""
    import torch
    count = len(off) - 1
    cap = int(zk.lib.zk_compress_bound_list(len(data), count, int(cdict is not None)))
    src = torch.from_numpy(np.frombuffer(bytes(data) + b"\0", np.uint8).copy()).to(_dev())
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device=_dev())
    cs = torch.zeros(count, dtype=torch.int32, device=_dev())
    ds = torch.zeros(count, dtype=torch.int32, device=_dev())
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).to(_dev()) if prefix else None
    wr = engine.encode_frame_list_dev(src, _i64(off), count, level, checksum, dst, cap, cs, ds, d_prefix=d_pre, prefix_len=len(prefix) if prefix else 0, dictionary=cdict)
    torch.cuda.synchronize()
    return dst[:wr].cpu().numpy().tobytes(), cs.cpu().numpy().astype(np.int64), ds.cpu().numpy().astype(np.int64)


def dev_encode_dedup(engine, c, level, checksum, prefix=None, cdict=None, dst_cap=None, slice_kib=0, misalign=0):
    import torch
    n = int(c.off[-1] - c.off[0])
    bound = int(zk.lib.zk_compress_bound_list(n, c.count, int(cdict is not None)))
    cap = bound if dst_cap is None else dst_cap
    t, p, d_off = _put(c, misalign)
    dst = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    ids, uniq, cs, ds = (_poisoned(c.count) for _ in range(4))
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).to(_dev()) if prefix else None
    torch.cuda.synchronize()
    r = Enc()
    r.rc, r.n_unique, r.written, r.bound = 0, 0, 0, bound
    try:
        engine.set_kernel_choice(dedup_slice_kib=slice_kib)
        r.n_unique, r.written = engine.encode_dedup_dev(p, d_off, c.count, level, checksum, dst, cap, ids, uniq, cs, ds, d_prefix=d_pre,
                                                        prefix_len=len(prefix) if prefix else 0, dictionary=cdict)
    except zk.ZkError as ex:
        r.rc = ex.code
    finally:
        engine.set_kernel_choice(dedup_slice_kib=0)
    torch.cuda.synchronize()
    r.all = dst.cpu().numpy()
    r.ids, r.uniq, r.c_sizes, r.d_sizes = (x.cpu().numpy().view(np.uint32) for x in (ids, uniq, cs, ds))
    return r


def expand(c, frames):
    """the source from the decoded unique frames and the model's ids"""
    return b"".join(frames[int(k)] for k in c.model()[2])


@pytest.mark.parametrize("route", ["plain", "prefix", "dictionary"])
@pytest.mark.parametrize("level", [1, 3])
def test_encode_dedup_dev(engine, level, route):
    import torch
    c = CASES["enc_mix"]
    prefix = PREFIX if route == "prefix" else None
    d = S.fixture_dicts()["trained"] if route == "dictionary" else None
    cdict = zk.EncodeDictionary(engine, zk.Dictionary(d)) if d else None
    try:
        want_ref, want_uniq, want_ids = c.model()
        nu = len(want_uniq)
        # the reference, once: zk_encode_frame_list_dev on every unique frame alone
        alone = [dev_encode_list(engine, c.frames[int(u)], [0, len(c.frames[int(u)])], level, True, prefix, cdict) for u in want_uniq]
        want = b"".join(a[0] for a in alone)
        want_cs = [int(a[1][0]) for a in alone]
        want_ds = [len(c.frames[int(u)]) for u in want_uniq]
        assert [int(a[2][0]) for a in alone] == want_ds
        for slice_kib, misalign in ((0, 0), (1, 3)):
            r = dev_encode_dedup(engine, c, level, True, prefix, cdict, slice_kib=slice_kib, misalign=misalign)
            assert r.rc == 0 and r.n_unique == nu and r.written == len(want) <= r.bound, (slice_kib, r.rc, r.n_unique, r.written, len(want))
            assert (r.ids[:c.count] == want_ids).all() and (r.ids[c.count:] == POISON32).all()
            assert (r.uniq[:nu] == want_uniq).all() and (r.uniq[nu:] == POISON32).all()
            assert r.c_sizes[:nu].tolist() == want_cs and (r.c_sizes[nu:] == POISON32).all()
            assert r.d_sizes[:nu].tolist() == want_ds and (r.d_sizes[nu:] == POISON32).all()
            assert r.all[:r.written].tobytes() == want, slice_kib
            assert (r.all[r.written:] == POISON).all()                   # untouched past `written`
            # one byte short: -70 and nothing written, in one slice and in many
            r = dev_encode_dedup(engine, c, level, True, prefix, cdict, dst_cap=len(want) - 1, slice_kib=slice_kib)
            assert r.rc == TOO_SMALL and (r.all == POISON).all(), slice_kib
            # exactly enough, far below the bound
            r = dev_encode_dedup(engine, c, level, True, prefix, cdict, dst_cap=len(want), slice_kib=slice_kib)
            assert r.rc == 0 and r.written == len(want) and r.all[:r.written].tobytes() == want and (r.all[r.written:] == POISON).all()
        # the host-pointer call gives the same bytes, with the offsets it was given
        comp, off, cs, ds, ids = engine.encode_dedup(c.buf, c.off, level=level, checksum=True, prefix=prefix, dictionary=cdict)
        assert comp == want and cs.tolist() == want_cs and ds.tolist() == want_ds and ids.tolist() == want_ids.tolist() and off.tolist() == c.off.tolist()
        # reading back.  The unique frames decode (against the prefix or the dictionary) to the unique contents ...
        c_off = np.concatenate([[0], np.cumsum(want_cs)]).astype(np.uint64)
        d_off = np.concatenate([[0], np.cumsum(want_ds)]).astype(np.uint64)
        if d:
            engine.set_dictionary(zk.Dictionary(d))
        try:
            out, st = engine.decode_frames(want + b"\0" * 8, c_off, d_off, verify=True, prefix=prefix)
            assert not st.any()
            frames = [out[int(a):int(b)] for a, b in zip(d_off[:-1], d_off[1:])]
            assert expand(c, frames) == c.buf[c.lead:].tobytes()
            # ... and zk_decode_frame_list_dev with ids and the original offsets writes the source (it takes no prefix)
            if not prefix:
                n = int(c.off[-1] - c.off[0])
                d_comp = torch.from_numpy(np.frombuffer(want + b"\0" * 64, np.uint8).copy()).to(_dev())
                dst = torch.full((n + 64,), POISON, dtype=torch.uint8, device=_dev())
                status = torch.full((c.count,), -1, dtype=torch.int32, device=_dev())
                rc = engine.decode_frame_list_dev(d_comp, len(want), _i64(c_off), _i64(d_off), torch.from_numpy(want_ids.view(np.int32).copy()).to(_dev()),
                                                  _i64(c.off - c.off[0]), c.count, dst, n, True, status)
                torch.cuda.synchronize()
                assert rc == 0 and not status.cpu().numpy().any()
                assert dst[:n].cpu().numpy().tobytes() == c.buf[c.lead:].tobytes() and (dst[n:].cpu().numpy() == POISON).all()
        finally:
            engine.set_dictionary(None)
    finally:
        if cdict is not None:
            cdict.close()


def test_a_list_without_duplicates_and_one_of_one_content(engine):
    """n_unique == count takes the list encoder where the frames lie; 600 copies are one frame"""
    for name in ("all_distinct", "all_same", "one", "one_empty"):
        c = CASES[name]
        want_ref, want_uniq, want_ids = c.model()
        want, want_cs, _ = dev_encode_list(engine, c.unique_bytes(), np.concatenate([[0], np.cumsum([len(c.frames[int(u)]) for u in want_uniq])]), 1, True)
        for slice_kib in (0, 1):
            r = dev_encode_dedup(engine, c, 1, True, slice_kib=slice_kib, misalign=1)
            assert r.rc == 0 and r.n_unique == len(want_uniq) and (r.ids[:c.count] == want_ids).all()
            assert r.all[:r.written].tobytes() == want and (r.all[r.written:] == POISON).all()
            assert r.c_sizes[:r.n_unique].tolist() == want_cs.tolist()


def test_round_trip_of_a_chunked_input(engine):
    """text with repeated paragraphs, cut by content at avg_size 256: Engine.encode_dedup stores each distinct chunk once, and
    zk_decode_frame_list_dev with ids and the offsets returns the source"""
    import torch
    rng = np.random.default_rng(9)
    paragraphs = [CM.word_text(100 + k, int(n)).tobytes() for k, n in enumerate(rng.integers(600, 3000, 12))]
    data = np.frombuffer(b"".join(paragraphs[int(k)] for k in rng.integers(0, 12, 60)), np.uint8)
    n = len(data)
    d_src = torch.from_numpy(data.copy()).to(_dev())
    d_off = engine.chunk_boundaries_dev(d_src, n, avg_size=256)
    comp, off, cs, ds, ids = engine.encode_dedup(data, avg_size=256, level=1, checksum=True)
    assert off.tolist() == d_off.cpu().numpy().view(np.uint64).tolist()
    count = len(off) - 1
    frames = [data[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])]
    want_ref, want_uniq, want_ids = M.model(frames)
    assert ids.tolist() == want_ids.tolist() and len(cs) == len(want_uniq) < count
    assert ds.tolist() == [len(frames[int(u)]) for u in want_uniq]
    print("chunks:", count, "distinct:", len(cs), "payload:", len(comp), "of", n)
    c_off = np.concatenate([[0], np.cumsum(cs.astype(np.int64))]).astype(np.uint64)
    u_off = np.concatenate([[0], np.cumsum(ds.astype(np.int64))]).astype(np.uint64)
    d_comp = torch.from_numpy(np.frombuffer(comp + b"\0" * 64, np.uint8).copy()).to(_dev())
    dst = torch.full((n + 64,), POISON, dtype=torch.uint8, device=_dev())
    status = torch.full((count,), -1, dtype=torch.int32, device=_dev())
    rc = engine.decode_frame_list_dev(d_comp, len(comp), _i64(c_off), _i64(u_off), torch.from_numpy(ids.view(np.int32).copy()).to(_dev()), d_off, count, dst, n, True, status)
    torch.cuda.synchronize()
    assert rc == 0 and not status.cpu().numpy().any()
    assert dst[:n].cpu().numpy().tobytes() == data.tobytes()


def test_the_list_encoder_still_writes_every_frame(engine):
    """existing behaviour: zk_encode_frame_list_dev on an input with duplicates encodes each of them"""
    c = CASES["enc_mix"]
    comp, cs, ds = dev_encode_list(engine, c.buf[c.lead:].tobytes(), c.off - c.off[0], 1, True)
    assert len(cs) == c.count and (cs > 0).all() and int(cs.sum()) == len(comp) and ds.tolist() == [len(f) for f in c.frames]
    at = np.concatenate([[0], np.cumsum(cs)])
    pieces = {}
    for i, f in enumerate(c.frames):
        pieces.setdefault(f, set()).add(comp[int(at[i]):int(at[i + 1])])
    assert all(len(v) == 1 for v in pieces.values())                 # equal frames, equal bytes -- written once per frame all the same
    r = dev_encode_dedup(engine, c, 1, True)
    assert r.written < len(comp)


def test_served_while_batches_are_in_flight(engine):
    """both decode contexts hold a submitted batch: the map and the deduplicating encode are served with the results they have when idle"""
    c = CASES["enc_mix"]
    idle = dev_encode_dedup(engine, c, 1, True, slice_kib=1)
    assert idle.rc == 0
    with IF.Flight(engine) as fl:
        fl.reach("both", IF.Staged(IF.long_()), IF.Staged(IF.long_()))
        rc, nu, (ref, ids, uniq) = dev_map(engine, c, 4, 3)
        assert rc == 0
        assert_map(c, nu, ref, ids, uniq)
        busy = dev_encode_dedup(engine, c, 1, True, slice_kib=1)
        assert busy.rc == 0 and busy.written == idle.written and (busy.all == idle.all).all() and (busy.ids == idle.ids).all()
        assert set(fl.live) == IF.BUSY["both"]
        fl.wait_all()

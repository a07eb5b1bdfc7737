"""zk_chunk_boundaries[_dev] and zk_encode_chunked[_dev] on the GPU (include/zeekstd_amd.h; zeekstd_amd/csrc/zk_cdc.hip, zk_cdc.h): the
offsets against the numpy model of the rule (tests/helpers/cdc_model.py) bit for bit on the input list the emulator tests share -- in one
slice and in slices of 1 KiB, from source pointers 0, 1, 3 and 7 bytes off a 256-byte boundary --, the host-pointer call, a destination for the offsets that is too
small, the chunked encode against zk_encode_frame_list_dev on the model's offsets on the plain, prefix and dictionary routes, min == max
against the uniform route, what an insertion leaves of the compressed frames, and both calls while decode batches are in flight."""
import ctypes as C

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import cdc_model as M
from helpers import dict_fixtures as df
from helpers import enc_dict_sim as S
from helpers import in_flight as IF
from helpers.dev_decode import dev as _dev

pytestmark = pytest.mark.gpu

CASES = M.cases()
POISON, GUARD = 0xA5, 4096
POISON64 = 0x5A5A5A5A5A5A5A5A
TOO_SMALL, ARG = -70, -2003


def _src(data, misalign=0):
    """the bytes on the device, `misalign` bytes into a tensor (torch's allocations start on 256 bytes)"""
    import torch
    t = torch.zeros(len(data) + misalign + 64, dtype=torch.uint8, device=_dev())
    if len(data):
        t[misalign:misalign + len(data)] = torch.from_numpy(np.ascontiguousarray(data).copy()).to(_dev())
    return t


def dev_cuts(engine, data, mn, avg, mx, misalign=0, off_cap=None):
    """one zk_chunk_boundaries_dev call into a poisoned array of off_cap + 1 entries (by default n / min + 1) -> (rc, count, the whole array)"""
    import torch
    n = len(data)
    t = _src(data, misalign)
    res = M.resolve(mn, avg, mx)
    cap = n // res[0] + 1 if off_cap is None else off_cap
    off = torch.full((cap + 1 + 8,), POISON64, dtype=torch.int64, device=_dev())
    par = zk._lib.ChunkParams(mn, avg, mx, 0)
    count = C.c_uint32(0xFFFFFFFF)
    torch.cuda.synchronize()
    rc = zk.lib.zk_chunk_boundaries_dev(engine._h, t.data_ptr() + misalign if n else None, n, C.byref(par), off.data_ptr(), cap, C.byref(count), None)
    torch.cuda.synchronize()
    return rc, count.value, off.cpu().numpy().view(np.uint64)


def assert_cuts(engine, c, misalign=0):
    want = c.cuts()
    rc, count, off = dev_cuts(engine, c.data, c.mn, c.avg, c.mx, misalign)
    assert rc == 0 and count == len(want) - 1, (rc, count, len(want) - 1)
    assert (off[:count + 1] == want).all(), int(np.nonzero(off[:count + 1] != want)[0][0])
    assert (off[count + 1:] == POISON64).all()


@pytest.mark.parametrize("name", list(CASES))
def test_offsets_equal_the_model(engine, name):
    """one slice from an aligned pointer; slices of 1 KiB (a seam every 1024 bytes) from pointer + 1; one slice from pointer + 3 and + 7"""
    c = CASES[name]
    assert_cuts(engine, c)
    try:
        engine.set_kernel_choice(cdc_slice_kib=1)
        assert_cuts(engine, c, 1)
    finally:
        engine.set_kernel_choice(cdc_slice_kib=0)
    assert_cuts(engine, c, 3)
    assert_cuts(engine, c, 7)


@pytest.mark.parametrize("name", list(CASES))
def test_host_call_gives_the_same_offsets(engine, name):
    c = CASES[name]
    want = c.cuts()
    got = engine.chunk_boundaries(c.data, c.avg, c.mn, c.mx)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist()
    if name.startswith(("random", "text", "dense_mid", "len")):
        try:
            engine.set_kernel_choice(cdc_slice_kib=1)
            assert engine.chunk_boundaries(c.data, c.avg, c.mn, c.mx).tolist() == want.tolist()
        finally:
            engine.set_kernel_choice(cdc_slice_kib=0)


def test_python_device_call_and_defaults(engine):
    """min = max = 0 are avg / 4 and 4 avg; a device tensor comes back"""
    c = CASES["text_1024"]
    want = M.cuts(c.data, *M.resolve(0, 1024, 0))
    assert M.resolve(0, 1024, 0) == (256, 10, 4096)
    got = engine.chunk_boundaries_dev(_src(c.data), len(c.data), avg_size=1024)
    assert got.is_cuda and got.cpu().numpy().view(np.uint64).tolist() == want.tolist()
    # every default: one frame of an input below min = 512 KiB, and NULL parameters are the same
    assert engine.chunk_boundaries(c.data).tolist() == [0, len(c.data)]
    count = C.c_uint32()
    off = np.zeros(2, np.uint64)
    assert zk.lib.zk_chunk_boundaries(engine._h, c.data.ctypes.data, len(c.data), None, off.ctypes.data, 1, C.byref(count)) == 0
    assert count.value == 1 and off.tolist() == [0, len(c.data)]


@pytest.mark.parametrize("row", M.PARAM_TABLE)
def test_parameter_table_with_an_engine(engine, row):
    """every row through zk_chunk_boundaries_dev, zk_chunk_boundaries and zk_encode_chunked_dev on a live engine: an accepted row gives the
    model's cuts under the resolved defaults; a refused one -2003 with the count, the offsets and the destination as they were"""
    import torch
    mn, avg, mx, flags = row
    want = M.resolve(mn, avg, mx, flags)
    data = CASES["text_1024"].data
    n = len(data)
    par = zk._lib.ChunkParams(mn, avg, mx, flags)
    cap = n // 64 + 1
    t = _src(data)
    off = torch.full((cap + 1,), POISON64, dtype=torch.int64, device=_dev())
    host = np.full(cap + 1, POISON64, np.uint64)
    dst_cap = int(zk.lib.zk_compress_bound_list(n, cap, 0))
    dst = torch.full((dst_cap,), POISON, dtype=torch.uint8, device=_dev())
    cs = torch.full((cap,), -1, dtype=torch.int32, device=_dev())
    count, hcount, nf, wr = C.c_uint32(12345), C.c_uint32(12345), C.c_uint32(12345), C.c_uint64(12345)
    torch.cuda.synchronize()
    rc = zk.lib.zk_chunk_boundaries_dev(engine._h, t.data_ptr(), n, C.byref(par), off.data_ptr(), cap, C.byref(count), None)
    hrc = zk.lib.zk_chunk_boundaries(engine._h, data.ctypes.data, n, C.byref(par), host.ctypes.data, cap, C.byref(hcount))
    torch.cuda.synchronize()
    got = off.cpu().numpy().view(np.uint64)
    if want is None:
        assert rc == ARG and hrc == ARG and count.value == 12345 and hcount.value == 12345
        assert (got == POISON64).all() and (host == POISON64).all()
        erc = zk.lib.zk_encode_chunked_dev(engine._h, t.data_ptr(), n, C.byref(par), 1, 0, None, 0, None, dst.data_ptr(), dst_cap, off.data_ptr(), cap,
                                           cs.data_ptr(), None, C.byref(nf), C.byref(wr), None)
        torch.cuda.synchronize()
        assert erc == ARG and nf.value == 12345 and wr.value == 12345
        assert (off.cpu().numpy().view(np.uint64) == POISON64).all() and (dst.cpu().numpy() == POISON).all() and (cs.cpu().numpy() == -1).all()
        assert int(zk.lib.zk_compress_bound_chunked(n, C.byref(par), 0)) == 0
    else:
        cuts = M.cuts(data, *want)
        k = len(cuts) - 1
        assert rc == 0 and hrc == 0 and count.value == k and hcount.value == k
        assert (got[:k + 1] == cuts).all() and (got[k + 1:] == POISON64).all()
        assert (host[:k + 1] == cuts).all() and (host[k + 1:] == POISON64).all()
        erc = zk.lib.zk_encode_chunked_dev(engine._h, t.data_ptr(), n, C.byref(par), 1, 0, None, 0, None, dst.data_ptr(), dst_cap, off.data_ptr(), cap,
                                           cs.data_ptr(), None, C.byref(nf), C.byref(wr), None)
        torch.cuda.synchronize()
        assert erc == 0 and nf.value == k and int(cs.cpu().numpy()[:k].sum()) == wr.value <= int(zk.lib.zk_compress_bound_chunked(n, C.byref(par), 0))


@pytest.mark.parametrize("name", ["random_1024", "len0_256", "dense_mid_256"])
def test_small_off_cap(engine, name):
    """off_cap one below count: -70, the count, and nothing written; the size query with a NULL array; the host call alike"""
    c = CASES[name]
    want = c.cuts()
    count = len(want) - 1
    rc, got, off = dev_cuts(engine, c.data, c.mn, c.avg, c.mx, off_cap=count - 1)
    assert rc == TOO_SMALL and got == count and (off == POISON64).all()
    rc, got, off = dev_cuts(engine, c.data, c.mn, c.avg, c.mx, off_cap=count)             # exactly enough: below n / min + 1, so counted first
    assert rc == 0 and got == count and (off[:count + 1] == want).all() and (off[count + 1:] == POISON64).all()
    par = zk._lib.ChunkParams(c.mn, c.avg, c.mx, 0)
    n_out = C.c_uint32()
    t = _src(c.data)
    assert zk.lib.zk_chunk_boundaries_dev(engine._h, t.data_ptr() if len(c.data) else None, len(c.data), C.byref(par), None, 0, C.byref(n_out), None) == TOO_SMALL
    assert n_out.value == count
    host = np.full(count + 1, POISON64, np.uint64)
    n_out = C.c_uint32()
    rc = zk.lib.zk_chunk_boundaries(engine._h, c.data.ctypes.data if len(c.data) else None, len(c.data), C.byref(par), host.ctypes.data, count - 1, C.byref(n_out))
    assert rc == TOO_SMALL and n_out.value == count and (host == POISON64).all()


# ---------------------------------------------------------------------------------------------- the chunked encode
class Enc:
    pass


def dev_encode_chunked(engine, data, mn, avg, mx, level, checksum, prefix=None, cdict=None, dst_cap=None, off_cap=None):
    import torch
    n = len(data)
    par = zk._lib.ChunkParams(mn, avg, mx, 0)
    bound = int(zk.lib.zk_compress_bound_chunked(n, C.byref(par), int(cdict is not None)))
    cap = bound if dst_cap is None else dst_cap
    frames = n // M.resolve(mn, avg, mx)[0] + 1 if off_cap is None else off_cap
    src = _src(data)
    dst = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    off = torch.full((frames + 1 + 8,), POISON64, dtype=torch.int64, device=_dev())
    cs = torch.full((max(frames, 1),), -1, dtype=torch.int32, device=_dev())
    ds = torch.full((max(frames, 1),), -1, dtype=torch.int32, device=_dev())
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).to(_dev()) if prefix else None
    torch.cuda.synchronize()
    r = Enc()
    r.rc, r.frames, r.written, r.bound = 0, 0, 0, bound
    try:
        r.frames, r.written = engine.encode_chunked_dev(src, n, dst, cap, off, frames, avg, mn, mx, level, checksum, cs, ds,
                                                        d_prefix=d_pre, prefix_len=len(prefix) if prefix else 0, dictionary=cdict)
    except zk.ZkError as ex:
        r.rc = ex.code
    torch.cuda.synchronize()
    r.all = dst.cpu().numpy()
    r.off = off.cpu().numpy().view(np.uint64)
    r.c_sizes = cs.cpu().numpy().astype(np.int64)
    r.d_sizes = ds.cpu().numpy().astype(np.int64)
    return r


def dev_encode_list(engine, data, off, level, checksum, prefix=None, cdict=None):
    """zk_encode_frame_list_dev on the given offsets -> (payload, c_sizes, d_sizes)"""
    import torch
    count = len(off) - 1
    cap = int(zk.lib.zk_compress_bound_list(len(data), count, int(cdict is not None)))
    src = _src(data)
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device=_dev())
    d_off = torch.from_numpy(np.asarray(off, np.uint64).view(np.int64).copy()).to(_dev())
    cs = torch.zeros(count, dtype=torch.int32, device=_dev())
    ds = torch.zeros(count, dtype=torch.int32, device=_dev())
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).to(_dev()) if prefix else None
    wr = engine.encode_frame_list_dev(src, d_off, count, level, checksum, dst, cap, cs, ds, d_prefix=d_pre, prefix_len=len(prefix) if prefix else 0, dictionary=cdict)
    torch.cuda.synchronize()
    return dst[:wr].cpu().numpy().tobytes(), cs.cpu().numpy().astype(np.int64), ds.cpu().numpy().astype(np.int64)


PREFIX = M.word_text(21, 3000).tobytes()


def routes():
    return {"plain_random": (CASES["random_4096"].data, (1024, 4096, 16384), None, False),
            "plain_text": (CASES["text_1024"].data, (256, 1024, 4096), None, False),
            "prefix": (M.word_text(2, 60000), (256, 1024, 4096), PREFIX, False),
            "dictionary": (np.frombuffer(df.records(77, 40000), np.uint8), (64, 256, 1024), None, True)}


@pytest.mark.parametrize("route", ["plain_random", "plain_text", "prefix", "dictionary"])
@pytest.mark.parametrize("level", [1, 3])
def test_encode_chunked_dev(engine, level, route):
    data, (mn, avg, mx), prefix, with_dict = routes()[route]
    d = S.fixture_dicts()["trained"] if with_dict else None
    cdict = zk.EncodeDictionary(engine, zk.Dictionary(d)) if with_dict else None
    try:
        want_off = M.cuts(data, mn, avg.bit_length() - 1, mx)
        count = len(want_off) - 1
        want, want_cs, want_ds = dev_encode_list(engine, data, want_off, level, True, prefix, cdict)
        r = dev_encode_chunked(engine, data, mn, avg, mx, level, True, prefix, cdict)
        assert r.rc == 0 and r.frames == count and r.written == len(want) <= r.bound
        assert (r.off[:count + 1] == want_off).all() and (r.off[count + 1:] == POISON64).all()
        assert r.all[:r.written].tobytes() == want and (r.all[r.written:] == POISON).all()
        assert r.c_sizes[:count].tolist() == want_cs.tolist() and r.d_sizes[:count].tolist() == want_ds.tolist() == np.diff(want_off.astype(np.int64)).tolist()
        # the engine decodes the frames with the returned offsets
        c_off = np.concatenate([[0], np.cumsum(r.c_sizes[:count])]).astype(np.uint64)
        if with_dict:
            engine.set_dictionary(zk.Dictionary(d))
        try:
            out, st = engine.decode_frames(want + b"\0" * 8, c_off, r.off[:count + 1], verify=True, prefix=prefix)
        finally:
            engine.set_dictionary(None)
        assert not st.any() and out == data.tobytes()
        # the host-pointer call gives the same bytes
        comp, off, cs = engine.encode_chunked(data, avg, mn, mx, level, True, prefix=prefix, dictionary=cdict)
        assert comp == want and off.tolist() == want_off.tolist() and cs.tolist() == want_cs.tolist()
        # a destination one byte short: -70, nothing written; offsets that find no room: -70 before anything is encoded
        r = dev_encode_chunked(engine, data, mn, avg, mx, level, True, prefix, cdict, dst_cap=len(want) - 1)
        assert r.rc == TOO_SMALL and (r.all == POISON).all()
        r = dev_encode_chunked(engine, data, mn, avg, mx, level, True, prefix, cdict, off_cap=count - 1)
        assert r.rc == TOO_SMALL and (r.all == POISON).all() and (r.off == POISON64).all()
    finally:
        if cdict is not None:
            cdict.close()


@pytest.mark.parametrize("level", [1, 3])
def test_equal_sizes_are_the_uniform_route(engine, level):
    import torch
    data = CASES["text_4096"].data[:150000]
    r = dev_encode_chunked(engine, data, 4096, 4096, 4096, level, True)
    nf = -(-len(data) // 4096)
    cap = int(zk.lib.zk_compress_bound(len(data), 4096))
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device=_dev())
    cs = torch.zeros(nf, dtype=torch.int32, device=_dev())
    got_nf, wr = engine.encode_frames_dev(_src(data), len(data), 4096, level, True, dst, cap, cs)
    assert r.rc == 0 and r.frames == got_nf == nf and r.written == wr
    assert r.all[:wr].tobytes() == dst[:wr].cpu().numpy().tobytes()
    assert r.c_sizes[:nf].tolist() == cs.cpu().numpy().tolist()
    assert r.off[:nf + 1].tolist() == list(range(0, len(data), 4096)) + [len(data)]


def test_an_insertion_leaves_the_other_frames_as_they_were(engine):
    """the 256 KiB random input and the same with 33 bytes inserted at 100 000: at most 8 compressed frames of the second are not frames of
    the first"""
    data = CASES["random_1024"].data
    edited = np.concatenate([data[:100000], M.rand(55, 33), data[100000:]])
    frames = []
    for d in (data, edited):
        comp, off, cs = engine.encode_chunked(d, 1024, 256, 4096, 1, True)
        at = np.concatenate([[0], np.cumsum(cs.astype(np.int64))])
        assert at[-1] == len(comp)
        frames.append([comp[int(a):int(b)] for a, b in zip(at[:-1], at[1:])])
    old = set(frames[0])
    new = sum(f not in old for f in frames[1])
    print("frames of the edited input that are new:", new, "of", len(frames[1]))
    assert 1 <= new <= 8


def test_served_while_batches_are_in_flight(engine):
    """both decode contexts hold a submitted batch: the boundaries and the chunked encode are served with the results they have when idle"""
    c = CASES["text_1024"]
    want = c.cuts()
    idle = dev_encode_chunked(engine, c.data, c.mn, c.avg, c.mx, 1, True)
    assert idle.rc == 0
    with IF.Flight(engine) as fl:
        fl.reach("both", IF.Staged(IF.long_()), IF.Staged(IF.long_()))
        rc, count, off = dev_cuts(engine, c.data, c.mn, c.avg, c.mx, misalign=3)
        assert rc == 0 and count == len(want) - 1 and (off[:count + 1] == want).all()
        assert engine.chunk_boundaries(c.data, c.avg, c.mn, c.mx).tolist() == want.tolist()
        busy = dev_encode_chunked(engine, c.data, c.mn, c.avg, c.mx, 1, True)
        assert busy.rc == 0 and busy.written == idle.written and (busy.all == idle.all).all() and (busy.off == idle.off).all()
        assert set(fl.live) == IF.BUSY["both"]
        fl.wait_all()

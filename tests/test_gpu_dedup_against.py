"""zk_dedup_index_*, zk_frame_keys[_dev], zk_dedup_against_dev and zk_encode_dedup_against_dev on the GPU (include/zeekstd_amd.h;
zeekstd_amd/csrc/zk_dedup_index.hip, zk_dedup_index.h): ids and fresh against the model of the rule (tests/helpers/dedup_against_model.py: a
dict from bytes to the smallest archive id, then the in-call dict) entry by entry on the generations the emulator tests share, under every
key width, from source pointers 0, 1, 3 and 7 bytes off a 256-byte boundary, with nothing written behind the arrays; the frame keys against
their numpy statement; generations appended on the plain and on the dictionary route against zk_encode_frame_list_dev on every fresh frame
alone, read back with zk_decode_frame_list_dev, into tight destinations, in passes and slices of 1 KiB; a candidate with a damaged checksum;
refused calls; the calls while decode batches are in flight; the kernel times; DedupStore."""
import ctypes as C

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import cdc_model as CM
from helpers import dedup_against_model as A
from helpers import dedup_model as M
from helpers import enc_dict_sim as S
from helpers import in_flight as IF
from helpers.dev_decode import dev as _dev

pytestmark = pytest.mark.gpu

GENS = A.generations()
POISON, GUARD = 0xA5, 4096
POISON32 = 0x5A5A5A5A
TOO_SMALL, ARG, TOO_MANY, CHECKSUM = -70, -2003, -1002, -22
MISALIGN = dict(zip(A.KEY_BITS, (1, 3, 7)))


def _i64(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).to(_dev())


def _u8(b, pad=0):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) + b"\0" * pad, np.uint8).copy()).to(_dev()) if len(b) + pad else torch.zeros(1, dtype=torch.uint8, device=_dev())


def _put(c, misalign=0):
    import torch
    t = torch.zeros(max(len(c.buf) + misalign, 1), dtype=torch.uint8, device=_dev())
    if len(c.buf):
        t[misalign:] = torch.from_numpy(c.buf.copy()).to(_dev())
    return t, t.data_ptr() + misalign, _i64(c.off)


def _poisoned(n):
    import torch
    return torch.full((n + 8,), POISON32, dtype=torch.int32, device=_dev())


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


class Arch:
    """an archive as a caller keeps it: the payload and its prefix sums (host copies, uploaded for every call), the decoded frames for the
    model, and the index"""

    def __init__(self, engine, bits=0):
        try:
            engine.set_kernel_choice(dedup_key_bits=bits)
            self.index = zk.DedupIndex(engine)
        finally:
            engine.set_kernel_choice(dedup_key_bits=0)
        self.comp, self.c_off, self.d_off, self.frames = b"", [0], [0], []

    n_frames = property(lambda self: len(self.c_off) - 1)

    def dev(self):
        return _u8(self.comp, 64), len(self.comp), _i64(self.c_off), _i64(self.d_off), self.n_frames

    def grow(self, payload, c_sizes, contents):
        self.comp += payload
        for cs, f in zip(c_sizes, contents):
            self.c_off.append(self.c_off[-1] + int(cs))
            self.d_off.append(self.d_off[-1] + len(f))
            self.frames.append(bytes(f))

    def close(self):
        self.index.close()


class R:
    pass


def dev_against(engine, arch, c, bits=0, misalign=0, pass_kib=0, n_frames=None, off=None, count=None):
    import torch
    t, p, d_off = _put(c, misalign)
    if off is not None:
        d_off = _i64(off)
    count = c.count if count is None else count
    ids, fresh = _poisoned(c.count), _poisoned(c.count)
    nf = C.c_uint32(12345)
    d_comp, comp_size, d_c, d_d, n = arch.dev()
    torch.cuda.synchronize()
    try:
        engine.set_kernel_choice(dedup_key_bits=bits, dedup_pass_kib=pass_kib)
        rc = zk.lib.zk_dedup_against_dev(engine._h, arch.index._h, d_comp.data_ptr(), comp_size, d_c.data_ptr(), d_d.data_ptr(), n if n_frames is None else n_frames,
                                         p, d_off.data_ptr(), count, ids.data_ptr(), fresh.data_ptr(), C.byref(nf), None)
    finally:
        engine.set_kernel_choice(dedup_key_bits=0, dedup_pass_kib=0)
    torch.cuda.synchronize()
    return rc, nf.value, _np32(ids), _np32(fresh)


def assert_against(c, want, nf, ids, fresh):
    want_ids, want_fresh = want
    assert nf == len(want_fresh), (nf, len(want_fresh))
    for name, got, w in (("ids", ids, want_ids), ("fresh", fresh, want_fresh)):
        bad = np.nonzero(got[:len(w)] != w)[0]
        assert bad.size == 0, (name, int(bad[0]), int(got[bad[0]]), int(w[bad[0]]))
        assert (got[len(w):] == POISON32).all(), name


def dev_append(engine, arch, c, level=1, cdict=None, dst_cap=None, bits=0, misalign=0, pass_kib=0, slice_kib=0, keep=True, comp=None):
    """zk_encode_dedup_against_dev with poisoned outputs; on success (and keep) the archive grows by the fresh frames"""
    import torch
    n = int(c.off[-1] - c.off[0])
    bound = int(zk.lib.zk_compress_bound_list(n, c.count, int(cdict is not None)))
    cap = bound if dst_cap is None else dst_cap
    t, p, d_off = _put(c, misalign)
    dst = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    ids, fresh, cs, ds = (_poisoned(c.count) for _ in range(4))
    d_comp, comp_size, d_c, d_d, nfr = arch.dev()
    if comp is not None:
        d_comp = _u8(comp, 64)
    torch.cuda.synchronize()
    r = R()
    r.rc, r.n_fresh, r.written, r.bound = 0, 0, 0, bound
    try:
        engine.set_kernel_choice(dedup_key_bits=bits, dedup_pass_kib=pass_kib, dedup_slice_kib=slice_kib)
        r.n_fresh, r.written = engine.encode_dedup_against_dev(arch.index, d_comp, comp_size, d_c, d_d, nfr, p, d_off, c.count, level, True, dst, cap, ids, fresh, cs, ds,
                                                               dictionary=cdict)
    except zk.ZkError as ex:
        r.rc = ex.code
    finally:
        engine.set_kernel_choice(dedup_key_bits=0, dedup_pass_kib=0, dedup_slice_kib=0)
    torch.cuda.synchronize()
    r.all = dst.cpu().numpy()
    r.ids, r.fresh, r.c_sizes, r.d_sizes = (_np32(x) for x in (ids, fresh, cs, ds))
    if r.rc == 0 and keep:
        arch.grow(r.all[:r.written].tobytes(), r.c_sizes[:r.n_fresh], [c.frames[int(j)] for j in r.fresh[:r.n_fresh]])
    return r


def untouched(r):
    return (r.all == POISON).all() and all((a == POISON32).all() for a in (r.ids, r.fresh, r.c_sizes, r.d_sizes))


def encode_alone(engine, frame, level, cdict=None):
    """zk_encode_frame_list_dev on one frame -> its bytes"""
    import torch
    cap = int(zk.lib.zk_compress_bound_list(len(frame), 1, int(cdict is not None)))
    dst = torch.zeros(cap + 64, dtype=torch.uint8, device=_dev())
    wr = engine.encode_frame_list_dev(_u8(frame, 1), _i64([0, len(frame)]), 1, level, True, dst, cap, None, None, dictionary=cdict)
    torch.cuda.synchronize()
    return dst[:wr].cpu().numpy().tobytes()


def read_back(engine, arch, ids, c):
    import torch
    n = int(c.off[-1] - c.off[0])
    d_comp, comp_size, d_c, d_d, _ = arch.dev()
    dst = torch.full((n + 64,), POISON, dtype=torch.uint8, device=_dev())
    status = torch.full((c.count,), -1, dtype=torch.int32, device=_dev())
    rc = engine.decode_frame_list_dev(d_comp, comp_size, d_c, d_d, torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).to(_dev()), _i64(c.off - c.off[0]),
                                      c.count, dst, n, True, status)
    torch.cuda.synchronize()
    assert rc == 0 and not status.cpu().numpy().any()
    out = dst.cpu().numpy()
    assert (out[n:] == POISON).all()
    return out[:n].tobytes()


@pytest.mark.parametrize("bits", A.KEY_BITS)
@pytest.mark.parametrize("name", list(GENS))
def test_map_equals_the_model(engine, name, bits):
    """every generation against the archive so far, then appended: zk_dedup_against_dev and zk_encode_dedup_against_dev give the model's ids
    and fresh under every key width, nothing written behind the arrays; the index grows by the fresh frames and holds their keys"""
    arch = Arch(engine, bits)
    try:
        for g, c in enumerate(GENS[name]):
            want = A.model(arch.frames, c.frames)
            rc, nf, ids, fresh = dev_against(engine, arch, c, bits, MISALIGN[bits], pass_kib=g)
            assert rc == 0
            assert_against(c, want, nf, ids, fresh)
            assert arch.index.count == arch.n_frames                  # the map alone leaves the index as it was
            r = dev_append(engine, arch, c, bits=bits, misalign=(0, 1, 3, 7)[g])
            assert r.rc == 0
            assert_against(c, want, r.n_fresh, r.ids, r.fresh)
            assert r.d_sizes[:r.n_fresh].tolist() == [len(c.frames[int(j)]) for j in want[1]] and (r.d_sizes[r.n_fresh:] == POISON32).all()
            assert int(r.c_sizes[:r.n_fresh].sum()) == r.written and (r.c_sizes[r.n_fresh:] == POISON32).all() and (r.all[r.written:] == POISON).all()
            assert arch.index.count == arch.n_frames == len(arch.frames)
        keys, lens = arch.index.export()
        assert (keys == A.frame_keys(arch.frames)).all() and lens.tolist() == [len(f) for f in arch.frames]
        # the archive holds every frame of every generation now
        c = GENS[name][0]
        rc, nf, ids, fresh = dev_against(engine, arch, c, bits)
        assert rc == 0 and nf == 0
        assert_against(c, A.model(arch.frames, c.frames), nf, ids, fresh)
        assert read_back(engine, arch, ids[:c.count], c) == c.buf[c.lead:].tobytes()
    finally:
        arch.close()


def test_frame_keys_equal_the_numpy_statement(engine):
    import torch
    for name in ("enc_mix", "edges", "all_empty"):
        c = M.cases()[name]
        want = A.frame_keys(c.frames)
        assert (engine.frame_keys(c.buf, c.off) == want).all(), name
        for misalign in (0, 1, 3, 7):
            t, p, d_off = _put(c, misalign)
            keys = torch.full((c.count + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=_dev())
            torch.cuda.synchronize()
            engine.frame_keys_dev(p, d_off, c.count, keys)
            torch.cuda.synchronize()
            got = keys.cpu().numpy().view(np.uint64)
            assert (got[:c.count] == want).all() and (got[c.count:] == 0x5A5A5A5A5A5A5A5A).all(), (name, misalign)
    assert A.frame_key(b"") == 0 and len(engine.frame_keys(b"", [0])) == 0


def test_add_archive_dev_and_an_archive_with_duplicates(engine):
    """an index made by decoding the archive holds the keys the appending index exported, and answers alike -- also in passes of 1 KiB; an
    archive written WITHOUT dedup holds duplicate contents: the smallest archive frame wins"""
    arch = Arch(engine)
    other = Arch(engine, 4)
    try:
        for c in GENS["mix"]:
            assert dev_append(engine, arch, c).rc == 0
        d_comp, comp_size, d_c, d_d, n = arch.dev()
        engine.set_kernel_choice(dedup_pass_kib=1)
        try:
            other.index.add_archive_dev(d_comp, comp_size, d_c, d_d, 5)
            assert other.index.count == 5
            other.index.add_archive_dev(d_comp, comp_size, d_c, d_d, n)
        finally:
            engine.set_kernel_choice(dedup_pass_kib=0)
        assert other.index.count == n
        for a, b in zip(other.index.export(), arch.index.export()):
            assert (a == b).all()
        other.comp, other.c_off, other.d_off, other.frames = arch.comp, arch.c_off, arch.d_off, arch.frames
        c = GENS["near"][1]
        got = [dev_against(engine, x, c, bits) for x, bits in ((arch, 0), (other, 4))]
        assert got[0][0] == got[1][0] == 0 and got[0][1] == got[1][1] and (got[0][2] == got[1][2]).all() and (got[0][3] == got[1][3]).all()
        # duplicates: the list encoder writes every frame
        frames, c = A.dup_archive()
        import torch
        n_b = sum(len(f) for f in frames)
        cap = int(zk.lib.zk_compress_bound_list(n_b, len(frames), 0))
        dst = torch.zeros(cap + 64, dtype=torch.uint8, device=_dev())
        cs = torch.zeros(len(frames), dtype=torch.int32, device=_dev())
        off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
        wr = engine.encode_frame_list_dev(_u8(b"".join(frames), 1), _i64(off), len(frames), 1, True, dst, cap, cs, None)
        torch.cuda.synchronize()
        for bits in A.KEY_BITS:
            dup = Arch(engine, bits)
            try:
                dup.grow(dst[:wr].cpu().numpy().tobytes(), cs.cpu().numpy(), frames)
                d_comp, comp_size, d_c, d_d, n = dup.dev()
                dup.index.add_archive_dev(d_comp, comp_size, d_c, d_d, n)
                assert dup.index.count == len(frames)
                rc, nf, ids, fresh = dev_against(engine, dup, c, bits, 3)
                assert rc == 0
                assert_against(c, A.model(frames, c.frames), nf, ids, fresh)
            finally:
                dup.close()
    finally:
        arch.close()
        other.close()


@pytest.mark.parametrize("route", ["plain", "dictionary"])
def test_three_generations_appended(engine, route):
    """the output frames are zk_encode_frame_list_dev's on each fresh frame alone; a destination one byte short is -70 with nothing touched
    and the index as it was, one of exactly `written` bytes succeeds; passes and slices of 1 KiB give the same bytes; one
    zk_decode_frame_list_dev per generation over the final archive returns each source"""
    d = S.fixture_dicts()["trained"] if route == "dictionary" else None
    cdict = zk.EncodeDictionary(engine, zk.Dictionary(d)) if d else None
    arch = Arch(engine)
    try:
        if d:
            engine.set_dictionary(zk.Dictionary(d))                  # the verifying decode needs it: the caller's business
        kept = []
        for g, c in enumerate(GENS["mix"]):
            want_ids, want_fresh = A.model(arch.frames, c.frames)
            want = b"".join(encode_alone(engine, c.frames[int(j)], 1, cdict) for j in want_fresh)
            m = arch.index.count
            r = dev_append(engine, arch, c, cdict=cdict, dst_cap=len(want) - 1, slice_kib=g % 2)
            assert r.rc == TOO_SMALL and untouched(r) and arch.index.count == m == arch.n_frames
            r = dev_append(engine, arch, c, cdict=cdict, pass_kib=1, slice_kib=1, misalign=3, keep=False)
            assert r.rc == 0 and r.all[:r.written].tobytes() == want
            arch.index.truncate(m)                                    # an append the caller does not keep
            assert arch.index.count == m
            r = dev_append(engine, arch, c, cdict=cdict, dst_cap=len(want))
            assert r.rc == 0 and r.written == len(want) <= r.bound and r.all[:r.written].tobytes() == want and (r.all[r.written:] == POISON).all()
            assert_against(c, (want_ids, want_fresh), r.n_fresh, r.ids, r.fresh)
            assert arch.index.count == m + len(want_fresh) == arch.n_frames
            kept.append((c, want_ids))
        assert arch.n_frames < sum(c.count for c, _ in kept)
        for c, ids in kept:
            assert read_back(engine, arch, ids, c) == c.buf[c.lead:].tobytes()
    finally:
        engine.set_dictionary(None)
        arch.close()
        if cdict is not None:
            cdict.close()


def test_a_candidate_with_a_damaged_checksum(engine):
    """one flipped byte in the Content_Checksum of an archive frame the list holds: the checksum error, the arrays and the destination as
    they were, the index unchanged; a list that does not touch the frame is served"""
    arch = Arch(engine)
    try:
        c0, c1 = GENS["mix"][:2]
        assert dev_append(engine, arch, c0).rc == 0
        want = A.model(arch.frames, c1.frames)
        hit = int(want[0][want[0] < arch.n_frames].max())             # an archive frame the second generation holds
        assert len(arch.frames[hit]) > 0
        good = arch.comp
        bad = bytearray(good)
        bad[arch.c_off[hit + 1] - 2] ^= 0x10
        arch.comp = bytes(bad)
        m = arch.index.count
        rc, nf, ids, fresh = dev_against(engine, arch, c1)
        assert rc == CHECKSUM and nf == 0 and (ids == POISON32).all() and (fresh == POISON32).all() and arch.index.count == m
        r = dev_append(engine, arch, c1)
        assert r.rc == CHECKSUM and untouched(r) and arch.index.count == m
        miss = M.Case("miss", [f for f in c1.frames if f != arch.frames[hit]], lead=1)
        rc, nf, ids, fresh = dev_against(engine, arch, miss)
        assert rc == 0
        assert_against(miss, A.model(arch.frames, miss.frames), nf, ids, fresh)
        arch.comp = good
        rc, nf, ids, fresh = dev_against(engine, arch, c1)
        assert rc == 0
        assert_against(c1, want, nf, ids, fresh)
    finally:
        arch.close()


def test_refused_calls_write_nothing(engine):
    """a decreasing list, a frame above ZK_SEEKABLE_MAX_FRAME_SIZE, more frames than ZK_SEEKABLE_MAX_FRAMES, n_frames < m: the code, and the
    poisoned arrays, the destination and the index as they were"""
    import torch
    arch = Arch(engine)
    try:
        c = GENS["mix"][0]
        assert dev_append(engine, arch, c).rc == 0
        m = arch.index.count
        falling = c.off.copy()
        falling[5] = falling[4] - 1
        oversize = np.array([0, 10, 10 + 0x40000001, 20 + 0x40000001], np.uint64)
        t, p, _ = _put(c)
        d_comp, comp_size, d_c, d_d, n = arch.dev()
        dst = torch.full((1 << 16,), POISON, dtype=torch.uint8, device=_dev())
        for off, count, n_frames, want in ((falling, c.count, n, ARG), (oversize, 3, n, ARG), (c.off, 0x08000001, n, TOO_MANY), (c.off, c.count, m - 1, ARG)):
            d_off = _i64(off)
            arrs = [_poisoned(c.count) for _ in range(4)]
            nf, wr = C.c_uint32(12345), C.c_uint64(12345)
            torch.cuda.synchronize()
            rc = zk.lib.zk_dedup_against_dev(engine._h, arch.index._h, d_comp.data_ptr(), comp_size, d_c.data_ptr(), d_d.data_ptr(), n_frames, p, d_off.data_ptr(), count,
                                             arrs[0].data_ptr(), arrs[1].data_ptr(), C.byref(nf), None)
            assert rc == want and nf.value == 0
            nf = C.c_uint32(12345)
            rc = zk.lib.zk_encode_dedup_against_dev(engine._h, arch.index._h, d_comp.data_ptr(), comp_size, d_c.data_ptr(), d_d.data_ptr(), n_frames, p, d_off.data_ptr(),
                                                    count, 1, 1, None, dst.data_ptr(), 1 << 16, arrs[0].data_ptr(), arrs[1].data_ptr(), arrs[2].data_ptr(),
                                                    arrs[3].data_ptr(), C.byref(nf), C.byref(wr), None)
            torch.cuda.synchronize()
            assert rc == want and nf.value == 0 and wr.value == 12345 and arch.index.count == m
            assert all((_np32(a) == POISON32).all() for a in arrs) and (dst.cpu().numpy() == POISON).all()
        nf = C.c_uint32(7)
        assert zk.lib.zk_dedup_against_dev(engine._h, arch.index._h, None, 0, None, None, n, None, None, 0, None, None, C.byref(nf), None) == 0 and nf.value == 0
        assert zk.lib.zk_dedup_against_dev(engine._h, arch.index._h, d_comp.data_ptr(), comp_size, d_c.data_ptr(), d_d.data_ptr(), n, p, _i64(c.off).data_ptr(), c.count,
                                           None, None, None, None) == ARG
        assert engine.dedup_against_dev(arch.index, d_comp, comp_size, d_c, d_d, n, p, _i64(c.off), c.count) == 0      # NULL arrays: n_fresh alone
        d_comp2, comp_size2, d_c2, d_d2, _ = arch.dev()
        with pytest.raises(zk.ZkError):
            arch.index.add_archive_dev(d_comp2, comp_size2, d_c2, d_d2, m - 1)
        with pytest.raises(zk.ZkError):
            arch.index.truncate(m + 1)
        with pytest.raises(zk.ZkError):
            arch.index.export(m, 1)
        with pytest.raises(zk.ZkError):
            engine.set_kernel_choice(dedup_pass_kib=(1 << 22) + 1)
        assert arch.index.count == m
    finally:
        arch.close()


@pytest.mark.parametrize("state", IF.STATES)
def test_in_flight_rows(engine, state):
    """zk_dedup_against_dev, zk_encode_dedup_against_dev and zk_dedup_index_add_archive_dev take context 0: refused while it holds a batch, with
    everything as it was; served with the idle result otherwise.  The other index calls and zk_frame_keys* are served in every state"""
    import torch
    arch = Arch(engine)
    probe = Arch(engine)
    try:
        c0, c1 = GENS["mix"][:2]
        assert dev_append(engine, arch, c0).rc == 0
        m = arch.index.count
        idle = dev_against(engine, arch, c1)
        idle_enc = dev_append(engine, arch, c1, keep=False)
        arch.index.truncate(m)
        keys = A.frame_keys(c1.frames)
        assert idle[0] == 0 and idle_enc.rc == 0
        d_comp, comp_size, d_c, d_d, n = arch.dev()
        with IF.Flight(engine) as fl:
            fl.reach(state, IF.Staged(IF.long_()), IF.Staged(IF.long_()))
            busy = dev_against(engine, arch, c1)
            enc = dev_append(engine, arch, c1, keep=False)
            if 0 in IF.BUSY[state]:
                assert busy[0] == ARG and busy[1] == 12345 and (busy[2] == POISON32).all() and (busy[3] == POISON32).all()
                assert enc.rc == ARG and untouched(enc) and arch.index.count == m
                with pytest.raises(zk.ZkError):
                    probe.index.add_archive_dev(d_comp, comp_size, d_c, d_d, n)
                assert probe.index.count == 0
            else:
                assert busy[0] == 0 and busy[1] == idle[1] and (busy[2] == idle[2]).all() and (busy[3] == idle[3]).all()
                assert enc.rc == 0 and enc.written == idle_enc.written and (enc.all == idle_enc.all).all() and (enc.ids == idle_enc.ids).all()
                assert arch.index.count == m + enc.n_fresh
                probe.index.add_archive_dev(d_comp, comp_size, d_c, d_d, n)
                assert probe.index.count == n
            # served in every state
            arch.index.truncate(m)
            assert (engine.frame_keys(c1.buf, c1.off) == keys).all()
            t, p, d_off = _put(c1, 1)
            d_keys = torch.zeros(c1.count, dtype=torch.int64, device=_dev())
            engine.frame_keys_dev(p, d_off, c1.count, d_keys)
            assert (d_keys.cpu().numpy().view(np.uint64) == keys).all()
            k, s = arch.index.export()
            copy = zk.DedupIndex(engine)
            copy.add(k[:3], s[:3])
            copy.add_dev(_i64(k[3:]), torch.from_numpy(s[3:].view(np.int32).copy()).to(_dev()), len(k) - 3)
            assert copy.count == m and all((a == b).all() for a, b in zip(copy.export(), (k, s)))
            copy.close()
            assert set(fl.live) == IF.BUSY[state]
            fl.wait_all()
    finally:
        arch.close()
        probe.close()


def test_kernel_times_name_the_lookup(engine):
    arch = Arch(engine)
    try:
        c0, c1 = GENS["mix"][:2]
        assert dev_append(engine, arch, c0).rc == 0
        k, s = arch.index.export()
        zk.lib.zk_engine_set_profiling(engine._h, 1)
        try:
            rc = dev_against(engine, arch, c1)[0]
            times = engine.kernel_times()
            r = dev_append(engine, arch, c1, keep=False)
            enc_times = engine.kernel_times()
            copy = zk.DedupIndex(engine)
            copy.add(k, s)
            add_times = engine.kernel_times()
            copy.close()
        finally:
            zk.lib.zk_engine_set_profiling(engine._h, 0)
        assert rc == 0 and r.rc == 0
        names = {zk.lib.zk_engine_kernel_name(k).decode() for k in range(zk.lib.zk_engine_kernel_count())}
        assert {"zk_k_dxi_insert", "zk_k_dxi_lookup", "zk_k_dxi_compare", "zk_k_dxi_emit"} <= names
        assert {"zk_k_dedup_hash", "zk_k_dedup_insert", "zk_k_dxi_lookup", "zk_k_dxi_compare", "zk_k_dxi_emit", "zk_k_exec"} <= set(times), times
        assert {"zk_k_dedup_hash", "zk_k_dxi_lookup", "zk_k_dxi_compare", "zk_k_dxi_emit", "zk_k_enc_match"} <= set(enc_times), enc_times
        assert "zk_k_dxi_insert" in add_times, add_times
    finally:
        arch.close()


def test_dedup_store_appends_two_overlapping_texts(engine):
    rng = np.random.default_rng(11)
    paragraphs = [CM.word_text(300 + k, int(n)).tobytes() for k, n in enumerate(rng.integers(600, 3000, 16))]
    one = b"".join(paragraphs[int(k)] for k in rng.integers(0, 12, 40))
    two = b"".join(paragraphs[int(k)] for k in rng.integers(4, 16, 40))
    store = zk.DedupStore(engine, level=1)
    try:
        ids1, off1 = store.append(one, avg_size=256)
        n1 = store.n_frames
        ids2, off2 = store.append(two, avg_size=256)
        assert ids1.dtype == ids2.dtype == np.uint32 and store.index.count == store.n_frames
        assert n1 < len(ids1) and store.n_frames - n1 < len(ids2) and (ids2 < n1).any()       # the second text found chunks of the first
        print("chunks:", len(ids1), len(ids2), "stored:", n1, store.n_frames - n1, "payload:", store.comp_size, "of", len(one) + len(two))
        assert store.read(ids1, off1) == one and store.read(ids2, off2) == two
        n2 = store.n_frames
        ids3, off3 = store.append(one, offsets=off1)
        assert store.n_frames == n2 and (ids3 == ids1).all()         # nothing new: nothing stored
        assert store.append(b"", offsets=[0])[0].size == 0
    finally:
        store.close()

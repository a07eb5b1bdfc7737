"""zk_mark_frames_dev, zk_compact_archive_dev, zk_remap_ids_dev and zk_dedup_index_compact_dev on the GPU (include/zeekstd_amd.h;
zeekstd_amd/csrc/zk_compact.hip, zk_compact.h): the cases of tests/helpers/compact_model.py through the C ABI, out of place into a poisoned
destination with poisoned outputs and in place with slices of 1 KiB and the default, from buffers 0, 1, 3 and 7 bytes off a 256-byte boundary,
entry by entry and byte by byte against the numpy model; marks and renumbered ids; generations of real frames appended with
zk_encode_dedup_against_dev, two of them dropped, the archive compacted in place and the index with it, read back with
zk_decode_frame_list_dev and appended to again; every refusal with nothing written; the four calls while decode batches are in flight;
DedupStore.compact; one in-place call whose source offsets pass 2^32."""
import ctypes as C

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import compact_model as K
from helpers import dedup_against_model as A
from helpers import cdc_model as CM
from helpers import in_flight as IF
from helpers.dev_decode import dev as _dev

pytestmark = pytest.mark.gpu

CASES = K.cases()
GENS = A.generations()
POISON, GUARD = 0xA5, 4096
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
TOO_SMALL, ARG, TOO_MANY = -70, -2003, -1002
START = dict(zip(CASES, (K.STARTS * 8)))          # every case from one of the four starts; the edge cases from all of them (below)


def _i64(a, extra=0):
    import torch
    a = np.asarray(a, np.uint64)
    return torch.from_numpy(np.concatenate([a, np.full(extra, POISON64, np.uint64)]).view(np.int64).copy()).to(_dev())


def _i32(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).to(_dev())


def _u8(a):
    import torch
    a = np.asarray(a, np.uint8)
    return torch.from_numpy(a.copy()).to(_dev()) if len(a) else torch.zeros(1, dtype=torch.uint8, device=_dev())


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _np64(t):
    return t.cpu().numpy().view(np.uint64)


class R:
    pass


def dev_compact(engine, c, in_place, start=0, slice_kib=0, offsets_in_place=False, dst_cap=None, c_off=None, comp_size=None, n_frames=None, dst_shift=None):
    """one zk_compact_archive_dev call on the case: the buffer `start` bytes off a 256-byte boundary with a poisoned tail, the outputs poisoned
    behind what the call may write -> everything it left"""
    import torch
    n = c.n
    m = c.model()
    buf = torch.full((start + c.comp_size + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    if c.comp_size:
        buf[start:start + c.comp_size] = _u8(c.comp)
    d_c, d_d = _i64(c.c_off if c_off is None else c_off, 8), _i64(c.d_off, 8)
    live = _u8(c.live)
    cap = m["written"] if dst_cap is None else dst_cap
    dst = torch.full((start + max(m["written"], cap) + GUARD,), POISON, dtype=torch.uint8, device=_dev())
    c_out, d_out = (d_c, d_d) if offsets_in_place else (_i64([], n + 1 + 8), _i64([], n + 1 + 8))
    remap = _i32(np.full(n + 8, POISON32, np.uint32))
    nk, wr = C.c_uint32(12345), C.c_uint64(12345)
    p_src = buf.data_ptr() + start
    p_dst = p_src if in_place else dst.data_ptr() + start
    if dst_shift is not None:
        p_dst = p_src + dst_shift
    torch.cuda.synchronize()
    r = R()
    try:
        engine.set_kernel_choice(compact_slice_kib=slice_kib)
        r.rc = zk.lib.zk_compact_archive_dev(engine._h, p_src, c.comp_size if comp_size is None else comp_size, d_c.data_ptr(), d_d.data_ptr(), n if n_frames is None else n_frames,
                                             live.data_ptr(), p_dst, cap, c_out.data_ptr(), d_out.data_ptr(), remap.data_ptr(), C.byref(nk), C.byref(wr), None)
    finally:
        engine.set_kernel_choice(compact_slice_kib=0)
    torch.cuda.synchronize()
    r.n_kept, r.written = nk.value, wr.value
    r.buf, r.dst = buf.cpu().numpy(), dst.cpu().numpy()
    r.c_out, r.d_out, r.remap, r.c_in, r.d_in = _np64(c_out), _np64(d_out), _np32(remap), _np64(d_c), _np64(d_d)
    r.start, r.offsets_in_place = start, offsets_in_place
    return r


def assert_outputs(c, r, what):
    m = c.model()
    assert r.rc == 0 and r.n_kept == m["n_kept"] and r.written == m["written"], (what, r.rc, r.n_kept, r.written)
    nk = m["n_kept"]
    for name, got, want in (("remap", r.remap, m["remap"]), ("c_off_out", r.c_out, m["c_off_out"]), ("d_off_out", r.d_out, m["d_off_out"])):
        assert K.first_diff(got[:len(want)], want) is None, (what, name, K.first_diff(got[:len(want)], want))
    assert (r.remap[c.n:] == POISON32).all(), what                                   # nothing behind n_frames entries
    if not r.offsets_in_place:
        assert (r.c_out[nk + 1:] == POISON64).all() and (r.d_out[nk + 1:] == POISON64).all(), what     # nothing behind n_kept + 1 entries


def assert_out_of_place(c, r, what):
    assert_outputs(c, r, what)
    m = c.model()
    base, s = int(c.c_off[0]), r.start
    assert (r.dst[:s + base] == POISON).all(), (what, "before c_off[0]")
    bad = K.first_diff(r.dst[s + base:s + m["written"]], m["dst"])
    assert bad is None, (what, bad)
    assert (r.dst[s + m["written"]:] == POISON).all(), (what, "behind written")
    assert (r.buf[s:s + c.comp_size] == c.comp).all() and (r.buf[:s] == POISON).all() and (r.buf[s + c.comp_size:] == POISON).all(), (what, "the source")


def assert_in_place(c, r, what):
    assert_outputs(c, r, what)
    s = r.start
    # bytes before the first removed frame and at or beyond written as they were, the kept frames between
    bad = K.first_diff(r.buf[s:s + c.comp_size], c.expect_in_place())
    assert bad is None, (what, bad, c.first_removed(), c.model()["written"])
    assert (r.buf[:s] == POISON).all() and (r.buf[s + c.comp_size:] == POISON).all(), (what, "outside the buffer")


def untouched(c, r):
    s = r.start
    ok = (r.dst == POISON).all() and (r.buf[s:s + c.comp_size] == c.comp).all() and (r.buf[:s] == POISON).all() and (r.buf[s + c.comp_size:] == POISON).all()
    return ok and (r.remap == POISON32).all() and (r.c_out == POISON64).all() and (r.d_out == POISON64).all()


@pytest.mark.parametrize("name", list(CASES))
def test_out_of_place_equals_the_model(engine, name):
    c = CASES[name]
    for start in (K.STARTS if name.startswith("sizes_edges") else (START[name],)):
        assert_out_of_place(c, dev_compact(engine, c, False, start), (name, start))


@pytest.mark.parametrize("name", list(CASES))
def test_in_place_equals_the_model(engine, name):
    """slices of 1 KiB (steps of one tile, direct and staged) and the default give the model's bytes; the offset arrays updated in place"""
    c = CASES[name]
    starts = K.STARTS if name.startswith("sizes_edges") else (START[name],)
    for start in starts:
        one = dev_compact(engine, c, True, start, slice_kib=1)
        assert_in_place(c, one, (name, start, "1 KiB"))
        whole = dev_compact(engine, c, True, start, slice_kib=0, offsets_in_place=True)
        assert_in_place(c, whole, (name, start, "default"))
        assert (one.buf == whole.buf).all()
    m = c.model()
    nk = m["n_kept"]
    assert (whole.c_in[:nk + 1] == m["c_off_out"]).all() and (whole.d_in[:nk + 1] == m["d_off_out"]).all()
    assert (whole.c_in[nk + 1:c.n + 1] == c.c_off[nk + 1:]).all() and (whole.c_in[c.n + 1:] == POISON64).all()


def test_mark_frames(engine):
    import torch
    n = 300
    live = torch.zeros(n + 8, dtype=torch.uint8, device=_dev())
    live[n:] = POISON
    a, b = _i32([5, 7, 7, 299, 0, 5]), _i32([8, 7, 100])
    torch.cuda.synchronize()
    engine.mark_frames_dev(a, 6, n, live)
    engine.mark_frames_dev(b, 3, n, live)                                            # marks accumulate, repeated ids
    got = live.cpu().numpy()
    assert np.nonzero(got[:n])[0].tolist() == [0, 5, 7, 8, 100, 299] and set(got[:n].tolist()) == {0, 1} and (got[n:] == POISON).all()
    bad = _i32([3, n, 4])
    assert zk.lib.zk_mark_frames_dev(engine._h, bad.data_ptr(), 3, n, live.data_ptr(), None) == ARG
    torch.cuda.synchronize()
    assert (live.cpu().numpy() == got).all()                                         # an id equal to n_frames: live untouched
    assert zk.lib.zk_mark_frames_dev(engine._h, None, 0, n, None, None) == 0


def test_remap_ids(engine):
    import torch
    c = CASES["random_10"]
    m = c.model()
    kept = np.nonzero(c.live)[0].astype(np.uint32)
    gone = np.nonzero(c.live == 0)[0].astype(np.uint32)
    rng = np.random.default_rng(3)
    ids = kept[rng.integers(0, len(kept), 1000)]
    d_remap, d_ids = _i32(m["remap"]), _i32(ids)
    out = _i32(np.full(len(ids) + 8, POISON32, np.uint32))
    torch.cuda.synchronize()
    engine.remap_ids_dev(d_remap, c.n, d_ids, len(ids), out)
    got = _np32(out)
    assert (got[:len(ids)] == m["remap"][ids]).all() and (got[len(ids):] == POISON32).all()
    engine.remap_ids_dev(d_remap, c.n, d_ids, len(ids))                              # in place
    assert (_np32(d_ids) == m["remap"][ids]).all()
    for wrong in (int(gone[0]), c.n, 0xFFFFFFFF):
        w = ids.copy()
        w[500] = wrong
        d_w = _i32(w)
        out = _i32(np.full(len(ids), POISON32, np.uint32))
        torch.cuda.synchronize()
        assert zk.lib.zk_remap_ids_dev(engine._h, d_remap.data_ptr(), c.n, d_w.data_ptr(), len(w), out.data_ptr(), None) == ARG
        assert zk.lib.zk_remap_ids_dev(engine._h, d_remap.data_ptr(), c.n, d_w.data_ptr(), len(w), d_w.data_ptr(), None) == ARG
        torch.cuda.synchronize()
        assert (_np32(out) == POISON32).all() and (_np32(d_w) == w).all()
    assert zk.lib.zk_remap_ids_dev(engine._h, None, c.n, None, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------ real frames
class Arch:
    """an archive as a caller keeps it: the payload and its prefix sums on the host, the decoded frames for the model, and the index"""

    def __init__(self, engine, bits=0):
        try:
            engine.set_kernel_choice(dedup_key_bits=bits)
            self.index = zk.DedupIndex(engine)
        finally:
            engine.set_kernel_choice(dedup_key_bits=0)
        self.bits = bits
        self.comp, self.c_off, self.d_off, self.frames = np.zeros(0, np.uint8), [0], [0], []

    n_frames = property(lambda self: len(self.c_off) - 1)

    def dev(self):
        return _u8(np.concatenate([self.comp, np.zeros(64, np.uint8)])), len(self.comp), _i64(self.c_off), _i64(self.d_off), self.n_frames

    def against(self, engine, c):
        import torch
        src, d_off = _u8(c.buf), _i64(c.off)
        ids, fresh = _i32(np.full(c.count, POISON32, np.uint32)), _i32(np.full(c.count, POISON32, np.uint32))
        d_comp, comp_size, d_c, d_d, n = self.dev()
        torch.cuda.synchronize()
        try:
            engine.set_kernel_choice(dedup_key_bits=self.bits)
            nf = engine.dedup_against_dev(self.index, d_comp, comp_size, d_c, d_d, n, src, d_off, c.count, ids, fresh)
        finally:
            engine.set_kernel_choice(dedup_key_bits=0)
        return _np32(ids), _np32(fresh)[:nf]

    def append(self, engine, c):
        import torch
        nb = int(c.off[-1] - c.off[0])
        bound = int(zk.lib.zk_compress_bound_list(nb, c.count, 0))
        src, d_off = _u8(c.buf), _i64(c.off)
        dst = torch.zeros(bound + 64, dtype=torch.uint8, device=_dev())
        ids, fresh, cs, ds = (_i32(np.full(c.count, POISON32, np.uint32)) for _ in range(4))
        d_comp, comp_size, d_c, d_d, n = self.dev()
        torch.cuda.synchronize()
        try:
            engine.set_kernel_choice(dedup_key_bits=self.bits)
            nf, wr = engine.encode_dedup_against_dev(self.index, d_comp, comp_size, d_c, d_d, n, src, d_off, c.count, 1, True, dst, bound,
                                                     ids, fresh, cs, ds)
        finally:
            engine.set_kernel_choice(dedup_key_bits=0)
        self.comp = np.concatenate([self.comp, dst[:wr].cpu().numpy()])
        for k in range(nf):
            self.c_off.append(self.c_off[-1] + int(_np32(cs)[k]))
            self.d_off.append(self.d_off[-1] + int(_np32(ds)[k]))
            self.frames.append(bytes(c.frames[int(_np32(fresh)[k])]))
        return _np32(ids).copy()

    def read(self, engine, ids, c):
        import torch
        n = int(c.off[-1] - c.off[0])
        d_comp, comp_size, d_c, d_d, _ = self.dev()
        dst = torch.full((n + 64,), POISON, dtype=torch.uint8, device=_dev())
        status = torch.full((c.count,), -1, dtype=torch.int32, device=_dev())
        rc = engine.decode_frame_list_dev(d_comp, comp_size, d_c, d_d, _i32(ids), _i64(c.off - c.off[0]), c.count, dst, n, True, status)
        torch.cuda.synchronize()
        assert rc == 0 and not status.cpu().numpy().any()
        return dst[:n].cpu().numpy().tobytes()

    def close(self):
        self.index.close()


@pytest.mark.parametrize("bits", A.KEY_BITS)
def test_generations_dropped_and_the_archive_compacted(engine, bits):
    """three generations appended, the first and the third dropped: the archive compacted in place decodes the kept generation with its
    renumbered ids (checksums verified); the index compacted exports the kept frames' keys and lengths, answers a new generation as the
    model does over the kept frames, takes a further append, and an index rebuilt by add from the export answers the same"""
    import torch
    gens = GENS["mix"]
    arch = Arch(engine, bits)
    rebuilt = None
    try:
        ids = [arch.append(engine, c) for c in gens]
        n = arch.n_frames
        keep = [1]
        d_comp, comp_size, d_c, d_d, _ = arch.dev()
        live = torch.zeros(n, dtype=torch.uint8, device=_dev())
        remap = _i32(np.full(n, POISON32, np.uint32))
        d_ids = {g: _i32(ids[g]) for g in keep}
        torch.cuda.synchronize()
        for g in keep:
            engine.mark_frames_dev(d_ids[g], len(ids[g]), n, live)
        lv = live.cpu().numpy()
        assert set(np.nonzero(lv)[0].tolist()) == set(int(i) for g in keep for i in ids[g]) and 0 < lv.sum() < n
        m = K.model(arch.comp, np.array(arch.c_off, np.uint64), np.array(arch.d_off, np.uint64), lv)
        nk, wr = engine.compact_archive_dev(d_comp, comp_size, d_c, d_d, n, live, d_comp, comp_size, d_c, d_d, remap)
        assert nk == m["n_kept"] and wr == m["written"] and (_np32(remap) == m["remap"]).all()
        got = d_comp.cpu().numpy()
        assert (got[:wr] == m["dst"]).all() and (got[wr:comp_size] == arch.comp[wr:]).all()
        assert (_np64(d_c)[:nk + 1] == m["c_off_out"]).all() and (_np64(d_d)[:nk + 1] == m["d_off_out"]).all()
        for g in keep:
            engine.remap_ids_dev(remap, n, d_ids[g], len(ids[g]))
        arch.index.compact_dev(remap, n)
        # the caller's view of the compacted archive
        kept = np.nonzero(lv)[0]
        arch.comp, arch.c_off, arch.d_off = got[:wr].copy(), [int(x) for x in m["c_off_out"]], [int(x) for x in m["d_off_out"]]
        arch.frames = [arch.frames[int(s)] for s in kept]
        for g in keep:
            new_ids = _np32(d_ids[g])
            assert (new_ids == m["remap"][ids[g]]).all()
            assert arch.read(engine, new_ids, gens[g]) == gens[g].buf[gens[g].lead:].tobytes()
        assert arch.index.count == nk == arch.n_frames
        k, s = arch.index.export()
        assert (k == A.frame_keys(arch.frames)).all() and s.tolist() == [len(f) for f in arch.frames]
        rebuilt = Arch(engine, bits)
        rebuilt.index.add(k, s)
        rebuilt.comp, rebuilt.c_off, rebuilt.d_off, rebuilt.frames = arch.comp, arch.c_off, arch.d_off, arch.frames
        # a new generation -- the dropped first one -- against the kept frames
        want = A.model(arch.frames, gens[0].frames)
        for x in (arch, rebuilt):
            got_ids, got_fresh = x.against(engine, gens[0])
            assert (got_ids == want[0]).all() and (got_fresh == want[1]).all()
        assert 0 < len(want[1]) and (want[0] < nk).any()
        # ... appended (the table takes the fresh frames), then the third against all of it
        assert (arch.append(engine, gens[0]) == want[0]).all() and arch.index.count == arch.n_frames == nk + len(want[1])
        want = A.model(arch.frames, gens[2].frames)
        got_ids, got_fresh = arch.against(engine, gens[2])
        assert (got_ids == want[0]).all() and (got_fresh == want[1]).all()
        assert arch.read(engine, arch.append(engine, gens[2]), gens[2]) == gens[2].buf[gens[2].lead:].tobytes()
    finally:
        arch.close()
        if rebuilt is not None:
            rebuilt.close()


def test_refusals_write_nothing(engine):
    import torch
    c = CASES["alternating"]
    m = c.model()
    # -70: *written is the size that is needed
    r = dev_compact(engine, c, False, 1, dst_cap=m["written"] - 1)
    assert r.rc == TOO_SMALL and r.n_kept == 0 and r.written == m["written"] and untouched(c, r)
    # a partial overlap of d_dst and d_comp
    for shift in (16, c.comp_size + 7):
        r = dev_compact(engine, c, False, 0, dst_shift=shift)
        assert r.rc == ARG and r.n_kept == 0 and r.written == 0 and untouched(c, r), shift
    # decreasing offsets; c_off[n] > comp_size (out of place and in place); too many frames
    falling = c.c_off.copy()
    falling[200] = falling[199] - 1
    for in_place in (False, True):
        r = dev_compact(engine, c, in_place, 3, c_off=falling)
        assert r.rc == ARG and r.n_kept == 0 and r.written == 0 and untouched(c, r)
        r = dev_compact(engine, c, in_place, 3, comp_size=c.comp_size - 1)
        assert r.rc == ARG and untouched(c, r)
        r = dev_compact(engine, c, in_place, 0, n_frames=0x08000001)
        assert r.rc == TOO_MANY and untouched(c, r)
    # NULL live or destination; no frames
    d_c, d_d, buf = _i64(c.c_off), _i64(c.d_off), _u8(np.concatenate([c.comp, np.zeros(8, np.uint8)]))
    live = _u8(c.live)
    nk, wr = C.c_uint32(7), C.c_uint64(7)
    torch.cuda.synchronize()
    f = zk.lib.zk_compact_archive_dev
    assert f(engine._h, buf.data_ptr(), c.comp_size, d_c.data_ptr(), d_d.data_ptr(), c.n, None, buf.data_ptr(), c.comp_size, None, None, None, C.byref(nk), C.byref(wr), None) == ARG
    assert f(engine._h, buf.data_ptr(), c.comp_size, d_c.data_ptr(), d_d.data_ptr(), c.n, live.data_ptr(), None, c.comp_size, None, None, None, C.byref(nk), C.byref(wr), None) == ARG
    assert nk.value == 0 and wr.value == 0
    base = CASES["sizes_edges_base"]
    assert f(engine._h, buf.data_ptr(), 0, _i64(base.c_off).data_ptr(), None, 0, None, buf.data_ptr(), 0, None, None, None, C.byref(nk), C.byref(wr), None) == 0
    assert nk.value == 0 and wr.value == int(base.c_off[0])
    assert f(engine._h, None, 0, None, None, 0, None, None, 0, None, None, None, C.byref(nk), C.byref(wr), None) == 0 and wr.value == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy()[:c.comp_size] == c.comp).all()
    # NULL outputs: the totals alone
    assert engine.compact_archive_dev(buf, c.comp_size, d_c, d_d, c.n, live, buf, c.comp_size) == (m["n_kept"], m["written"])
    # an index of another count, a remap that no compaction writes: the index as it was
    x = zk.DedupIndex(engine)
    try:
        frames = GENS["mix"][0].frames[:20]
        keys, lens = A.frame_keys(frames), np.array([len(fr) for fr in frames], np.uint32)
        x.add(keys, lens)
        remap = np.arange(20, dtype=np.uint32)
        remap[3] = K.REMOVED
        remap[4:] -= 1
        twisted = remap.copy()
        twisted[0], twisted[1] = 1, 0
        for bad, n in ((remap, 19), (np.concatenate([remap, [19]]), 21), (twisted, 20)):
            assert zk.lib.zk_dedup_index_compact_dev(x._h, _i32(bad).data_ptr(), n, None) == ARG
            k, s = x.export()
            assert x.count == 20 and (k == keys).all() and (s == lens).all()
        x.compact_dev(_i32(remap), 20)
        k, s = x.export()
        assert x.count == 19 and (k == np.delete(keys, 3)).all() and (s == np.delete(lens, 3)).all()
        with pytest.raises(zk.ZkError):
            engine.set_kernel_choice(compact_slice_kib=(1 << 22) + 1)
    finally:
        x.close()


@pytest.mark.parametrize("state", IF.STATES)
def test_in_flight_rows(engine, state):
    """the four calls are served while context 0, context 1 or both hold a submitted batch, on an archive the batches do not read, with the
    result they have with nothing in flight; the batches stay in flight and their verdicts are what they are alone (Flight)"""
    import torch
    c = CASES["sizes_edges"]
    m = c.model()
    kept = np.nonzero(c.live)[0].astype(np.uint32)
    frames = GENS["edges"][0].frames[:c.n]
    assert len(frames) == c.n
    keys, lens = A.frame_keys(frames), np.array([len(f) for f in frames], np.uint32)
    x = zk.DedupIndex(engine)
    try:
        x.add(keys, lens)
        with IF.Flight(engine) as fl:
            fl.reach(state, IF.Staged(IF.long_()), IF.Staged(IF.long_()))
            live = torch.zeros(c.n, dtype=torch.uint8, device=_dev())
            engine.mark_frames_dev(_i32(kept), len(kept), c.n, live)
            assert (live.cpu().numpy() == c.live).all()
            assert_out_of_place(c, dev_compact(engine, c, False, 3), state)
            assert_in_place(c, dev_compact(engine, c, True, 1, slice_kib=1), state)
            d_ids = _i32(kept)
            engine.remap_ids_dev(_i32(m["remap"]), c.n, d_ids, len(kept))
            assert (_np32(d_ids) == np.arange(len(kept))).all()
            x.compact_dev(_i32(m["remap"]), c.n)
            k, s = x.export()
            assert x.count == len(kept) and (k == keys[kept]).all() and (s == lens[kept]).all()
            assert set(fl.live) == IF.BUSY[state]
            fl.wait_all()
    finally:
        x.close()


def test_kernel_times_name_the_move(engine):
    c = CASES["sizes_edges"]
    zk.lib.zk_engine_set_profiling(engine._h, 1)
    try:
        r = dev_compact(engine, c, True, 0, slice_kib=1)
        times = engine.kernel_times()
    finally:
        zk.lib.zk_engine_set_profiling(engine._h, 0)
    assert r.rc == 0
    names = {zk.lib.zk_engine_kernel_name(k).decode() for k in range(zk.lib.zk_engine_kernel_count())}
    assert {"zk_k_cmp_mark", "zk_k_cmp_emit", "zk_k_cmp_move", "zk_k_cmp_remap_ids", "zk_k_cmp_take"} <= names
    assert {"zk_k_cmp_emit", "zk_k_cmp_move"} <= set(times), times


def test_dedup_store_compact(engine):
    """three appends of overlapping data, two kept: read() of the kept snapshots returns their bytes, comp_size shrank by exactly the removed
    frames' compressed sizes, and a later append of the dropped data stores it again"""
    rng = np.random.default_rng(17)
    paragraphs = [CM.word_text(500 + k, int(n)).tobytes() for k, n in enumerate(rng.integers(600, 3000, 20))]
    one = b"".join(paragraphs[int(k)] for k in rng.integers(0, 10, 40))
    two = b"".join(paragraphs[int(k)] for k in rng.integers(5, 15, 40))
    three = b"".join(paragraphs[int(k)] for k in rng.integers(10, 20, 40))
    store = zk.DedupStore(engine, level=1)
    try:
        (ids1, off1), (ids2, off2), (ids3, off3) = (store.append(t, avg_size=256) for t in (one, two, three))
        n, size = store.n_frames, store.comp_size
        c_sizes = np.diff(store._c_off)
        used = np.zeros(n, bool)
        used[ids2] = True
        used[ids3] = True
        assert 0 < (~used).sum() < n and (ids2 < store.index.count).all()
        new2, new3 = store.compact([ids2, ids3])
        assert store.n_frames == int(used.sum()) == store.index.count
        assert store.comp_size == size - int(c_sizes[~used].sum())
        assert (np.diff(store._c_off) == c_sizes[used]).all()
        assert store.read(new2, off2) == two and store.read(new3, off3) == three
        m = store.n_frames
        again, off = store.append(one, offsets=off1)
        assert store.n_frames > m and store.index.count == store.n_frames              # the dropped chunks are stored again
        assert store.read(again, off) == one and store.read(new2, off2) == two
        assert store.compact([]) == [] and store.n_frames == 0 and store.comp_size == 0 and store.index.count == 0
    finally:
        store.close()


def test_one_in_place_call_past_4gib(engine):
    """66 entries of 64 MiB, filled on the device; five removed, the first and one in the middle among them: the source offsets of the last
    kept entries lie above 2^32 (the destination reaches 61 * 64 MiB, just below it: removing the first entry, as asked, and four more of 66
    leaves no more).  The expectation is built on the device from slices and compared there."""
    import torch
    size, n = 64 << 20, 66
    gone = (0, 20, 33, 34, 65)
    ar = torch.arange(size // 8, dtype=torch.int64, device=_dev())
    base = ((ar * 0x1E3779B97F4A7C15) ^ (ar >> 7)).view(torch.uint8)                 # 64 MiB, 8 bytes per word
    del ar
    buf = torch.empty(n * size + 64, dtype=torch.uint8, device=_dev())
    for e in range(n):
        buf[e * size:(e + 1) * size] = base + (e * 37 & 0xFF)
    buf[n * size:] = POISON
    del base
    keep = [e for e in range(n) if e not in gone]
    want = torch.cat([buf[e * size:(e + 1) * size] for e in keep])
    tail = buf[len(keep) * size:].clone()
    c_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
    live = np.ones(n, np.uint8)
    live[list(gone)] = 0
    d_c, d_d, remap = _i64(c_off), _i64(c_off * np.uint64(2)), _i32(np.zeros(n, np.uint32))
    d_live = _u8(live)
    torch.cuda.synchronize()
    nk, wr = engine.compact_archive_dev(buf, n * size, d_c, d_d, n, d_live, buf, n * size, d_c, d_d, remap)
    torch.cuda.synchronize()
    assert nk == len(keep) and wr == len(keep) * size and int(c_off[keep[-1]]) >= 1 << 32          # the last kept entry's source bytes lie at and above 2^32
    assert torch.equal(buf[:wr], want), "the kept entries"
    assert torch.equal(buf[wr:], tail), "at and beyond written"
    assert (_np64(d_c)[:nk + 1] == c_off[:nk + 1]).all() and (_np64(d_d)[:nk + 1] == 2 * c_off[:nk + 1]).all()
    assert (_np32(remap)[keep] == np.arange(nk)).all() and (_np32(remap)[list(gone)] == K.REMOVED).all()

"""zk_refine_entries[_dev] on the device, skippable-frame entries in every decode route, and decodes of refined tables, against the
pure-Python splitter and libzstd 1.5.7 of tests/helpers/entry_inputs.py.  Bit-exact: no tolerances anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import entry_inputs as EI
from helpers import in_flight as IF
from helpers.dev_decode import dev, upload
from helpers.in_flight import POISON, REFUSED, SLACK, STATES, Flight, Staged, minus_ones, poisoned, settle

pytestmark = pytest.mark.gpu

CASES = ["identity", "coarse", "skip_entries", "pzstd", "plain", "coarse63", "coarse64", "coarse65"]


@functools.lru_cache(maxsize=None)
def archive(name):
    if name.startswith("coarse") and name != "coarse":
        return EI.head(EI.coarse(), int(name[6:]))          # 63 / 64 / 65 entries: the split kernel's grid edge
    return next(mk for mk in EI.GOOD if mk.__name__ == name)()


@functools.lru_cache(maxsize=None)
def expected(name):
    return EI.refined(archive(name))


def t64(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).to(dev())


_UP = {}


def up(a):
    """the archive on the device, once: (bytes + padding, their count, c_off, d_off or None)"""
    if a.name not in _UP:
        u = upload(a.comp, a.c, a.d if a.d is not None else a.c)
        _UP[a.name] = (u[0], u[1], u[2], u[3] if a.d is not None else None)
    return _UP[a.name]


def refine_dev(engine, a, cap=None, fill=-1):
    """zk_refine_entries_dev into poisoned arrays of cap + 1 (+ 8 of slack) -> (rc, n_out, c_out, d_out, entry_of, status) as numpy"""
    import torch
    n = len(a.c) - 1
    u = up(a)
    if cap is None:
        rc, m = engine.refine_entries_dev(u[0], u[1], u[2], u[3], n, None, None, None, 0, minus_ones(n))
        assert rc == -70
        cap = m
    co, do = torch.full((cap + 9,), fill, dtype=torch.int64, device=dev()), torch.full((cap + 9,), fill, dtype=torch.int64, device=dev())
    eo, st = minus_ones(cap + 8), minus_ones(n)
    settle()
    rc, m = engine.refine_entries_dev(u[0], u[1], u[2], u[3], n, co, do, eo, cap, st)
    return rc, m, co.cpu().numpy().view(np.uint64), do.cpu().numpy().view(np.uint64), eo.cpu().numpy(), st.cpu().numpy()


def check_refined(a, r, rc, m, co, do, eo, st, cap):
    assert m == len(r.c) - 1
    assert np.array_equal(co[:m + 1], r.c) and np.array_equal(do[:m + 1], r.d) and np.array_equal(eo[:m].view(np.uint32), r.entry_of)
    assert (co[cap + 1:].view(np.int64) == -1).all() and (do[cap + 1:].view(np.int64) == -1).all() and (eo[cap:] == -1).all()    # nothing behind the arrays


# ------------------------------------------------------------------------------------------------ refine results
@pytest.mark.parametrize("name", CASES)
def test_refine_entries_dev_gives_the_python_splitters_table(engine, name):
    a, r = archive(name), expected(name)
    rc, m, co, do, eo, st = refine_dev(engine, a)
    assert rc == 0 and not st.any()
    check_refined(a, r, rc, m, co, do, eo, st, m)
    if name == "identity":
        assert np.array_equal(co[:m + 1], a.c) and np.array_equal(do[:m + 1], a.d)
    if name == "plain":
        assert do[0] == 0 and int(do[m]) == len(EI.plain_bytes(a))


@pytest.mark.parametrize("name", CASES)
def test_refine_entries_host_pointers(engine, name):
    a, r = archive(name), expected(name)
    co, do, eo, st = engine.refine_entries(a.comp, a.c, a.d)
    assert not st.any() and len(st) == len(a.c) - 1
    assert np.array_equal(co, r.c) and np.array_equal(do, r.d) and np.array_equal(eo, r.entry_of)


def test_refine_entries_of_a_slice_that_does_not_start_at_zero(engine):
    """host pointers: c_off[0] > 0 and d_off[0] > 0 -- the refined table continues both"""
    a, r = archive("coarse"), expected("coarse")
    lo, hi = 5, 23
    co, do, eo, st = engine.refine_entries(a.comp, a.c[lo:hi + 1], a.d[lo:hi + 1])
    j0, j1 = int(np.flatnonzero(r.entry_of == lo)[0]), int(np.flatnonzero(r.entry_of == hi - 1)[-1]) + 1
    assert not st.any() and np.array_equal(co, r.c[j0:j1 + 1]) and np.array_equal(do, r.d[j0:j1 + 1]) and np.array_equal(eo, r.entry_of[j0:j1] - lo)


def test_out_cap_one_short_is_dst_too_small_and_writes_nothing(engine):
    a, r = archive("skip_entries"), expected("skip_entries")
    m = len(r.c) - 1
    rc, got, co, do, eo, st = refine_dev(engine, a, cap=m - 1)
    assert rc == -70 and got == m and not st.any()          # *n_out is right, entry_status written
    assert (co.view(np.int64) == -1).all() and (do.view(np.int64) == -1).all() and (eo == -1).all()
    # out_cap = 0 with NULL outputs asks for the size
    u = up(a)
    st0 = minus_ones(len(a.c) - 1)
    rc, got = engine.refine_entries_dev(u[0], u[1], u[2], u[3], len(a.c) - 1, None, None, None, 0, st0)
    assert rc == -70 and got == m and not st0.cpu().numpy().any()
    # no entry: nothing to do
    rc, got = engine.refine_entries_dev(u[0], u[1], u[2], u[3], 0, None, None, None, 0, st0)
    assert rc == 0 and got == 0


# ------------------------------------------------------------------------------------------------ skippable entries, no refining
def one_frame_table(name):
    """the archive under the EXPECTED refined table (the helper's, not the engine's): every entry is one frame, skippable ones among them"""
    a, r = archive(name), expected(name)
    return a, r.c, r.d, EI.plain_bytes(a)


def test_skippable_entries_decode_through_decode_frames(engine):
    a, c, d, want = one_frame_table("skip_entries")
    assert (np.diff(d.astype(np.int64)) == 0).sum() >= 20
    out, st = engine.decode_frames(a.comp + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    assert not st.any() and out == want
    # ... and a batch of nothing but skippable frames: no block, no byte
    out, st = engine.decode_frames(a.comp + b"\0" * 8, c, d, first=0, count=20, raise_on_error=False)
    assert not st.any() and out == b"" and d[20] == 0


def dev_decode(engine, comp, c, d, first=0, count=None, verify=True):
    import torch
    count = len(c) - 1 - first if count is None else count
    total = int(d[first + count] - d[first])
    u = upload(comp, c, d)
    out, st = poisoned(total), minus_ones(count)
    settle()
    rc = engine.decode_frames_dev(u[0], u[1], u[2], u[3], first, count, out, total, verify, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == POISON).all(), "written behind the destination"
    return rc, got[:total].tobytes(), st.cpu().numpy()


def test_skippable_entries_decode_through_decode_frames_dev(engine):
    a, c, d, want = one_frame_table("skip_entries")
    rc, out, st = dev_decode(engine, a.comp, c, d)
    assert rc == 0 and not st.any() and out == want
    rc, out, st = dev_decode(engine, a.comp, c, d, 0, 20)
    assert rc == 0 and not st.any() and out == b""
    # a skippable entry whose table size is not 0, and one whose size field disagrees with the entry
    d2 = d.copy(); d2[5:] += np.uint64(3)
    rc, out, st = dev_decode(engine, a.comp, c, d2, 0, 20)
    assert rc == -20 and st.tolist() == [0] * 4 + [20] + [0] * 15
    c2 = c.copy(); c2[3] -= np.uint64(1)
    rc, out, st = dev_decode(engine, a.comp, c2, d, 0, 20)
    assert st[2] == 72 and st[3] != 0 and not st[4:].any()


# ------------------------------------------------------------------------------------------------ decoding the refined table
_REFINED = {}


def engine_refined(engine, name):
    """the ENGINE's refined table of an archive (held against the helper's by the tests above) and the whole stream's bytes under libzstd"""
    if name not in _REFINED:
        a = archive(name)
        co, do, eo, st = engine.refine_entries(a.comp, a.c, a.d)
        assert not st.any()
        want = EI.Z.decode_stream(a.comp, which=EI.JUDGE)
        assert want == EI.plain_bytes(a)
        _REFINED[name] = (a, co, do, want)
    return _REFINED[name]


@pytest.mark.parametrize("name", ["coarse", "pzstd", "plain"])
def test_refined_table_decodes_through_decode_frames_dev(engine, name):
    a, c, d, want = engine_refined(engine, name)
    rc, out, st = dev_decode(engine, a.comp, c, d)
    assert rc == 0 and not st.any() and out == want


def test_refined_table_decodes_through_a_frame_list_with_repeats(engine):
    import torch
    a, c, d, want = engine_refined(engine, "coarse")
    n = len(c) - 1
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.permutation(n)[:300], rng.integers(0, n, 60), np.flatnonzero(np.diff(d.astype(np.int64)) == 0)[:10]]).astype(np.uint32)
    sizes = (d[1:] - d[:-1])[ids]
    oo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    listed = b"".join(want[int(d[i]):int(d[i + 1])] for i in ids)
    u = upload(a.comp, c, d)
    out, st = poisoned(len(listed)), minus_ones(len(ids))
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(dev())
    settle()
    rc = engine.decode_frame_list_dev(u[0], u[1], u[2], u[3], d_ids, t64(oo), len(ids), out, len(listed), True, st)
    got = out.cpu().numpy()
    assert rc == 0 and not st.cpu().numpy().any() and got[:len(listed)].tobytes() == listed and (got[len(listed):] == POISON).all()


def test_refined_table_serves_ranges_across_refined_boundaries_and_zero_size_entries(engine):
    a, c, d, want = engine_refined(engine, "coarse")
    n, total = len(c) - 1, len(want)
    zero = np.flatnonzero(np.diff(d.astype(np.int64)) == 0)
    assert len(zero) >= 10
    at = [int(x) for x in d]
    offs = [at[int(z)] for z in zero[:10]] + [at[7] - 3, at[100] - 1, at[500], 0, total - 9, at[900] - 50]
    lens = [40] * 5 + [0] * 5 + [10, 2, at[520] - at[500] + 5, at[3] + 1, 9, 100]
    lens = [min(l, total - o) for o, l in zip(offs, lens)]
    out, st = engine.read_ranges(a.comp + b"\0" * 8, c, d, offs, lens, verify=True)
    assert not st.any()
    for o, l, got in zip(offs, lens, out):
        assert got == want[o:o + l], (o, l)
    import torch
    u = upload(a.comp, c, d)
    packed = b"".join(want[o:o + l] for o, l in zip(offs, lens))
    dst, dst_st = poisoned(len(packed)), minus_ones(len(offs))
    settle()
    rc = engine.read_ranges_dev(u[0], u[1], u[2], u[3], n, t64(offs), t64(lens), None, len(offs), dst, len(packed), True, dst_st)
    got = dst.cpu().numpy()
    assert rc == 0 and not dst_st.cpu().numpy().any() and got[:len(packed)].tobytes() == packed and (got[len(packed):] == POISON).all()


def test_refined_table_through_submit_and_wait_on_both_contexts(engine):
    a, c, d, want = engine_refined(engine, "coarse")
    n = len(c) - 1
    sizes = list(zip(np.diff(c.astype(np.int64)).tolist(), np.diff(d.astype(np.int64)).tolist()))
    b = IF._batch("refined_coarse", a.comp, sizes, [want[int(d[i]):int(d[i + 1])] for i in range(n)])
    with Flight(engine) as fl:
        s0 = fl.submit(b, 0, n // 2)
        s1 = fl.submit(b, n // 2, n - n // 2)
        assert {s0, s1} == {0, 1}
        for s in (s1, s0):
            rc, st = fl.wait(s)
            assert rc == 0 and not st.any()


def test_refined_table_through_the_host_pipeline_and_the_small_path(engine):
    a, c, d, want = engine_refined(engine, "coarse")
    n = len(c) - 1
    out, st = engine.decode_frames(a.comp + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    assert not st.any() and out == want
    # at most 64 entries from host pointers: the small path; a window with skippable, empty and ordinary entries
    sizes = np.diff(d.astype(np.int64))
    first = next(i for i in range(n - 64) if (sizes[i:i + 64] == 0).sum() >= 3 and (sizes[i:i + 64] > 0).sum() >= 30)
    try:
        for small in (0, 1, 2):                             # by shape (the small path), the general pipeline, the small path's two-kernel form
            engine.set_kernel_choice(small_path=small)
            out, st = engine.decode_frames(a.comp + b"\0" * 8, c, d, first=first, count=64, raise_on_error=False)
            assert not st.any() and out == want[int(d[first]):int(d[first + 64])], small
    finally:
        engine.set_kernel_choice(reset=0)


@functools.lru_cache(maxsize=None)
def mixed():
    """a batch that mixes skippable, empty and ordinary entries (some checksummed), one frame per entry"""
    a, c, d, want = one_frame_table("skip_entries")
    return a, c, d, want


@pytest.mark.parametrize("choice", [dict(exec_seg=2), dict(entropy=2), dict(xxh64=1), dict(xxh64=2), dict(xxh64=3), dict(xxh64=4), dict(xxh64=5),
                                    dict(exec_lanes=128), dict(exec_lanes=1024), dict(exec_seg=2, seg_fill=1), dict(exec_seg=2, seg_fill=2)],
                         ids=lambda c: ",".join("%s=%d" % kv for kv in c.items()))
def test_mixed_batch_under_pinned_kernels(engine, choice):
    a, c, d, want = mixed()
    try:
        engine.set_kernel_choice(reset=0)
        engine.set_kernel_choice(**choice)
        rc, out, st = dev_decode(engine, a.comp, c, d)
        assert rc == 0 and not st.any() and out == want
        if "small_path" not in choice:
            out, st = engine.decode_frames(a.comp + b"\0" * 8, c, d, raise_on_error=False)
            assert not st.any() and out == want
    finally:
        engine.set_kernel_choice(reset=0)


# ------------------------------------------------------------------------------------------------ damaged entries
def test_damaged_entries_stay_one_entry_and_fail_where_libzstd_refuses(engine):
    """DAMAGED (tests/helpers/entry_inputs.py): entry_status is nonzero wherever the structure alone decides (the Python splitter stops) and
    where the table's size disagrees with the frames', and only where libzstd refuses the entry too (or the format does: Refined.lax).  The
    size walk decodes no literals, so an entry whose damage sits there refines like a good one -- and its frame then fails when it is
    decoded.  Decoding the refined table fails exactly the entries libzstd refuses (+ lax ones) and delivers libzstd's bytes for the others."""
    a, what = EI.damaged()
    r = EI.refined(a)
    n = len(a.c) - 1
    rc, m, co, do, eo, st = refine_dev(engine, a)
    flagged = set(np.flatnonzero(st).tolist())
    structural = r.bad - r.bad_deep
    assert structural <= flagged, sorted(structural - flagged)
    assert flagged <= r.bad | r.lax, sorted(flagged - r.bad - r.lax)
    assert rc == (int(st[min(flagged)]) if flagged else 0) and rc < 0
    by_name = {w: e for e, w in what.items() if w != "flip"}
    for w in ("truncated", "junk1", "junk2", "junk3", "junk4", "junk9", "junk40", "skip_past", "skip_short"):
        assert st[by_name[w]] == -72, (w, int(st[by_name[w]]))
    assert st[by_name["size_wrong"]] == -20 and st[by_name["good"]] == 0
    # the refined table: a flagged entry is ONE entry with its own range and its size from d_off; the others as the helper says
    eo = eo[:m].view(np.uint32)
    assert np.array_equal(co[[0, m]], a.c[[0, n]]) and np.array_equal(do[[0, m]], a.d[[0, n]])
    for e in range(n):
        j = np.flatnonzero(eo == e)
        want_j = np.flatnonzero(r.entry_of == e)
        if e in flagged:
            assert len(j) == 1 and co[j[0]] == a.c[e] and co[j[0] + 1] == a.c[e + 1] and do[j[0]] == a.d[e] and do[j[0] + 1] == a.d[e + 1]
        elif e not in r.bad:
            assert np.array_equal(co[j], r.c[want_j]) and np.array_equal(do[j], r.d[want_j]), e
        else:                                               # damaged where only a full decode sees it: split like a good entry, inside its own range
            assert len(j) >= 1 and co[j[0]] == a.c[e] and co[j[-1] + 1] == a.c[e + 1] and do[j[0]] == a.d[e] and do[j[-1] + 1] == a.d[e + 1]
    # decode it: differential
    c2, d2 = co[:m + 1].copy(), do[:m + 1].copy()
    rc, out, dst = dev_decode(engine, a.comp, c2, d2, verify=True)
    failed = {int(eo[j]) for j in np.flatnonzero(dst)}
    assert failed >= r.bad and failed - r.bad <= r.lax, (sorted(r.bad - failed), sorted(failed - r.bad - r.lax))
    refused = [e for e, w in what.items() if w == "flip" and e in failed]
    assert len(refused) >= 20 and sum(1 for e, w in what.items() if w == "flip" and e not in failed) >= 20
    for e in range(n):
        if e not in failed:
            assert out[int(a.d[e]):int(a.d[e + 1])] == EI.entry_verdict(a, e), e


# ------------------------------------------------------------------------------------------------ Level B
def test_seek_table_refined_and_decoder_with_refine_entries(engine):
    from zeekstd_amd import api
    rng = np.random.default_rng(11)
    for name in ("coarse", "pzstd"):
        a, r = archive(name), expected(name)
        want = EI.plain_bytes(a)
        table = api.SeekTable.new()
        table.log_frames(np.diff(a.c.astype(np.int64)), np.diff(a.d.astype(np.int64)))
        fine = table.refined(engine, a.comp)
        fc, fd = fine.offsets()
        assert np.array_equal(fc, r.c) and np.array_equal(fd, r.d)
        dec = api.DecodeOptions(a.comp).engine(engine).seek_table(table).refine_entries(True).into_decoder()
        assert dec.seek_table() == fine
        for _ in range(12):
            off = int(rng.integers(0, len(want) - 1))
            ln = int(rng.integers(1, 5000))
            dec.set_offset_limit(len(want)); dec.set_offset(off); dec.set_offset_limit(min(len(want), off + ln))
            assert dec.read_to_end() == want[off:off + ln], (name, off, ln)
        dec.close()
        # without the flag such an archive is refused as before, where an entry holds more than one frame
        plain_dec = api.DecodeOptions(a.comp).engine(engine).seek_table(table).into_decoder()
        with pytest.raises(api.Error):
            plain_dec.read_to_end()
        plain_dec.close()


def test_a_short_read_inside_a_coarse_entry_costs_no_more_submissions_with_the_flag(engine):
    """the same short read inside the entry of COARSE that decodes to the most bytes, without the flag (one submission, which fails: the entry
    holds many frames) and with it (the frames the read touches)"""
    from zeekstd_amd import api
    a = archive("coarse")
    want = EI.plain_bytes(a)
    coarse = api.SeekTable.new()
    coarse.log_frames(np.diff(a.c.astype(np.int64)), np.diff(a.d.astype(np.int64)))
    e = int(np.argmax(np.diff(a.d.astype(np.int64))))
    assert len(a.pieces[e]) > 1
    off, ln = int(a.d[e]) + int(a.d[e + 1] - a.d[e]) // 2, 200
    cost = []
    for flag in (False, True):
        dec = api.DecodeOptions(a.comp).engine(engine).seek_table(coarse).refine_entries(flag).into_decoder()
        before = dec.gpu_submissions()
        dec.set_offset(off); dec.set_offset_limit(off + ln)
        if flag:
            assert dec.read_to_end() == want[off:off + ln]
        else:
            with pytest.raises(api.Error):
                dec.read_to_end()
        cost.append(dec.gpu_submissions() - before)
        dec.close()
    assert cost[0] >= 1 and cost[1] <= cost[0], cost


def test_a_plain_stream_gets_a_table_and_a_decoder_reads_it(engine):
    from zeekstd_amd import api
    a, r = archive("plain"), expected("plain")
    want = EI.plain_bytes(a)
    table = api.SeekTable.refined(engine, a.comp)
    c, d = table.offsets()
    assert table.num_frames() == 300 and np.array_equal(c, r.c) and np.array_equal(d, r.d)
    dec = api.DecodeOptions(a.comp).engine(engine).seek_table(table).into_decoder()
    assert dec.read_to_end() == want
    dec.set_offset(len(want) // 3); dec.set_offset_limit(len(want) // 3 + 777)
    assert dec.read_to_end() == want[len(want) // 3:len(want) // 3 + 777]
    dec.close()
    # a bad entry: its code, and the message
    with pytest.raises(api.Error) as ei:
        api.SeekTable.refined(engine, a.comp[:-3])
    assert ei.value.code == -72


# ------------------------------------------------------------------------------------------------ the in-flight row
@pytest.mark.parametrize("state", STATES)
def test_refine_entries_between_a_submit_and_its_wait(engine, state):
    """the row of the table above zk_decode_submit_dev: refused while context 0 holds a batch (a, c) -- outputs, *n_out and the batches as they
    were --, served beside a batch on context 1 (b)"""
    import zeekstd_amd as zk
    a, r = archive("skip_entries"), expected("skip_entries")
    n, m = len(a.c) - 1, len(r.c) - 1
    u = up(a)
    h_comp = np.frombuffer(a.comp + b"\0" * 8, np.uint8).copy()
    with Flight(engine) as fl:
        fl.reach(state, Staged(IF.small()), Staged(IF.small()))
        import torch
        co, do = torch.full((m + 9,), -1, dtype=torch.int64, device=dev()), torch.full((m + 9,), -1, dtype=torch.int64, device=dev())
        eo, st = minus_ones(m + 8), minus_ones(n)
        settle()
        n_out = C.c_uint32(7)
        rc = zk.lib.zk_refine_entries_dev(engine._h, u[0].data_ptr(), u[1], u[2].data_ptr(), u[3].data_ptr(), n, co.data_ptr(), do.data_ptr(), eo.data_ptr(),
                                          m, C.byref(n_out), st.data_ptr(), None)
        hco, hdo, heo, hst = np.full(m + 1, 5, np.uint64), np.full(m + 1, 5, np.uint64), np.full(m, 5, np.uint32), np.full(n, 5, np.int32)
        hn = C.c_uint32(7)
        hrc = zk.lib.zk_refine_entries(engine._h, h_comp.ctypes.data, len(a.comp), a.c.ctypes.data, a.d.ctypes.data, n, hco.ctypes.data, hdo.ctypes.data,
                                       heo.ctypes.data, m, C.byref(hn), hst.ctypes.data)
        if state == "ctx1":
            assert rc == 0 and n_out.value == m and hrc == 0 and hn.value == m
            assert np.array_equal(co.cpu().numpy().view(np.uint64)[:m + 1], r.c) and np.array_equal(do.cpu().numpy().view(np.uint64)[:m + 1], r.d)
            assert np.array_equal(eo.cpu().numpy()[:m].view(np.uint32), r.entry_of) and not st.cpu().numpy().any()
            assert np.array_equal(hco, r.c) and np.array_equal(hdo, r.d) and np.array_equal(heo, r.entry_of) and not hst.any()
        else:
            assert rc == REFUSED and hrc == REFUSED and n_out.value == 7 and hn.value == 7
            for t in (co, do, eo, st):
                assert (t.cpu().numpy() == -1).all()
            assert (hco == 5).all() and (hdo == 5).all() and (heo == 5).all() and (hst == 5).all()
        fl.wait_all()                                        # (the batches are checked: bytes, statuses, slack)

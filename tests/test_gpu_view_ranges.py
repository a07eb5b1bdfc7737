"""zk_read_view_ranges_dev / Engine.read_view_ranges_dev / DedupStore.read_ranges: byte ranges of a view (ids, offsets) of a device-resident
archive, against the model of tests/helpers/view_model.py.  The destination and the statuses are poisoned before every call and compared as a
whole: the ranges' bytes, and the poison everywhere else -- between the destinations and behind the last one."""
import numpy as np
import pytest

from helpers import dict_fixtures as df
from helpers import in_flight as F
from helpers import view_model as V
from oracle import zko

pytestmark = pytest.mark.gpu

POISON = V.POISON
TAIL = 257
ST_POISON = -12345


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev_u64(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64).copy()).to(dev)


def _dev_u32(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint32)).view(np.int32).copy()).to(dev)


class Arc:
    """an archive in HBM and what its frames decode to"""

    def __init__(self, comp, sizes, frames):
        torch, dev = _torch()
        self.comp = bytes(comp)
        self.c = np.concatenate([[0], np.cumsum([s[0] for s in sizes])]).astype(np.uint64)
        self.d = np.concatenate([[0], np.cumsum([s[1] for s in sizes])]).astype(np.uint64)
        self.n = len(sizes)
        self.frames = frames
        self.sizes = [len(f) for f in frames]
        assert self.sizes == [s[1] for s in sizes]
        self.d_comp = torch.from_numpy(np.frombuffer(self.comp + b"\0" * 64, np.uint8).copy()).to(dev)
        self.d_c, self.d_d = _dev_u64(self.c), _dev_u64(self.d)

    def damaged(self, flips):
        """a copy with bytes of the compressed stream XORed: {position: mask}"""
        comp = bytearray(self.comp)
        for at, mask in flips.items():
            comp[at] ^= mask
        return Arc(bytes(comp), list(zip(np.diff(self.c).tolist(), np.diff(self.d).tolist())), self.frames)


def make_arc(engine, sizes, seed, dictionary=None, data=None):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    data = zko.gen_chunks(int(off[-1]), seed) if data is None else data
    comp, fr = engine.encode_frame_list(data, off, 1, True, dictionary=dictionary)
    arr = np.frombuffer(data, np.uint8)
    return Arc(comp, fr, [arr[int(a):int(b)] for a, b in zip(off[:-1], off[1:])])


_ARCS = {}


def edge_arc(engine):
    """the frames of 0, 1, 15, 16, 17, 63, 64, 65, 4 095, 4 096, 65 535, 65 537 and 200 000 bytes and a dozen of 1-3 KiB, level 1, checksums"""
    if "edge" not in _ARCS:
        _ARCS["edge"] = make_arc(engine, V.edge_sizes(), 0x51E0)
    return _ARCS["edge"]


def call(engine, arc, ids, voff, ranges, given, cap, size, verify=True):
    """one zk_read_view_ranges_dev over a poisoned destination and poisoned statuses -> (rc, statuses, the destination, frames decoded)"""
    import zeekstd_amd as zk
    torch, dev = _torch()
    d_dst = torch.full((size,), POISON, dtype=torch.uint8, device=dev)
    d_st = torch.full((max(len(ranges), 1),), ST_POISON, dtype=torch.int32, device=dev)
    d_ids = _dev_u32(ids if len(ids) else [0])
    d_voff = _dev_u64(voff)
    d_o, d_l = _dev_u64([r[0] for r in ranges] or [0]), _dev_u64([r[1] for r in ranges] or [0])
    d_do = _dev_u64(given) if given is not None else None
    torch.cuda.synchronize()
    rc = zk.lib.zk_read_view_ranges_dev(engine._h, arc.d_comp.data_ptr(), len(arc.comp), arc.d_c.data_ptr(), arc.d_d.data_ptr(), arc.n, d_ids.data_ptr(),
                                        d_voff.data_ptr(), len(ids), d_o.data_ptr(), d_l.data_ptr(), d_do.data_ptr() if d_do is not None else None, len(ranges),
                                        d_dst.data_ptr(), cap, int(verify), d_st.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, d_st.cpu().numpy()[:len(ranges)], d_dst.cpu().numpy(), engine.ranges_frames_decoded()


def check(engine, arc, ids, voff, ranges, mode, what, dst_cap=None, frame_err=None, verify=True):
    """the call against the model: return value, statuses, every byte of the destination (but those of ranges that failed for a frame, which
    are nobody's promise) and the number of distinct frames decoded"""
    given, offs, end = V.destinations(ranges, mode, v0=int(voff[0]), vend=int(voff[-1]))
    cap = end if dst_cap is None else dst_cap
    size = max(end, cap) + TAIL
    want = V.model(arc.frames, ids, voff, [r[0] for r in ranges], [r[1] for r in ranges], given, cap, size, frame_err=frame_err)
    rc, st, got, decoded = call(engine, arc, ids, voff, ranges, given, cap, size, verify)
    assert rc == want["rc"], (what, mode, rc, want["rc"])
    if want["dst"] is None:
        assert (got == POISON).all() and (st == ST_POISON).all(), (what, "a refused view wrote")
        return want, got
    assert st.tolist() == want["status"].tolist(), (what, mode, V.first_diff(st, want["status"]))
    for at, n in want["unspecified"]:
        want["dst"][at:at + n] = got[at:at + n]
    bad = V.first_diff(got, want["dst"])
    if bad is not None:
        i = max((k for k, at in enumerate(offs) if at <= bad[0]), key=lambda k: offs[k], default=None)
        pytest.fail(f"{what}, {mode}: first wrong byte at {bad} of the destination (range {i}: {ranges[i] if i is not None else None} at {offs[i] if i is not None else None})")
    assert decoded == len(want["decoded"]), (what, decoded, len(want["decoded"]))
    return want, got


VIEW_NAMES = ["identity", "reversed", "thrice_in_a_row", "thrice_interleaved", "random_300", "subset", "single", "empty_runs", "based_12345"]


# ---- 1. every view, every range shape, packed and with shuffled destinations
@pytest.mark.parametrize("name", VIEW_NAMES)
@pytest.mark.parametrize("mode", ["packed", "shuffled"])
def test_views_against_the_model(engine, name, mode):
    arc = edge_arc(engine)
    ids, voff = V.views(arc.sizes)[name]
    check(engine, arc, ids, voff, V.ranges_of(voff, dense=len(ids) <= 120), mode, name)


def test_an_empty_view_and_an_empty_list(engine):
    arc = edge_arc(engine)
    want, _ = check(engine, arc, np.zeros(0, np.uint32), np.array([77], np.uint64), [(77, 0), (76, 0), (78, 0), (77, 1)], "packed", "empty view")
    assert want["status"].tolist() == [0, V.OUT_OF_RANGE, V.OUT_OF_RANGE, V.OUT_OF_RANGE]
    ids, voff = V.views(arc.sizes)["identity"]
    rc, st, got, _ = call(engine, arc, ids, voff, [], None, 0, TAIL)
    assert rc == 0 and (got == POISON).all() and (st == ST_POISON).all()


# ---- 2. the identity view is zk_read_ranges_dev
def test_identity_view_is_read_ranges(engine):
    torch, dev = _torch()
    arc = edge_arc(engine)
    ids, voff = V.views(arc.sizes)["identity"]
    total = int(voff[-1])
    ranges = V.ranges_of(voff) + [(total, 1), (total + 1, 0), (5, V.U64), (total - 10, 11)]
    for mode in ("packed", "shuffled"):
        given, offs, end = V.destinations(ranges, mode, vend=total)
        cap = end - 3                                            # the last destinations leave it
        rc, st, got, decoded = call(engine, arc, ids, voff, ranges, given, cap, end + TAIL)
        d_dst = torch.full((end + TAIL,), POISON, dtype=torch.uint8, device=dev)
        d_st = torch.full((len(ranges),), ST_POISON, dtype=torch.int32, device=dev)
        rc2 = engine.read_ranges_dev(arc.d_comp, len(arc.comp), arc.d_c, arc.d_d, arc.n, _dev_u64([r[0] for r in ranges]), _dev_u64([r[1] for r in ranges]),
                                     _dev_u64(given) if given is not None else None, len(ranges), d_dst, cap, True, d_st)
        torch.cuda.synchronize()
        assert rc == rc2 == next(int(x) for x in st if x)               # the first failing range in list order
        assert st.tolist() == d_st.cpu().numpy().tolist() and {V.DST_TOO_SMALL, V.OUT_OF_RANGE, 0} <= set(st.tolist())
        assert np.array_equal(got, d_dst.cpu().numpy())
        assert decoded == engine.ranges_frames_decoded() == sum(1 for n in arc.sizes if n)


# ---- 3. a frame is decoded once
def test_every_frame_is_decoded_once(engine):
    arc = edge_arc(engine)
    views = V.views(arc.sizes)
    rng = np.random.default_rng(0xD0CE)
    for name in ("thrice_in_a_row", "thrice_interleaved"):
        ids, voff = views[name]
        total = int(voff[-1])
        ranges = []
        for k in range(50):
            off = int(rng.integers(0, total))
            ranges.append((off, min(int(rng.integers(1, (2000, 90000)[k % 2])), total - off)))
        want, _ = check(engine, arc, ids, voff, ranges, "packed", name)
        assert 3 <= len(want["decoded"]) <= arc.n                 # (check() held the engine's count against it)
    f = arc.sizes.index(4096)
    ids = np.full(1000, f, np.uint32)
    voff = V.offsets_of(arc.sizes, ids)
    check(engine, arc, ids, voff, [(0, 1000 * 4096), (4095, 2), (999 * 4096, 4096), (123 * 4096 + 7, 3 * 4096)], "shuffled", "one frame a thousand times")
    assert engine.ranges_frames_decoded() == 1


# ---- 4. passes
def test_passes_over_the_scratch(engine):
    """40 frames of 64 KiB and a pass of 1 MiB: three passes, and under the interleaved view one range's entries fall into all of them"""
    if "t64k" not in _ARCS:
        _ARCS["t64k"] = make_arc(engine, [65536] * 40, 0x51E1)
    arc = _ARCS["t64k"]
    ids, voff = V.views(arc.sizes)["thrice_interleaved"]
    ranges = V.ranges_of(voff, dense=False)
    try:
        _, base = check(engine, arc, ids, voff, ranges, "shuffled", "default pass")
        assert engine.ranges_frames_decoded() == 40
        engine.set_kernel_choice(range_pass_mib=1)
        _, one = check(engine, arc, ids, voff, ranges, "shuffled", "1 MiB passes")
        assert engine.ranges_frames_decoded() == 40
        assert np.array_equal(base, one)
    finally:
        engine.set_kernel_choice(reset=0)


# ---- 5. 64-bit coordinates
def test_a_stream_past_4gib_without_the_memory_for_it(engine):
    if "two" not in _ARCS:
        _ARCS["two"] = make_arc(engine, [65536, 100, 3000], 0x51E2)
    arc = _ARCS["two"]
    ids = np.zeros(70000, np.uint32)
    ids[65534:65544] = [1, 0, 2, 0, 1, 1, 0, 2, 2, 0]
    voff = V.offsets_of(arc.sizes, ids)
    end, at = int(voff[-1]), 1 << 32
    assert end > 4_500_000_000 and int(voff[65534]) < at < int(voff[65544])
    ranges = [(at - 3000, 7000), (at - 1, 2), (at, 1), (at - 1, 1), (at - 70000, 140000), (end - 4000, 4000), (end - 1, 1), (end, 0), (int(voff[65534]) - 10, 300), (int(voff[65538]) - 1, 3300),
              (12345, 100000)]
    for mode in ("packed", "shuffled"):
        want, _ = check(engine, arc, ids, voff, ranges, mode, "4.6 GB stream")
        assert not want["status"].any() and len(want["decoded"]) == 3
    # a small view whose first offset lies just below 2^32
    e = edge_arc(engine)
    ids, _ = V.views(e.sizes)["subset"]
    voff = V.offsets_of(e.sizes, ids, at - 1000)
    ranges = [(at - 1000, 3000), (at - 1, 2), (at, 17), (int(voff[-1]) - 5, 5), (at - 1001, 1), (int(voff[0]), int(voff[-1] - voff[0])), (1000, 1)]
    want, _ = check(engine, e, ids, voff, ranges, "shuffled", "first offset below 2^32")
    assert want["status"].tolist() == [0, 0, 0, 0, V.OUT_OF_RANGE, 0, V.OUT_OF_RANGE]


# ---- 6. bad views
@pytest.mark.parametrize("kind", ["id", "size", "order"])
def test_bad_views_are_refused_whole(engine, kind):
    arc = edge_arc(engine)
    ids, voff = V.views(arc.sizes)["random_300"]
    ranges = [(int(voff[10]), int(voff[20] - voff[10])), (int(voff[100]) + 1, 5)]
    for j in (12, 250):                                          # an entry that a range touches, one that none touches
        i2, v2 = ids.copy(), voff.copy()
        if kind == "id":
            i2[j] = arc.n
        elif kind == "size":
            v2[j + 1:] += np.uint64(1)
        else:
            k = next(k for k in range(j, 300) if v2[k + 1] > v2[k])
            v2[k], v2[k + 1] = v2[k + 1], v2[k]
        for mode in ("packed", "shuffled"):
            want, _ = check(engine, arc, i2, v2, ranges, mode, (kind, j))
            assert want["rc"] == V.ARGUMENT
    check(engine, arc, ids, voff, ranges, "packed", "the view itself")


# ---- 7. bad ranges
def test_bad_ranges_get_their_code_and_neighbours_are_served(engine):
    arc = edge_arc(engine)
    ids, voff = V.views(arc.sizes)["based_12345"]
    v0, vend = int(voff[0]), int(voff[-1])
    good = V.ranges_of(voff, dense=False)[:40]
    bad = [(v0 - 1, 1), (0, 0), (vend, 1), (vend + 1, 0), (vend - 10, 11), (v0 + 5, V.U64), (V.U64, 2), (1 << 63, 1 << 63)]
    ranges = good[:15] + bad[:4] + good[15:] + bad[4:]
    for mode in ("packed", "shuffled"):
        want, _ = check(engine, arc, ids, voff, ranges, mode, "bad ranges")
        assert [int(s) for s in want["status"] if s] == [V.OUT_OF_RANGE] * len(bad) and want["rc"] == V.OUT_OF_RANGE
    given, offs, end = V.destinations(good, "shuffled", v0=v0, vend=vend)
    cap = sorted(offs)[-3] + 1
    want, _ = check(engine, arc, ids, voff, good, "shuffled", "dst_cap", dst_cap=cap)
    assert V.DST_TOO_SMALL in want["status"].tolist() and 0 in want["status"].tolist() and want["rc"] == next(int(s) for s in want["status"] if s)
    # packed: the capacity ends inside a range; everything behind it is cut as well
    _, poffs, pend = V.destinations(good, "packed", v0=v0, vend=vend)
    k = max(i for i, (_, n) in enumerate(good) if n > 1 and poffs[i] > 0)
    want, _ = check(engine, arc, ids, voff, good, "packed", "packed dst_cap", dst_cap=poffs[k] + good[k][1] - 1)
    assert want["status"][k] == V.DST_TOO_SMALL and want["status"][0] == 0


# ---- 8. damaged frames
def test_damaged_frames_fail_their_ranges_in_view_order(engine):
    torch, dev = _torch()
    good = edge_arc(engine)
    a, b = good.sizes.index(4095), good.sizes.index(65537)
    arc = good.damaged({(int(good.c[a]) + int(good.c[a + 1])) // 2: 0x10, int(good.c[b + 1]) - 1: 0x01})     # a's payload, b's checksum
    total = int(arc.d[-1])
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    d_fs = torch.zeros(arc.n, dtype=torch.int32, device=dev)
    engine.decode_frames_dev(arc.d_comp, len(arc.comp), arc.d_c, arc.d_d, 0, arc.n, d_out, total, True, d_fs)
    fst = d_fs.cpu().numpy()
    assert fst[a] != 0 and fst[b] != 0 and np.count_nonzero(fst) == 2
    err = {a: int(fst[a]), b: int(fst[b])}
    for name, order in (("a then b", [3, a, 5, b, 6, 7]), ("b then a", [3, b, 5, a, 6, 7])):
        ids = np.array(order, np.uint32)
        voff = V.offsets_of(arc.sizes, ids)
        ranges = [(0, int(voff[-1])), (int(voff[1]), 10), (int(voff[3]) + 5, 10), (0, int(voff[1])), (int(voff[4]), int(voff[6] - voff[4])), (int(voff[2]) - 1, 2)]
        want, _ = check(engine, arc, ids, voff, ranges, "shuffled", name, frame_err=err)
        first, second = (err[a], err[b]) if name == "a then b" else (err[b], err[a])
        assert want["status"].tolist() == [-first, -first, -second, 0, 0, -first] and want["rc"] == -first
    ids, voff = V.views(arc.sizes)["thrice_interleaved"]
    want, _ = check(engine, arc, ids, voff, V.ranges_of(voff, dense=False), "packed", "interleaved", frame_err=err)
    assert sum(1 for s in want["status"] if s == 0) >= 100 and {-err[a], -err[b]} <= set(want["status"].tolist())


# ---- 9. a dictionary
def test_with_a_dictionary(engine):
    import zeekstd_amd as zk
    idx, blob = df.load()
    d = df.piece(blob, idx["dicts"]["trained"])
    sizes = [300, 0, 2000, 70000, 17, 1500]
    cdict = zk.EncodeDictionary(engine, zk.Dictionary(d))
    try:
        arc = make_arc(engine, sizes, 0, dictionary=cdict, data=df.records(77, sum(sizes)))
        ids, voff = V.views(arc.sizes)["thrice_interleaved"]
        engine.set_dictionary(zk.Dictionary(d))
        check(engine, arc, ids, voff, V.ranges_of(voff), "shuffled", "dictionary")
    finally:
        engine.set_dictionary(None)
        cdict.close()


# ---- 10. while batches are in flight
def test_in_flight(engine):
    arc = edge_arc(engine)
    ids, voff = V.views(arc.sizes)["reversed"]
    ranges = V.ranges_of(voff, dense=False)[:60]
    given, offs, end = V.destinations(ranges, "shuffled")
    batch = F.engine_made(engine, 8, 65536, 0x51E3)
    with F.Flight(engine) as fl:
        fl.reach("ctx0", batch)
        before = engine.ranges_frames_decoded()
        rc, st, got, decoded = call(engine, arc, ids, voff, ranges, given, end, end + TAIL)
        assert rc == F.REFUSED and (got == POISON).all() and (st == ST_POISON).all() and decoded == before
        fl.wait_all()
    with F.Flight(engine) as fl:
        fl.reach("ctx1", batch)
        check(engine, arc, ids, voff, ranges, "shuffled", "beside context 1")
        fl.wait_all()                                            # (the batch's bytes and statuses are checked there)
    with F.Flight(engine) as fl:
        fl.reach("both", batch)
        rc, st, got, _ = call(engine, arc, ids, voff, ranges, given, end, end + TAIL)
        assert rc == F.REFUSED and (got == POISON).all() and (st == ST_POISON).all()
        fl.wait_all()


def test_kernels_are_registered(engine):
    import zeekstd_amd as zk
    names = {zk.lib.zk_engine_kernel_name(k).decode() for k in range(zk.lib.zk_engine_kernel_count())}
    assert {"zk_k_view_plan", "zk_k_view_mark", "zk_k_view_gather", "zk_k_view_status"} <= names
    arc = edge_arc(engine)
    ids, voff = V.views(arc.sizes)["reversed"]
    engine.set_profiling(True)
    try:
        check(engine, arc, ids, voff, V.ranges_of(voff, dense=False), "packed", "profiled")
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert all(times.get(k, 0) > 0 for k in ("zk_k_view_plan", "zk_k_view_mark", "zk_k_view_gather", "zk_k_view_status")), times


# ---- 11. DedupStore end to end
def test_dedup_store_read_ranges(engine):
    import zeekstd_amd as zk
    rng = np.random.default_rng(23)
    one = bytearray(zko.gen_chunks(300000, 0x51E4))
    two = bytearray(one)
    for at in (1000, 77777, 200001):
        two[at:at + 40] = bytes(rng.integers(0, 256, 40, dtype=np.uint8))
    one, two = bytes(one), bytes(two)
    store = zk.DedupStore(engine, level=1)
    try:
        (ids1, off1), (ids2, off2) = (store.append(t, avg_size=1024) for t in (one, two))
        assert len(set(ids2.tolist()) & set(ids1.tolist())) > len(ids2) // 2          # most chunks of the second version are the first's

        def slices(text, off):
            n = len(text)
            r = [(0, n), (n - 1, 1), (n, 0), (999, 100), (77770, 5000), (150000, 100000)] + [(int(o), 1) for o in off[1:-1:17]]
            return [o for o, _ in r], [k for _, k in r], [text[o:o + k] for o, k in r]
        for text, ids, off in ((one, ids1, off1), (two, ids2, off2)):
            o, k, want = slices(text, off)
            assert store.read_ranges(ids, off, o, k) == want
        (new2,) = store.compact([ids2])
        o, k, want = slices(two, off2)
        assert store.read_ranges(new2, off2, o, k) == want and store.read(new2, off2) == two
        assert store.read_ranges(new2, off2, [], []) == []
    finally:
        store.close()

"""zk_frame_digests[_dev] and zk_archive_digests_dev on the GPU (include/zeekstd_amd.h "THE DIGEST"; zeekstd_amd/csrc/zk_digest.hip, zk_digest.h):
SHA-256 and the BLAKE2s tree of every frame against hashlib (tests/helpers/digest_model.py) on the lists the emulator tests run, from source
pointers 0, 1, 3 and 15 bytes off, with nothing written behind the digests; a list that lies wholly beyond 2^32 and one that straddles it; the
refusals; the archive route in passes of 1 KiB, over a sub-range, against a dictionary and with a damaged frame; the calls while decode batches
are in flight; DedupStore.digests()."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import zeekstd_amd as zk
from helpers import cdc_model as CM
from helpers import digest_model as D
from helpers import enc_dict_sim as S
from helpers import in_flight as IF
from helpers.dev_decode import dev as _dev

pytestmark = pytest.mark.gpu

POISON, GUARD = D.POISON, 256
ARG, TOO_MANY = D.ARGUMENT, D.FRAME_INDEX_TOO_LARGE
MAX_FRAMES = 0x08000000                                      # ZK_SEEKABLE_MAX_FRAMES
ALGOS = list(D.ALGOS)


def _i64(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).to(_dev())


def _u8(a, lead=0, pad=0):
    """the bytes on the device, `lead` bytes into a fresh allocation -> (tensor, address of the first byte)"""
    import torch
    a = np.frombuffer(bytes(a), np.uint8) if not isinstance(a, np.ndarray) else a
    t = torch.zeros(max(len(a) + lead + pad, 1), dtype=torch.uint8, device=_dev())
    if len(a):
        t[lead:lead + len(a)] = torch.from_numpy(a.copy()).to(_dev())
    return t, t.data_ptr() + lead


def _poisoned(count):
    import torch
    return torch.full((count * 32 + GUARD,), POISON, dtype=torch.uint8, device=_dev())


def _split(out, count):
    got = out.cpu().numpy()
    return got[:count * 32].reshape(count, 32), got[count * 32:]


def dev_digests(engine, algo, src_ptr, off, count=None, out=None, out_ptr=None):
    """zk_frame_digests_dev over a poisoned array -> (rc, digests, the bytes behind them)"""
    off = np.asarray(off, np.uint64)
    count = len(off) - 1 if count is None else count
    n = max(len(off) - 1, 0)
    out = _poisoned(n) if out is None else out
    d_off = _i64(off) if len(off) else None
    IF.settle()
    rc = zk.lib.zk_frame_digests_dev(engine._h, D.ALGOS.get(algo, algo), src_ptr, d_off.data_ptr() if d_off is not None else None, count,
                                     out.data_ptr() if out_ptr is None else out_ptr, None)
    return (rc, *_split(out, n))


def assert_rows(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (what, bad[:8].tolist())


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(D.lists()))
def test_model_lists(engine, algo, name):
    """device and host form equal hashlib on every list at the four misalignments; the bytes behind 32 * count stay; Engine.frame_digests agrees"""
    data, off = D.lists()[name]
    want = D.want(algo, name)
    for misalign in D.MISALIGN:
        t, p = _u8(data, lead=misalign)
        shift = np.uint64(0 if misalign == 0 else 1000 + misalign)              # (the offsets are coordinates: the source pointer names byte 0)
        rc, got, tail = dev_digests(engine, algo, p - int(shift), off + shift)
        assert rc == 0, (name, misalign, rc)
        assert_rows(got, want, (algo, name, misalign))
        assert (tail == POISON).all(), (algo, name, misalign, "a store behind the digests")
    host = engine.frame_digests(data, off, algo)
    assert host.shape == (len(off) - 1, 32) and host.dtype == np.uint8
    assert_rows(host, want, (algo, name, "host"))
    lead = np.concatenate([np.full(77, 0x5A, np.uint8), data])                   # off[0] != 0 on the host route
    assert_rows(engine.frame_digests(lead, off + np.uint64(77), algo), want, (algo, name, "host, off[0] = 77"))


def test_the_header_s_literals(engine):
    assert engine.frame_digests(b"", [0, 0], "sha256")[0].tobytes().hex() == D.EMPTY_SHA256
    assert engine.frame_digests(b"", [0, 0], "blake2s-tree")[0].tobytes().hex() == D.EMPTY_TREE
    assert engine.frame_digests(bytes(i & 255 for i in range(4097)), [0, 4097], "blake2s-tree")[0].tobytes().hex() == D.TREE_4097
    with pytest.raises(ValueError):
        engine.frame_digests(b"", [0, 0], "md5")


@pytest.fixture(scope="module")
def beyond():
    """a device buffer of 2^32 + 8 MiB bytes of which only the last 9 MiB are filled: every 8-byte word carries its own index, so an offset cut to
    32 bits reads other bytes.  -> (tensor, the host copy of the filled tail, the byte the tail starts at)"""
    import torch
    total = (1 << 32) + (8 << 20)
    start = (1 << 32) - (1 << 20)
    buf = torch.empty(total // 8, dtype=torch.int64, device=_dev())
    buf[start // 8:] = torch.arange(start // 8, total // 8, dtype=torch.int64, device=_dev())
    tail = np.arange(start // 8, total // 8, dtype=np.uint64).view(np.uint8)
    yield buf, tail, start
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("algo", ALGOS)
def test_a_list_beyond_2_to_the_32(engine, beyond, algo):
    buf, tail, start = beyond
    rng = np.random.default_rng(32)
    for what, first, sizes in (("wholly beyond", (1 << 32) + 12345, rng.integers(0, 200 << 10, 40)),
                               ("straddles", (1 << 32) - 70000, np.array([0, 100000, 5, 4097, 0, 30000, 64, 8192]))):
        if what == "wholly beyond":
            sizes[[3, 17]] = 0
        off = np.zeros(len(sizes) + 1, np.uint64)
        off[0] = first
        off[1:] = first + np.cumsum(sizes.astype(np.uint64))
        assert int(off[-1]) <= start + len(tail)
        want = D.model(algo, tail, off - np.uint64(start))
        rc, got, behind = dev_digests(engine, algo, buf.data_ptr(), off)
        assert rc == 0, (what, rc)
        assert_rows(got, want, (algo, what))
        assert (behind == POISON).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_refusals(engine, algo):
    """the codes of the rule; a refused call leaves the poisoned digests as they were"""
    import torch
    data, off = D.lists()["short_65"]
    t, p = _u8(data)
    count = len(off) - 1

    def untouched(r):
        return (r[1] == POISON).all() and (r[2] == POISON).all()

    for bad in (0, 3, -1, 256 + D.ALGOS[algo]):
        r = dev_digests(engine, bad, p, off)
        assert r[0] == ARG and untouched(r), bad
        assert zk.lib.zk_frame_digests_dev(engine._h, bad, None, None, 0, None, None) == ARG           # (before anything is looked at)
    down = off.copy()
    down[10] = down[9] - np.uint64(1) if down[9] else down[11] + np.uint64(1)
    r = dev_digests(engine, algo, p, down)
    assert r[0] == ARG and untouched(r)
    out = _poisoned(count)
    for k in (1, 2, 3):
        r = dev_digests(engine, algo, p, off, out=out, out_ptr=out.data_ptr() + k)
        assert r[0] == ARG and untouched(r), k
    d_off = _i64(off)
    IF.settle()
    assert zk.lib.zk_frame_digests_dev(engine._h, D.ALGOS[algo], p, None, count, out.data_ptr(), None) == ARG
    assert zk.lib.zk_frame_digests_dev(engine._h, D.ALGOS[algo], p, d_off.data_ptr(), count, None, None) == ARG
    assert zk.lib.zk_frame_digests_dev(engine._h, D.ALGOS[algo], None, d_off.data_ptr(), count, out.data_ptr(), None) == ARG       # bytes, but no source
    assert zk.lib.zk_frame_digests_dev(engine._h, D.ALGOS[algo], p, d_off.data_ptr(), MAX_FRAMES + 1, out.data_ptr(), None) == TOO_MANY
    assert zk.lib.zk_frame_digests_dev(engine._h, D.ALGOS[algo], None, None, 0, None, None) == 0
    assert (out.cpu().numpy() == POISON).all()
    # NULL source with nothing to read is a list like any other
    r = dev_digests(engine, algo, None, np.zeros(4, np.uint64))
    assert r[0] == 0 and all(row.tobytes() == D.digest(algo, b"") for row in r[1])
    # the host form
    host = np.full(count * 32 + 64, POISON, np.uint8)
    args = (data.ctypes.data, off.ctypes.data, count, host.ctypes.data)
    assert zk.lib.zk_frame_digests(engine._h, 7, *args) == ARG
    assert zk.lib.zk_frame_digests(engine._h, D.ALGOS[algo], data.ctypes.data, down.ctypes.data, count, host.ctypes.data) == ARG
    assert zk.lib.zk_frame_digests(engine._h, D.ALGOS[algo], data.ctypes.data, None, count, host.ctypes.data) == ARG
    assert zk.lib.zk_frame_digests(engine._h, D.ALGOS[algo], data.ctypes.data, off.ctypes.data, count, None) == ARG
    assert zk.lib.zk_frame_digests(engine._h, D.ALGOS[algo], None, off.ctypes.data, count, host.ctypes.data) == ARG
    assert zk.lib.zk_frame_digests(engine._h, D.ALGOS[algo], data.ctypes.data, off.ctypes.data, MAX_FRAMES + 1, host.ctypes.data) == TOO_MANY
    assert zk.lib.zk_frame_digests(engine._h, D.ALGOS[algo], None, None, 0, None) == 0
    assert (host == POISON).all()


# ---------------------------------------------------------------- the archive route
class Archive:
    """a list encoded with checksums: the payload (64 bytes of padding behind it) and its prefix sums on the device"""

    def __init__(self, engine, name, dictionary=None):
        self.data, self.off = D.lists()[name]
        self.name, self.count = name, len(self.off) - 1
        comp, sizes = engine.encode_frame_list(self.data, self.off, level=1, checksum=True, dictionary=dictionary)
        self.comp = np.frombuffer(comp, np.uint8).copy()
        self.c_off = np.zeros(self.count + 1, np.uint64)
        self.c_off[1:] = np.cumsum([s[0] for s in sizes], dtype=np.uint64)
        assert [s[1] for s in sizes] == np.diff(self.off.astype(np.int64)).tolist()
        self.upload(self.comp)

    def upload(self, comp):
        self.d_comp, _ = _u8(comp, pad=64)
        self.d_c, self.d_d = _i64(self.c_off), _i64(self.off)

    def digests(self, engine, algo, first=0, count=None, pass_kib=0):
        count = self.count - first if count is None else count
        out = _poisoned(count)
        IF.settle()
        try:
            engine.set_kernel_choice(dedup_pass_kib=pass_kib)
            rc = zk.lib.zk_archive_digests_dev(engine._h, D.ALGOS[algo], self.d_comp.data_ptr(), len(self.comp), self.d_c.data_ptr(), self.d_d.data_ptr(), first, count,
                                               out.data_ptr(), None)
        finally:
            engine.set_kernel_choice(dedup_pass_kib=0)
        return (rc, *_split(out, count))


_ARCH = {}


def archive(engine, name):
    if name not in _ARCH:
        _ARCH[name] = Archive(engine, name)
    return _ARCH[name]


@pytest.mark.parametrize("algo", ALGOS)
def test_archive_digests_equal_the_raw_frames(engine, algo):
    """the edge list -- empty frames among it -- encoded with checksums: in one pass, in passes of 1 KiB (several frames in one, a frame above a
    pass), over a sub-range"""
    a = archive(engine, "edges_waves")
    want = D.want(algo, "edges_waves")
    assert (np.diff(a.off.astype(np.int64)) == 0).any() and int(a.off[-1]) > 100 << 10
    for pass_kib in (0, 1):
        rc, got, behind = a.digests(engine, algo, pass_kib=pass_kib)
        assert rc == 0, (pass_kib, rc)
        assert_rows(got, want, (algo, "pass", pass_kib))
        assert (behind == POISON).all()
    rc, got, behind = a.digests(engine, algo, first=3, count=7, pass_kib=1)
    assert rc == 0
    assert_rows(got, want[3:10], (algo, "frames 3 .. 9"))
    assert (behind == POISON).all()
    assert zk.lib.zk_archive_digests_dev(engine._h, D.ALGOS[algo], a.d_comp.data_ptr(), len(a.comp), a.d_c.data_ptr(), a.d_d.data_ptr(), 5, 0, None, None) == 0


@pytest.mark.parametrize("algo", ALGOS)
def test_archive_digests_against_a_dictionary(engine, algo):
    d = S.fixture_dicts()["trained"]
    cdict = zk.EncodeDictionary(engine, zk.Dictionary(d))
    try:
        a = Archive(engine, "short_257", dictionary=cdict)
        engine.set_dictionary(zk.Dictionary(d))
        rc, got, behind = a.digests(engine, algo, pass_kib=1)
        assert rc == 0, rc
        assert_rows(got, D.want(algo, "short_257"), (algo, "dictionary"))
        assert (behind == POISON).all()
    finally:
        engine.set_dictionary(None)
        cdict.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_archive_refusals_and_a_damaged_frame(engine, algo):
    """a frame with a flipped payload byte returns that frame's -(code) -- what zk_decode_frames_dev returns for the same archive -- and nothing
    outside d_digests[0, 32 count) is written; an unknown algo, NULL pointers, a misaligned array, a range beyond any table"""
    import torch
    a = Archive(engine, "edges")
    code = D.ALGOS[algo]
    args = (a.d_comp.data_ptr(), len(a.comp), a.d_c.data_ptr(), a.d_d.data_ptr())
    out = _poisoned(a.count)
    IF.settle()
    for rc in (zk.lib.zk_archive_digests_dev(engine._h, 9, *args, 0, a.count, out.data_ptr(), None),
               zk.lib.zk_archive_digests_dev(engine._h, code, None, *args[1:], 0, a.count, out.data_ptr(), None),
               zk.lib.zk_archive_digests_dev(engine._h, code, *args, 0, a.count, None, None),
               zk.lib.zk_archive_digests_dev(engine._h, code, *args, 0, a.count, out.data_ptr() + 2, None),
               zk.lib.zk_archive_digests_dev(engine._h, code, *args, MAX_FRAMES - 1, 2, out.data_ptr(), None)):
        assert rc == ARG
    assert zk.lib.zk_archive_digests_dev(engine._h, code, *args, 0, MAX_FRAMES + 1, out.data_ptr(), None) == TOO_MANY
    assert (out.cpu().numpy() == POISON).all()
    j = int(np.argmax(np.diff(a.off.astype(np.int64)) == 4096))
    damaged = a.comp.copy()
    damaged[int(a.c_off[j]) + 100] ^= 0x40
    a.upload(damaged)
    dst = torch.zeros(int(a.off[-1]) + 64, dtype=torch.uint8, device=_dev())
    IF.settle()
    expect = engine.decode_frames_dev(a.d_comp, len(a.comp), a.d_c, a.d_d, 0, a.count, dst, int(a.off[-1]), True)
    assert expect < 0 and expect > -1000
    for pass_kib in (0, 1):
        rc, _, behind = a.digests(engine, algo, pass_kib=pass_kib)
        assert rc == expect, (pass_kib, rc, expect)
        assert (behind == POISON).all()
    # frames in front of the damaged one are none of its business
    rc, got, _ = a.digests(engine, algo, first=0, count=j)
    assert rc == 0
    assert_rows(got, D.want(algo, "edges")[:j], (algo, "in front of the damaged frame"))


@pytest.mark.parametrize("state", IF.STATES)
def test_in_flight_rows(engine, state):
    """zk_frame_digests[_dev] use the encoder's scratch: served in every state.  zk_archive_digests_dev decodes on context 0: refused while it holds a
    batch, with the digests as they were.  The batches' outputs are checked when they are waited for"""
    a = archive(engine, "edges_waves")
    data, off = D.lists()["edges"]
    t, p = _u8(data, lead=3)
    with IF.Flight(engine) as fl:
        fl.reach(state, IF.Staged(IF.long_()), IF.Staged(IF.long_()))
        for algo in ALGOS:
            rc, got, behind = dev_digests(engine, algo, p, off)
            assert rc == 0 and (behind == POISON).all()
            assert_rows(got, D.want(algo, "edges"), (state, algo, "list"))
            assert_rows(engine.frame_digests(data, off, algo), D.want(algo, "edges"), (state, algo, "host"))
            rc, got, behind = a.digests(engine, algo, pass_kib=64)
            if 0 in IF.BUSY[state]:
                assert rc == ARG and (got == POISON).all() and (behind == POISON).all(), (state, algo)
            else:
                assert rc == 0 and (behind == POISON).all(), (state, algo, rc)
                assert_rows(got, D.want(algo, "edges_waves"), (state, algo, "archive"))
        assert set(fl.live) == IF.BUSY[state]
        fl.wait_all()


def test_kernel_times_name_the_digest_kernels(engine):
    data, off = D.lists()["edges"]
    t, p = _u8(data)
    zk.lib.zk_engine_set_profiling(engine._h, 1)
    try:
        assert dev_digests(engine, "blake2s-tree", p, off)[0] == 0
        tree = engine.kernel_times()
        assert dev_digests(engine, "sha256", p, off)[0] == 0
        sha = engine.kernel_times()
    finally:
        zk.lib.zk_engine_set_profiling(engine._h, 0)
    assert {"zk_k_digest_plan", "zk_k_digest_leaves", "zk_k_digest_roots"} <= set(tree), tree
    assert "zk_k_digest_leaves" in sha and "zk_k_digest_roots" not in sha, sha


def test_dedup_store_digests(engine):
    """after two appends with overlap, and after a compact, the digests are hashlib's of every stored chunk as store.read returns it"""
    rng = np.random.default_rng(11)
    paragraphs = [CM.word_text(300 + k, int(n)).tobytes() for k, n in enumerate(rng.integers(600, 3000, 16))]
    one = b"".join(paragraphs[int(k)] for k in rng.integers(0, 12, 40))
    two = b"".join(paragraphs[int(k)] for k in rng.integers(4, 16, 40))
    store = zk.DedupStore(engine, level=1)

    def check():
        n = store.n_frames
        sizes = np.diff(store._d_off.astype(np.int64))
        chunks = [store.read([i], [0, int(sizes[i])]) for i in range(n)]
        for algo in ALGOS:
            got = store.digests(algo=algo)
            assert got.shape == (n, 32)
            assert [g.tobytes() for g in got] == [D.digest(algo, c) for c in chunks], algo
        part = store.digests(first=2, count=5, algo="sha256")
        assert [g.tobytes() for g in part] == [hashlib.sha256(c).digest() for c in chunks[2:7]]
        assert store.digests(first=n, algo="sha256").shape == (0, 32)
        with pytest.raises(ValueError):
            store.digests(first=n - 1, count=2)

    try:
        ids1, _ = store.append(one, avg_size=256)
        n1 = store.n_frames
        ids2, off2 = store.append(two, avg_size=256)
        assert (ids2 < n1).any() and store.n_frames > n1
        check()
        (ids2,) = store.compact([ids2])
        assert store.n_frames < n1 + len(ids2) and store.read(ids2, off2) == two
        check()
    finally:
        store.close()

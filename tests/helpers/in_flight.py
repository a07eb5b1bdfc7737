"""TEST INFRASTRUCTURE -- what tests/test_gpu_in_flight.py submits with zk_decode_submit_dev, how it gets the engine into each of the three
busy states, and the rows of the contract table above zk_decode_submit_dev (include/zeekstd_amd.h) as calls with small arguments of their own.

A Batch is an archive with what every frame of it must decode to; expected bytes are the generator's (tests/helpers/gen_batches.py, frames
cached per process), an encoder input's own, or -- for damaged frames -- the oracle's.  A Staged is one submission of it: the archive on
the device (uploaded once per batch), an output buffer filled with 0xA5 with 64 bytes of slack behind it, statuses filled with -1.
Staged.check holds the wait's return code, every status, every byte and the slack against the batch: bit-exact, no tolerances.
A Flight keeps the submitted batches of one test by slot and waits for whatever is left when the test ends, whichever way it ends."""
import collections
import ctypes as C
import functools
import time

import numpy as np

from conftest import GOLDENS, PREFIX_GOLDENS, offsets_from_frames
from helpers import gen_batches as G
from helpers.dev_decode import dev, upload
from oracle import zko

POISON = 0xA5
SLACK = 64
REFUSED = -2003                                              # ZK_ERR_ARGUMENT
STATES = ("ctx0", "ctx1", "both")                            # which contexts hold a submitted batch
BUSY = {"ctx0": {0}, "ctx1": {1}, "both": {0, 1}}
FOLLOW_MIN = 512 << 10                                       # ZK_FOLLOW_MIN_FRAME_BYTES (zk_dec_plan.h)

# want: per frame the bytes it decodes to, None where nothing is promised (a refused frame); refused: the frames whose status is not 0;
# codes: {frame: the status it must have}, where one is promised
Batch = collections.namedtuple("Batch", "name comp c d want refused codes verify")


def _batch(name, comp, sizes, want, refused=(), codes=None, verify=True):
    c, d = offsets_from_frames(sizes)
    assert len(want) == len(sizes) and all(w is None or len(w) == s[1] for w, s in zip(want, sizes))
    return Batch(name, bytes(comp), c, d, tuple(want), frozenset(refused), dict(codes or {}), verify)


def _generated(name, frames):
    comp, sizes, _ = G.archive(frames)
    return _batch(name, comp, sizes, [f.data for f in frames])


@functools.lru_cache(maxsize=None)
def small():
    """200 default frames: sizes of 0, 1 and 2 bytes among them, every block type, many blocks with tables of their own"""
    b = _generated("small", G.frames(G.DEFAULT_SEEDS[:200]))
    sizes = np.diff(b.d.astype(np.int64))
    assert (sizes == 0).any() and ((sizes > 0) & (sizes < 32)).any()
    return b


@functools.lru_cache(maxsize=None)
def long_():
    """60 frames with long blocks; more blocks that define tables than frames: no batch for zk_k_entropy_frame"""
    frames = G.frames(G.LONG_SEEDS, "long")
    assert sum(f.own for f in frames) > len(frames)
    return _generated("long", frames)


@functools.lru_cache(maxsize=None)
def shared():
    return _generated("shared", G.batch_shared())


@functools.lru_cache(maxsize=None)
def filt():
    """200 default frames with at most one defining block each: what zk_k_entropy_frame takes when ZK_CHOICE_ENTROPY = 2 asks for it"""
    frames = G.filtered(200)
    assert sum(f.own for f in frames) <= len(frames)
    return _generated("filt", frames)


@functools.lru_cache(maxsize=None)
def dense():
    return _generated("dense", G.frames(G.DENSE_SEEDS, "dense"))


@functools.lru_cache(maxsize=None)
def damaged():
    """filt() with one to three flipped bits in 40 of its frames (the construction of test_fused_kernel_on_damaged_frames_against_the_oracle),
    checksums not verified: a frame is refused exactly where the oracle refuses it, an accepted one carries the oracle's bytes"""
    base = filt()
    c, d = base.c, base.d
    rng = np.random.default_rng(31)
    bad = bytearray(base.comp)
    hit = sorted(int(x) for x in rng.choice(len(base.want), 40, replace=False))
    for f in hit:
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(int(c[f]), int(c[f + 1])))] ^= 1 << int(rng.integers(0, 8))
    want, refused = list(base.want), set()
    for f in hit:
        n = int(d[f + 1] - d[f])
        try:
            o, used = zko.frame_decode(bytes(bad[int(c[f]):int(c[f + 1])]), n + 64, False)
            want[f] = o if len(o) == n and used == int(c[f + 1] - c[f]) else None
        except zko.OracleError:
            want[f] = None
        if want[f] is None: refused.add(f)
    assert len(refused) >= 8 and len(hit) - len(refused) >= 4, (len(refused), len(hit))
    assert min(refused) > 0, "the first failing frame is not the first frame"
    sizes = list(zip(np.diff(c.astype(np.int64)).tolist(), np.diff(d.astype(np.int64)).tolist()))
    return _batch("damaged", bad, sizes, want, refused, verify=False)


_MADE = {}


def engine_made(engine, nf, fs, seed, repeat=1):
    """an archive this engine's encoder makes of zko.gen_chunks, level 1, checksummed (made while nothing is in flight; cached) -- `repeat` times over"""
    key = (nf, fs, seed)
    if key not in _MADE:
        data = zko.gen_chunks(nf * fs, seed)
        comp, sizes = engine.encode_frames(data, fs, 1, True)
        assert len(sizes) == nf
        _MADE[key] = (comp, sizes, [data[i * fs:(i + 1) * fs] for i in range(nf)])
    comp, sizes, want = _MADE[key]
    return _batch("made_%dx%d_%x_x%d" % (nf, fs, seed, repeat), comp * repeat, list(sizes) * repeat, want * repeat)


def checksum_flipped(batch, frame):
    """the batch with one bit flipped in the stored Content_Checksum of `frame`: -22 for that frame alone, every byte as before"""
    bad = bytearray(batch.comp)
    bad[int(batch.c[frame + 1]) - 1] ^= 0x40
    sizes = list(zip(np.diff(batch.c.astype(np.int64)).tolist(), np.diff(batch.d.astype(np.int64)).tolist()))
    return _batch(batch.name + "_cks%d" % frame, bad, sizes, batch.want, {frame}, {frame: 22})


# ---------------------------------------------------------------------------------------------- one submission
_UPLOADED = {}


def uploaded(batch):
    if batch.name not in _UPLOADED:
        _UPLOADED[batch.name] = upload(batch.comp, batch.c, batch.d)
    return _UPLOADED[batch.name]


def settle():
    """the fills and uploads the test queued on torch's stream are done (the engine's queues are not ordered behind torch's).  Not a device-wide
    synchronisation: that would wait for the submitted batches too"""
    import torch
    torch.cuda.current_stream().synchronize()


def poisoned(n):
    import torch
    return torch.full((n + SLACK,), POISON, dtype=torch.uint8, device=dev())


def minus_ones(n, dtype=None):
    import torch
    return torch.full((n,), -1, dtype=dtype or torch.int32, device=dev())


class Staged:
    def __init__(self, batch, first=0, count=None, out=None):
        import torch
        self.b, self.first = batch, first
        self.count = len(batch.want) - first if count is None else count
        self.total = int(batch.d[first + self.count] - batch.d[first])
        self.arch = uploaded(batch)
        self.out = poisoned(self.total) if out is None else out
        assert self.out.numel() == self.total + SLACK
        self.out.fill_(POISON)
        self.st = minus_ones(self.count)
        settle()

    def args(self):
        return (*self.arch, self.first, self.count, self.out, self.total, self.b.verify, self.st)

    def check(self, rc, what=""):
        b = self.b
        st = self.st.cpu().numpy()
        got = self.out.cpu().numpy()
        what = (b.name, what)
        assert (got[self.total:] == POISON).all(), ("slack written", what)
        frames = range(self.first, self.first + self.count)
        bad = {self.first + int(i) for i in np.flatnonzero(st)}
        assert bad == {f for f in b.refused if f in frames}, (what, sorted(bad)[:5], sorted(b.refused)[:5])
        for f, code in b.codes.items():
            if f in frames: assert st[f - self.first] == code, (what, f, int(st[f - self.first]))
        assert rc == (-int(st[min(bad) - self.first]) if bad else 0), (what, rc)
        base = int(b.d[self.first])
        if all(b.want[f] is not None for f in frames):
            assert got[:self.total].tobytes() == b"".join(b.want[f] for f in frames), what
        else:
            for f in frames:
                if b.want[f] is not None:
                    assert got[int(b.d[f]) - base:int(b.d[f + 1]) - base].tobytes() == b.want[f], (what, f)
        return st


def decode_sync(engine, batch, stream=None):
    """zk_decode_frames_dev of the whole batch -> (rc, Staged)"""
    s = Staged(batch)
    return engine.decode_frames_dev(*s.args(), stream), s


class Flight:
    """the batches one test has submitted, by slot.  Leaving the `with` block waits for whatever is still outstanding (and checks it, unless
    the block is being left by an exception), then puts the kernel choice and the dictionary back"""

    def __init__(self, engine, reset=True):
        self.e, self.live, self.reset = engine, {}, reset
        self.waited = 0.0                                    # seconds spent inside zk_decode_wait

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            for slot in sorted(self.live):
                s = self.live.pop(slot)
                rc = self.e.decode_wait(slot)
                if exc_type is None: s.check(rc, "left outstanding")
        finally:
            if self.reset:
                self.e.set_kernel_choice(reset=0)
                self.e.set_dictionary(None)
        return False

    def submit(self, batch, first=0, count=None, out=None):
        """a Batch, or a Staged made beforehand (staging takes time the batch submitted before it would use to finish)"""
        s = batch if isinstance(batch, Staged) else Staged(batch, first, count, out)
        slot = self.e.decode_submit_dev(*s.args())
        assert slot in (0, 1) and slot not in self.live, slot
        self.live[slot] = s
        return slot

    def wait(self, slot, what=""):
        """-> (the wait's return code, the statuses); the batch's results are checked"""
        t0 = time.perf_counter()
        rc = self.e.decode_wait(slot)
        self.waited += time.perf_counter() - t0
        s = self.live.pop(slot)
        return rc, s.check(rc, what)

    def wait_all(self):
        for slot in sorted(self.live): self.wait(slot)

    def reach(self, state, first, second=None):
        """submits and waits until exactly the contexts of `state` hold a batch, going by the slots the engine returns: `first`, and
        `second` where the turn was the other context's (or for "both").  Batches, or Stageds (then two of them)"""
        assert not self.live
        second = first if second is None else second
        assert not isinstance(first, Staged) or second is not first
        s = self.submit(first)
        if state == "both":
            assert {s, self.submit(second)} == {0, 1}
        else:
            want = 0 if state == "ctx0" else 1
            if s != want:
                assert self.submit(second) == want
                self.wait(s)
        assert set(self.live) == BUSY[state]


# ---------------------------------------------------------------------------------------------- the contract table, row by row
A, B, BOTH = STATES
ALWAYS_SERVED = {A: "served", B: "served", BOTH: "served"}
ALWAYS_REFUSED = {A: "refused", B: "refused", BOTH: "refused"}
NEEDS_CONTEXT_0 = {A: "refused", B: "served", BOTH: "refused"}
# run() makes the call with fresh buffers -> (return code, check of a served call, check that a refused call touched nothing)
Row = collections.namedtuple("Row", "name verdict run")


def _p(x):
    if x is None: return None
    if hasattr(x, "data_ptr"): return x.data_ptr()
    if isinstance(x, np.ndarray): return x.ctypes.data
    return int(x)


def _nothing():
    pass


def contract_rows(engine):
    """Every row of the table in include/zeekstd_amd.h but zk_decode_submit_dev / zk_decode_wait (test_slot_discipline), the zk_decoder_*
    reads (test_decoder_handles_keep_their_state) and zk_engine_destroy (test_destroy_completes_outstanding_batches).  Called while nothing is
    in flight: the expected results that are not the input's own bytes, the twin's or zko.xxh64's are the same call's with nothing in flight."""
    import torch
    import zeekstd_amd as zk
    from zeekstd_amd import api
    L, h, e = zk.lib, engine._h, engine
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).to(dev())
    g = next(x for x in GOLDENS if x.name == "text_l1_64k")
    c, d = g.offsets()
    data, nf, total = g.input(), len(g.frames), int(d[-1])
    gcomp = np.frombuffer(g.comp + b"\0" * 8, np.uint8).copy()
    arch = upload(g.comp, c, d)
    rows = []

    def exact(out, st, want):
        got = out.cpu().numpy() if hasattr(out, "cpu") else out
        st = st.cpu().numpy() if hasattr(st, "cpu") else st
        assert not st.any() and got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all()

    def untouched(*bufs):
        def check():
            for b, fill in bufs:
                got = b.cpu().numpy() if hasattr(b, "cpu") else b
                assert (got == got.dtype.type(fill)).all()
        return check

    def add(name, verdict):
        def deco(fn):
            rows.append(Row(name, verdict, fn))
            return fn
        return deco

    # ---- synchronous device-pointer decodes: context 0's
    def frames_dev(stream):
        def run():
            out, st = poisoned(total), minus_ones(nf)
            settle()
            rc = L.zk_decode_frames_dev(h, _p(arch[0]), arch[1], _p(arch[2]), _p(arch[3]), 0, nf, _p(out), total, 1, _p(st), stream)
            return rc, lambda: (_eq(rc, 0), exact(out, st, data)), untouched((out, POISON), (st, -1))
        return run
    add("zk_decode_frames_dev", NEEDS_CONTEXT_0)(frames_dev(None))
    side = torch.cuda.Stream()
    add("zk_decode_frames_dev on the caller's stream", NEEDS_CONTEXT_0)(frames_dev(side.cuda_stream))

    pg = next(x for x in PREFIX_GOLDENS if x.name == "pfx_text_l1")
    pc, pd = pg.offsets()
    pdata, pn, ptotal, prefix = pg.input(), len(pg.frames), int(pd[-1]), pg.prefix()
    parch = upload(pg.comp, pc, pd)
    d_prefix = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).to(dev())
    pcomp = np.frombuffer(pg.comp + b"\0" * 8, np.uint8).copy()
    h_prefix = np.frombuffer(prefix, np.uint8).copy()

    @add("zk_decode_frames_prefix_dev", NEEDS_CONTEXT_0)
    def _():
        out, st = poisoned(ptotal), minus_ones(pn)
        settle()
        rc = L.zk_decode_frames_prefix_dev(h, _p(parch[0]), parch[1], _p(parch[2]), _p(parch[3]), 0, pn, _p(d_prefix), len(prefix), _p(out), ptotal, 1, _p(st), None)
        return rc, lambda: (_eq(rc, 0), exact(out, st, pdata)), untouched((out, POISON), (st, -1))

    ids = np.array([3, 0, 2, 2, 1], np.uint32)
    sizes = (d[1:] - d[:-1])[ids]
    oo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    d_ids, d_oo = torch.from_numpy(ids.view(np.int32).copy()).to(dev()), t64(oo)
    listed = b"".join(data[int(d[i]):int(d[i + 1])] for i in ids)

    @add("zk_decode_frame_list_dev", NEEDS_CONTEXT_0)
    def _():
        out, st = poisoned(len(listed)), minus_ones(len(ids))
        settle()
        rc = L.zk_decode_frame_list_dev(h, _p(arch[0]), arch[1], _p(arch[2]), _p(arch[3]), _p(d_ids), _p(d_oo), len(ids), _p(out), len(listed), 1, _p(st), None)
        return rc, lambda: (_eq(rc, 0), exact(out, st, listed)), untouched((out, POISON), (st, -1))

    want_sizes = (d[1:] - d[:-1]).astype(np.int64)

    @add("zk_frame_content_sizes_dev", NEEDS_CONTEXT_0)
    def _():
        sz, st = minus_ones(nf, torch.int64), minus_ones(nf)
        settle()
        rc = L.zk_frame_content_sizes_dev(h, _p(arch[0]), arch[1], _p(arch[2]), 0, nf, _p(sz), _p(st), None)
        return rc, lambda: (_eq(rc, 0), _eq(sz.cpu().numpy().tolist(), want_sizes.tolist()), _eq(int(st.abs().sum().item()), 0)), untouched((sz, -1), (st, -1))

    at = [int(x) for x in d]
    offs = np.array([5, at[1] - 7, at[2], total - 20, at[3]], np.uint64)      # inside a frame, across a boundary, several frames, the tail, empty
    lens = np.array([50, 300, at[3] - at[2] + 9, 20, 0], np.uint64)
    ranged = b"".join(data[int(o):int(o + n)] for o, n in zip(offs, lens))
    touched = len({f for o, n in zip(offs, lens) if n for f in range(nf) if at[f] < int(o + n) and at[f + 1] > int(o)})
    d_offs, d_lens = t64(offs), t64(lens)

    @add("zk_read_ranges_dev", NEEDS_CONTEXT_0)
    def _():
        out, st = poisoned(len(ranged)), minus_ones(len(offs))
        before = e.ranges_frames_decoded()
        settle()
        rc = L.zk_read_ranges_dev(h, _p(arch[0]), arch[1], _p(arch[2]), _p(arch[3]), nf, _p(d_offs), _p(d_lens), None, len(offs), _p(out), len(ranged), 1, _p(st), None)
        return (rc, lambda: (_eq(rc, 0), exact(out, st, ranged), _eq(e.ranges_frames_decoded(), touched)),
                lambda: (untouched((out, POISON), (st, -1))(), _eq(e.ranges_frames_decoded(), before)))

    # ---- their host-pointer forms: refused BEFORE the staging
    @add("zk_frame_content_sizes", NEEDS_CONTEXT_0)
    def _():
        sz, st = np.full(nf, -1, np.int64), np.full(nf, -1, np.int32)
        before = e.ranges_frames_decoded()
        rc = L.zk_frame_content_sizes(h, _p(gcomp), len(g.comp), _p(c), 0, nf, _p(sz), _p(st))
        return (rc, lambda: (_eq(rc, 0), _eq(sz.tolist(), want_sizes.tolist()), _eq(st.tolist(), [0] * nf)),
                lambda: (untouched((sz, -1), (st, -1))(), _eq(e.ranges_frames_decoded(), before)))

    @add("zk_read_ranges", NEEDS_CONTEXT_0)
    def _():
        out, st = np.full(len(ranged) + SLACK, POISON, np.uint8), np.full(len(offs), -1, np.int32)
        before = e.ranges_frames_decoded()
        rc = L.zk_read_ranges(h, _p(gcomp), len(g.comp), _p(c), _p(d), nf, _p(offs), _p(lens), None, len(offs), _p(out), len(ranged), 1, _p(st))
        return (rc, lambda: (_eq(rc, 0), exact(out, st, ranged), _eq(e.ranges_frames_decoded(), touched)),
                lambda: (untouched((out, POISON), (st, -1))(), _eq(before > 0, True), _eq(e.ranges_frames_decoded(), before)))

    # ---- the host pipeline rotates through both contexts: refused whichever is busy
    @add("zk_decode_frames", ALWAYS_REFUSED)
    def _():
        out, st = np.full(total + SLACK, POISON, np.uint8), np.full(nf, -1, np.int32)
        rc = L.zk_decode_frames(h, _p(gcomp), len(g.comp), _p(c), _p(d), 0, nf, _p(out), total, 1, _p(st))
        return rc, _nothing, untouched((out, POISON), (st, -1))

    @add("zk_decode_frames_prefix", ALWAYS_REFUSED)
    def _():
        out, st = np.full(ptotal + SLACK, POISON, np.uint8), np.full(pn, -1, np.int32)
        rc = L.zk_decode_frames_prefix(h, _p(pcomp), len(pg.comp), _p(pc), _p(pd), 0, pn, _p(h_prefix), len(prefix), _p(out), ptotal, 1, _p(st))
        return rc, _nothing, untouched((out, POISON), (st, -1))

    table = api.SeekTable.new()
    for cs, ds in g.frames: table.log_frame(cs, ds)

    @add("zk_decode_shard", ALWAYS_REFUSED)
    def _():
        out = np.full(total + SLACK, POISON, np.uint8)
        first, count, written = C.c_uint32(), C.c_uint32(), C.c_uint64(7)
        rc = L.zk_decode_shard(h, _p(gcomp), len(g.comp), table._h, 0, 1, _p(out), total, 1, C.byref(first), C.byref(count), C.byref(written))
        return rc, _nothing, lambda: (untouched((out, POISON))(), _eq(written.value, 0))

    raw_dict = zk.Dictionary(b"some raw content for a dictionary" * 8)

    @add("zk_engine_set_dictionary", ALWAYS_REFUSED)
    def _():
        rc = L.zk_engine_set_dictionary(h, raw_dict._h)
        rc_none = L.zk_engine_set_dictionary(h, None)
        return rc, _nothing, lambda: _eq(rc_none, REFUSED)

    comm = np.zeros(64, np.uint8)                            # (never looked into: the call is refused before the collective library is asked for)
    one = np.array([16], np.uint32)
    d_pay = torch.zeros(64, dtype=torch.uint8, device=dev())

    @add("zk_gather_seekable", ALWAYS_REFUSED)
    def _():
        out, n_out = poisoned(256), C.c_uint64(7)
        settle()
        rc = L.zk_gather_seekable(h, _p(comm), 0, 1, 0, _p(d_pay), 16, _p(one), _p(one), 1, 1, _p(out), 256, C.addressof(n_out), None, None)
        return rc, _nothing, lambda: (untouched((out, POISON))(), _eq(n_out.value, 0))

    # ---- encoders and checksums: scratch and queues of their own
    text = zko.gen_text(65536, 9)
    fs = 16384
    twin = b"".join(zko.frame_encode(text[i:i + fs], 1, True) for i in range(0, len(text), fs))
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev())
    cap = int(L.zk_compress_bound(len(text), fs))

    @add("zk_encode_frames_dev / zk_encode_frames_prefix_dev", ALWAYS_SERVED)
    def _():
        out, cs, ds = poisoned(cap), minus_ones(4), minus_ones(4)
        nfo, wr = C.c_uint32(), C.c_uint64()
        settle()
        rc = L.zk_encode_frames_dev(h, _p(d_text), len(text), fs, 1, 1, _p(out), cap, _p(cs), _p(ds), C.byref(nfo), C.byref(wr), None)

        def served():
            assert rc == 0 and nfo.value == 4 and wr.value == len(twin)
            got = out.cpu().numpy()
            assert got[:len(twin)].tobytes() == twin and (got[cap:] == POISON).all()
            assert int(cs.sum().item()) == len(twin) and ds.cpu().numpy().tolist() == [fs] * 4
        return rc, served, _nothing

    @add("zk_encode_frames / zk_encode_frames_prefix", ALWAYS_SERVED)
    def _():
        comp, frames = e.encode_frames(text, fs, 1, True)
        return 0, lambda: (_eq(comp, twin), _eq([f[1] for f in frames], [fs] * 4)), _nothing

    def through_encoder():
        import io
        sink = io.BytesIO()
        enc = api.EncodeOptions().engine(e).frame_size_policy(api.FrameSizePolicy.Uncompressed(fs)).checksum_flag(True).compression_level(1).into_encoder(sink)
        enc.write_all(text)
        enc.finish()
        return sink.getvalue()
    idle = through_encoder()
    assert idle.startswith(twin)

    @add("zk_raw_encoder_* / zk_encoder_*", ALWAYS_SERVED)
    def _():
        got = through_encoder()
        return 0, lambda: _eq(got, idle), _nothing

    hoff = np.array([0, 100, 100, 5000, 65536], np.uint64)
    hashes = [zko.xxh64(text[int(a):int(b)]) for a, b in zip(hoff[:-1], hoff[1:])]
    d_hoff = t64(hoff)

    @add("zk_xxh64_frames_dev", ALWAYS_SERVED)
    def _():
        out = minus_ones(4, torch.int64)
        settle()
        rc = L.zk_xxh64_frames_dev(h, _p(d_text), _p(d_hoff), 4, _p(out), None)
        return rc, lambda: (_eq(rc, 0), _eq(out.cpu().numpy().view(np.uint64).tolist(), hashes)), _nothing

    @add("zk_xxh64_frames", ALWAYS_SERVED)
    def _():
        got = e.xxh64_frames(text, hoff)
        return 0, lambda: _eq(got.tolist(), hashes), _nothing

    # ---- settings and diagnostics: host state only
    @add("zk_engine_set_kernel_choice / _set_fse_kernel / _set_profiling / _set_host_threads", ALWAYS_SERVED)
    def _():
        rcs = [L.zk_engine_set_kernel_choice(h, 1, 1), L.zk_engine_set_kernel_choice(h, 0, 0), L.zk_engine_set_fse_kernel(h, 0),
               L.zk_engine_set_profiling(h, 0), L.zk_engine_set_host_threads(h, 0)]
        return 0, lambda: _eq(rcs, [0] * 5), _nothing

    @add("zk_engine_checksums_followed / _entropy_fused / _ranges_frames_decoded / _kernel_times / _last_hip_error / _device_name", ALWAYS_SERVED)
    def _():
        before = (e.checksums_followed(), e.entropy_fused(), e.ranges_frames_decoded())
        ms = (C.c_float * L.zk_engine_kernel_count())()
        rc = L.zk_engine_kernel_times(h, ms, len(ms))
        name = e.device_name
        L.zk_engine_last_hip_error(h)
        return rc, lambda: (_eq(rc, 0), _eq("gfx950" in name, True), _eq((e.checksums_followed(), e.entropy_fused(), e.ranges_frames_decoded()), before)), _nothing

    # the counter zk_read_ranges' row wants to see kept: a call of it with nothing in flight
    rc, served, _ = next(r for r in rows if r.name == "zk_read_ranges").run()
    served()
    return rows


def _eq(got, want):
    assert got == want, (got, want)


def clock():
    return time.perf_counter()

"""What the engine does between zk_decode_submit_dev and its zk_decode_wait: the contract written above zk_decode_submit_dev in
include/zeekstd_amd.h ("Between a submit and its wait"), held against the device.

  a  batches of different shapes side by side, on a fresh engine whose contexts' scratch grows while the neighbour runs; the diagnostics
     (zk_engine_entropy_fused / zk_engine_checksums_followed) describe the batch that was waited for
  b  every pinned kernel variant with two batches in flight, a batch keeping the plan it was enqueued with; the checksums beside the
     executor (zk_k_xxh64_follow) in both contexts at once, by batch shape
  c  per-slot verdicts: a damaged batch beside an intact one
  d  slot discipline: alternation, waits in any order, what is refused and what a refusal leaves behind
  e  the contract table row by row in each of the three busy states, the zk_decoder_* handles, profiling, zk_engine_destroy
  f  with a dictionary

Expected bytes are the generator's (tests/helpers/gen_batches.py), an encoder input's own, the CPU twin's or the oracle's; every output
buffer is filled with 0xA5 with 64 bytes of slack that must stay, statuses start at -1, comparisons are bit-exact
(tests/helpers/in_flight.py).  No test assumes the slot its first submit gets: busy states are reached by submitting, waiting and reading
the slots the engine returns.  Every test waits for what it submitted (Flight) and leaves kernel choice and dictionary reset."""
import ctypes as C

import numpy as np
import pytest

import zeekstd_amd as zk
from zeekstd_amd import DecodeOptions, SeekTable, api
from zeekstd_amd.engine import ZkError
from conftest import GOLDENS
from helpers import in_flight as IF
from helpers.in_flight import Flight, Staged, REFUSED
from oracle import zko
from test_gpu_generated_variants import ALL_VARIANTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def made(engine):
    """the engine-made archives, encoded once while nothing is in flight.  20 frames of 640 KiB: at >= 512 KiB per frame and <= 64 frames a
    verified batch takes its checksums beside the executor by shape (zk_follow_wanted); two of them of equal layout; 64 frames of 4 KiB"""
    twins = [IF.engine_made(engine, 20, 640 << 10, 0x6400 + i) for i in range(2)]
    for t in twins:
        assert int(t.d[-1]) >= len(t.want) * IF.FOLLOW_MIN and len(t.want) <= 64
    return dict(twins=twins, tiny=IF.engine_made(engine, 64, 4096, 0x6410), big=IF.engine_made(engine, 20, 640 << 10, 0x6400, repeat=8))


def _no_follow_by_shape(batch):
    """frames of less than 512 KiB on average: zk_follow_wanted says no, alone or not -- the batch's plan is the synchronous call's"""
    return int(batch.d[-1]) < len(batch.want) * IF.FOLLOW_MIN


# ------------------------------------------------------------------------------------------------ a: different shapes side by side
def test_different_shapes_side_by_side_on_a_fresh_engine(made):
    """SMALL with LONG, LONG with SMALL, the same again after an odd number of submits (each batch on the other context), SHARED with DENSE, 64
    engine-made frames of 4 KiB with SHARED: every context reserves its scratch for the first time, and grows it, while its neighbour's kernels run (zk_devbuf_reserve frees and
    allocates).  Outputs and statuses are the generator's and equal what zk_decode_frames_dev makes of the same batch afterwards.
    None of these batches has frames of 512 KiB: none takes the checksums beside the executor and none the fused entropy kernel by shape,
    in flight or alone, so both diagnostics must read 0 after every wait and after the synchronous calls."""
    import torch
    batches = dict(small=IF.small(), long=IF.long_(), shared=IF.shared(), dense=IF.dense(), tiny=made["tiny"])
    assert all(_no_follow_by_shape(b) for b in batches.values())
    e = zk.Engine()
    try:
        kept = {}
        with Flight(e) as fl:
            def pair(x, y):
                sx, sy = Staged(batches[x]), Staged(batches[y])
                s0, s1 = fl.submit(sx), fl.submit(sy)
                assert {s0, s1} == {0, 1}
                for slot, name, s in ((s0, x, sx), (s1, y, sy)):
                    rc, st = fl.wait(slot, (x, y))
                    assert rc == 0
                    assert (e.entropy_fused(), e.checksums_followed()) == (False, 0), (name, x, y)
                    kept[name, slot] = (s.out, st)
                return s0
            first = pair("small", "long")
            assert pair("long", "small") == first
            only = fl.submit(batches["small"])
            assert only == first and fl.wait(only)[0] == 0
            assert pair("small", "long") == first ^ 1           # the same order on the other contexts
            pair("shared", "dense")
            pair("tiny", "shared")
            assert {slot for name, slot in kept if name == "small"} == {0, 1} and {slot for name, slot in kept if name == "long"} == {0, 1}
        for name, b in batches.items():
            rc, s = IF.decode_sync(e, b)
            st = s.check(rc, "synchronous")
            assert rc == 0 and (e.entropy_fused(), e.checksums_followed()) == (False, 0)
            for (n, slot), (out, st_in_flight) in kept.items():
                if n == name:
                    assert torch.equal(out, s.out) and np.array_equal(st_in_flight, st), (name, slot)
    finally:
        e.close()


@pytest.mark.parametrize("fused_first", [True, False], ids=["fused_submitted_first", "fused_submitted_second"])
@pytest.mark.parametrize("reverse", [False, True], ids=["waited_in_order", "waited_in_reverse"])
def test_diagnostics_describe_the_batch_that_was_waited_for(engine, made, fused_first, reverse):
    """zk_engine_entropy_fused: FILT under ZK_CHOICE_ENTROPY = 2 runs zk_k_entropy_frame, LONG (more defining blocks than frames) cannot;
    zk_engine_checksums_followed: an archive of 640 KiB frames enqueued under ZK_CHOICE_XXH64 = 4 has its checksums verified beside the
    executor (some of them: tests/test_gpu_kernel_choice.py insists on the same), SMALL enqueued under 1 has none.  In both submit orders and
    both wait orders the values read after a wait are that batch's, whichever was submitted or finished last.  The expected values are the
    synchronous call's under the same pin."""
    want = {}
    with Flight(engine):
        engine.set_kernel_choice(entropy=2)
        for name, b in (("filt", IF.filt()), ("long", IF.long_())):
            rc, s = IF.decode_sync(engine, b)
            s.check(rc)
            want[name] = engine.entropy_fused()
    assert want == {"filt": True, "long": False}
    with Flight(engine) as fl:
        engine.set_kernel_choice(entropy=2)
        order = [("filt", IF.filt()), ("long", IF.long_())][::1 if fused_first else -1]
        staged = [Staged(b) for _, b in order]
        slots = [fl.submit(s) for s in staged]
        assert set(slots) == {0, 1}
        for (name, _), slot in list(zip(order, slots))[::-1 if reverse else 1]:
            assert fl.wait(slot, name)[0] == 0
            assert engine.entropy_fused() == want[name], (name, slot)
    with Flight(engine) as fl:
        followed, plain = Staged(made["twins"][0]), Staged(IF.small())
        pins = [("followed", followed, 4), ("plain", plain, 1)][::1 if fused_first else -1]
        slots = []
        for _, s, xxh in pins:
            engine.set_kernel_choice(xxh64=xxh)
            slots.append(fl.submit(s))
        engine.set_kernel_choice(reset=0)
        for (name, s, _), slot in list(zip(pins, slots))[::-1 if reverse else 1]:
            assert fl.wait(slot, name)[0] == 0
            n = engine.checksums_followed()
            print(name, "on context", slot, "frames verified beside the executor:", n, "of", s.count)
            assert (1 <= n <= s.count) if name == "followed" else n == 0, (name, slot, n)


# ------------------------------------------------------------------------------------------------ b: every pinned variant, two in flight
@pytest.mark.parametrize("variant", list(ALL_VARIANTS), ids=list(ALL_VARIANTS))
def test_every_variant_with_two_batches_in_flight(engine, variant):
    """SMALL and LONG together under each pinned variant.  The choice is pinned before the first submit and reset between the two waits:
    a batch keeps the plan it was enqueued with.  Then an unpinned pair: the reset took."""
    with Flight(engine) as fl:
        a, b = Staged(IF.small()), Staged(IF.long_())
        engine.set_kernel_choice(reset=0)
        engine.set_kernel_choice(**ALL_VARIANTS[variant])
        s0, s1 = fl.submit(a), fl.submit(b)
        assert {s0, s1} == {0, 1}
        assert fl.wait(s0, variant)[0] == 0
        n = engine.checksums_followed()
        engine.set_kernel_choice(reset=0)
        assert fl.wait(s1, variant)[0] == 0
        if ALL_VARIANTS[variant].get("xxh64") == 4:
            print(variant, "frames verified beside the executor:", n, "of", a.count, "and", engine.checksums_followed(), "of", b.count)
            assert n <= a.count and engine.checksums_followed() <= b.count
        c, d = Staged(IF.long_()), Staged(IF.small())
        s0, s1 = fl.submit(c), fl.submit(d)
        assert fl.wait(s1)[0] == 0 and fl.wait(s0)[0] == 0
        assert (engine.entropy_fused(), engine.checksums_followed()) == (False, 0), "by shape neither batch is fused or followed"


def test_checksums_beside_the_executor_in_both_contexts(engine, made):
    """The construction of test_checksums_beside_the_executor with a neighbour: two archives of equal layout (20 frames of 640 KiB, which
    take zk_k_xxh64_follow by shape when submitted), no pin, verify on, on both contexts at once, three rounds into two output buffers
    whose contents alternate between the archives -- a checksum wave that read a stale line of the other archive's bytes would not verify
    its frame.  How many frames the waves verify is the dispatcher's and printed; what they leave is verified behind the executor.
    Then one stored checksum flipped, on either context beside the intact twin: -22 for that frame alone, whichever kernel found it."""
    twins = made["twins"]
    nf, total = len(twins[0].want), int(twins[0].d[-1])
    outs = [IF.poisoned(total), IF.poisoned(total)]
    with Flight(engine) as fl:
        for turn in range(3):
            st = [Staged(twins[(turn + k) & 1], out=outs[k]) for k in range(2)]
            slots = [fl.submit(s) for s in st]
            assert set(slots) == {0, 1}
            for slot in slots:
                assert fl.wait(slot, turn)[0] == 0
                n = engine.checksums_followed()
                print("turn", turn, "context", slot, "frames verified beside the executor:", n, "of", nf)
                assert n <= nf
        for flipped_first in (True, False):
            pair = [Staged(IF.checksum_flipped(twins[0], 7), out=outs[0]), Staged(twins[1], out=outs[1])][::1 if flipped_first else -1]
            slots = [fl.submit(s) for s in pair]
            for s, slot in zip(pair, slots):
                rc, status = fl.wait(slot, flipped_first)
                assert rc == (-22 if s.b.refused else 0)
                assert status.tolist() == [22 if f in s.b.refused else 0 for f in range(nf)]
                assert engine.checksums_followed() <= nf - len(s.b.refused)      # never the damaged frame


# ------------------------------------------------------------------------------------------------ c: per-slot verdicts
@pytest.mark.parametrize("damaged_first", [True, False], ids=["damaged_submitted_first", "damaged_submitted_second"])
@pytest.mark.parametrize("reverse", [False, True], ids=["waited_in_order", "waited_in_reverse"])
def test_each_wait_returns_its_own_batchs_verdict(engine, damaged_first, reverse):
    """DAMAGED (flipped bits in 40 of 200 frames, refused exactly where the oracle refuses, the oracle's bytes where it accepts) beside SMALL:
    the wait of the damaged batch returns its first failing frame's code, the other wait 0, and SMALL's bytes are exact (Staged.check).
    The damaged batch's statuses are also what the synchronous call reports for it."""
    bad = IF.damaged()
    with Flight(engine) as fl:
        rc_sync, s = IF.decode_sync(engine, bad)
        st_sync = s.check(rc_sync, "synchronous")
        assert rc_sync < 0
        pair = [Staged(bad), Staged(IF.small())][::1 if damaged_first else -1]
        slots = [fl.submit(s) for s in pair]
        assert set(slots) == {0, 1}
        for s, slot in list(zip(pair, slots))[::-1 if reverse else 1]:
            rc, st = fl.wait(slot)
            if s.b is bad:
                assert rc == rc_sync and np.array_equal(st, st_sync)
            else:
                assert rc == 0 and not st.any()


# ------------------------------------------------------------------------------------------------ d: slot discipline
def test_slot_discipline(engine):
    """Slots alternate, waits come in any order, and a submit whose turn is a busy context is refused although the other one is free
    (DESIGN.md says why).  A refused submit -- both busy, its turn's context busy, no frames, a missing pointer -- leaves the turn where it
    was and its buffers untouched.  zk_decode_wait on an idle slot and on slots -1 and 2 is an error.  count = 0: ZK_ERR_ARGUMENT from a
    submit (there would be nothing to wait for), 0 from the synchronous call."""
    a, b = IF.small(), IF.long_()

    def refused(batch, count=None, null_dst=False):
        s = Staged(batch)
        args = list(s.args())
        if count is not None: args[5] = count
        slot = C.c_int(-7)
        rc = zk.lib.zk_decode_submit_dev(engine._h, args[0].data_ptr(), args[1], args[2].data_ptr(), args[3].data_ptr(), args[4], args[5],
                                         None if null_dst else args[6].data_ptr(), args[7], 1, args[9].data_ptr(), C.byref(slot))
        assert rc == REFUSED and slot.value == -7
        assert bool((s.out == IF.POISON).all().item()) and bool((s.st == -1).all().item())

    with Flight(engine) as fl:
        s0, s1 = fl.submit(a), fl.submit(b)
        assert {s0, s1} == {0, 1}
        refused(a)                                               # both busy
        with pytest.raises(ZkError):
            engine.decode_submit_dev(*Staged(a).args())          # (what the wrapper makes of it)
        assert fl.wait(s1)[0] == 0                               # in reverse order
        refused(a)                                               # the turn is s0's, which is busy; s1 is free
        assert fl.wait(s0)[0] == 0
        # nothing outstanding: the refused submits have not moved the turn
        assert fl.submit(a) == s0
        refused(a, count=0); refused(a, null_dst=True)           # argument errors with one context busy ...
        assert fl.submit(b) == s1                                # ... leave the turn too
        assert fl.wait(s0)[0] == 0 and fl.wait(s1)[0] == 0
        for slot in (s0, s1, -1, 2):                             # idle, idle, no such slot
            assert zk.lib.zk_decode_wait(engine._h, slot) == REFUSED
            with pytest.raises(ZkError):
                engine.decode_wait(slot)
        refused(a, count=0)                                      # idle engine, and it still is afterwards
        assert fl.submit(a) == s0 and fl.wait(s0)[0] == 0
        s = Staged(a)
        args = list(s.args()); args[5] = 0
        assert engine.decode_frames_dev(*args) == 0              # the synchronous call with no frames: 0, nothing written
        assert bool((s.out == IF.POISON).all().item()) and bool((s.st == -1).all().item())
    # after all of it: a synchronous decode and a Decoder read
    good = next(x for x in GOLDENS if x.name == "text_100B_frames")
    out, st = engine.decode_frames(good.comp + b"\0" * 8, *good.offsets(), verify=True)
    assert out == good.input() and not st.any()
    table = SeekTable.new()
    for cs, ds in good.frames: table.log_frame(cs, ds)
    assert DecodeOptions(good.comp + table.to_bytes()).engine(engine).into_decoder().read_to_end() == good.input()


# ------------------------------------------------------------------------------------------------ e: the contract table
@pytest.mark.parametrize("state", IF.STATES)
def test_contract_table_row_by_row(engine, made, state):
    """Every row of the table above zk_decode_submit_dev while context 0, context 1 or both hold a submitted batch (160 frames of 640 KiB:
    long enough to be still running for the first rows).  refused: ZK_ERR_ARGUMENT, the call's output buffers as they were, for the two
    host-pointer forms that stage (zk_frame_content_sizes, zk_read_ranges) and for zk_read_ranges_dev zk_engine_ranges_frames_decoded as
    it was.  served: the result of the same call with nothing in flight -- the input's bytes, the twin's, zko.xxh64's.  Either way the busy
    contexts stay busy and the batches' results are exact after their waits (Flight).  Recorded, not asserted: how long the calls took
    against how long the waits behind them still had to wait -- a refusal that came after the batch would leave the wait nothing to do."""
    rows = IF.contract_rows(engine)
    with Flight(engine) as fl:
        fl.reach(state, made["big"])
        spent = []
        for row in rows:
            t0 = IF.clock()
            rc, served, untouched = row.run()
            spent.append((row.name, row.verdict[state], IF.clock() - t0))
            if row.verdict[state] == "refused":
                assert rc == REFUSED, (row.name, state, rc)
                untouched()
            else:
                assert rc == 0, (row.name, state, rc)
                served()
            assert set(fl.live) == IF.BUSY[state]
            for slot in (0, 1):                                  # (and the engine agrees: an idle context has nothing to wait for)
                if slot not in fl.live: assert zk.lib.zk_decode_wait(engine._h, slot) == REFUSED, row.name
        fl.waited = 0.0
        fl.wait_all()
        print(state, "zk_decode_wait behind the calls: %.0f us" % (fl.waited * 1e6))
        for name, verdict, dt in spent: print("  %-8s %8.0f us  %s" % (verdict, dt * 1e6, name))


@pytest.mark.parametrize("state", IF.STATES)
def test_refusals_of_the_staging_forms_come_at_once(engine, made, state):
    """zk_frame_content_sizes and zk_read_ranges (host pointers) staged through the engine's buffers, on context 0's queue, before they
    asked whether context 0 was free: the refusal came once the batch it was refused for had finished.  Called first thing behind the
    submits here; the hard assertions are the code, the untouched outputs and the counter (contract_rows); the time each refusal took and the
    time the wait behind them still needed are printed."""
    rows = [r for r in IF.contract_rows(engine) if r.name in ("zk_frame_content_sizes", "zk_read_ranges", "zk_decode_frames_prefix", "zk_read_ranges_dev")]
    assert len(rows) == 4
    with Flight(engine) as fl:
        fl.reach(state, made["big"])
        for row in rows:
            t0 = IF.clock()
            rc, served, untouched = row.run()
            dt = IF.clock() - t0
            if row.verdict[state] == "refused":
                assert rc == REFUSED, row.name
                untouched()
            else:
                assert rc == 0, row.name
                served()
            print(state, row.name, row.verdict[state], "%.0f us" % (dt * 1e6))
        fl.waited = 0.0
        fl.wait_all()
        print(state, "zk_decode_wait behind them: %.0f us" % (fl.waited * 1e6))


FSZ = 65536


@pytest.fixture(scope="module")
def seekable(engine):
    text = zko.gen_chunks(32 * FSZ, 41)
    comp, frames = engine.encode_frames(np.frombuffer(text, np.uint8), FSZ, 1, True)
    table = SeekTable.new()
    for c, d in frames: table.log_frame(c, d)
    return text, comp + table.to_bytes()


@pytest.mark.parametrize("state", IF.STATES)
def test_decoder_handles_keep_their_state(engine, seekable, state):
    """zk_decoder_* handles opened before the submits.  A read that needs a submission fails with the engine's error (ZK_ERR_IO, "invalid
    argument", as every engine failure reaches a handle) whichever context is busy, and leaves offset, cache, read-ahead and the
    submission counter as they were; seeks are the handle's own and go on working; a read the cache can serve is served, and one that
    begins in the cache delivers what the cache holds.  After the waits the same reads return the right bytes, the cached frames without
    a new submission."""
    text, src = seekable
    total = len(text)
    fresh = DecodeOptions(src).engine(engine).into_decoder()
    fresh.set_offset(5 * FSZ + 100); fresh.set_offset_limit(5 * FSZ + 200)
    ahead = DecodeOptions(src).engine(engine).batch_bytes(16 * FSZ).into_decoder()
    ahead.set_offset(4 * FSZ)
    assert ahead.decompress(bytearray(FSZ)) == FSZ and ahead.decompress(bytearray(10)) == 10     # frames 5 .. 20 are decoded ahead (tests/test_gpu_seeks.py)
    n_fresh, n_ahead = fresh.gpu_submissions(), ahead.gpu_submissions()

    def refused(d, n):
        with pytest.raises(api.Error) as err:
            d.read(n)
        assert err.value.is_io() and "invalid argument" in str(err.value), str(err.value)

    with Flight(engine) as fl:
        fl.reach(state, IF.small(), IF.long_())
        refused(fresh, 100)
        assert fresh.offset() == 5 * FSZ + 100 and fresh.offset_limit() == 5 * FSZ + 200 and fresh.gpu_submissions() == n_fresh
        fresh.set_offset_limit(total)
        assert fresh.seek(api.SeekFrom.Start, 7 * FSZ + 3) == 7 * FSZ + 3
        refused(fresh, 100)
        assert fresh.offset() == 7 * FSZ + 3 and fresh.gpu_submissions() == n_fresh
        # the handle with frames 5 .. 20 in its cache: served from it, refused beyond it.  (Its seeks stay inside the cache: one that leaves it
        # drops the read-ahead by itself, decode.rs:408-410)
        ahead.set_offset(9 * FSZ + 5); ahead.set_offset_limit(9 * FSZ + 305)
        assert ahead.read(1000) == text[9 * FSZ + 5:9 * FSZ + 305]
        ahead.set_offset_limit(total)
        ahead.set_offset(21 * FSZ - 50)                          # the cache's last 50 bytes, then frame 21, which is not in it
        assert ahead.read(200) == text[21 * FSZ - 50:21 * FSZ] and ahead.offset() == 21 * FSZ
        refused(ahead, 150)
        assert ahead.offset() == 21 * FSZ and ahead.gpu_submissions() == n_ahead
        fl.wait_all()
    assert fresh.read(100) == text[7 * FSZ + 3:7 * FSZ + 103] and fresh.gpu_submissions() == n_fresh + 1
    ahead.set_offset(12 * FSZ); ahead.set_offset_limit(12 * FSZ + 300)
    assert ahead.read(1000) == text[12 * FSZ:12 * FSZ + 300] and ahead.gpu_submissions() == n_ahead       # the refusals left the read-ahead alone
    ahead.set_offset_limit(total); ahead.set_offset(21 * FSZ)
    assert ahead.read(150) == text[21 * FSZ:21 * FSZ + 150] and ahead.gpu_submissions() == n_ahead + 1


def test_profiling_around_a_submitted_pair(engine):
    """zk_engine_set_profiling(1) around a submit / wait pair changes nothing (per-kernel events belong to the synchronous call); a
    synchronous decode afterwards reports finite, non-negative times, and positive ones for the kernels every verified batch runs."""
    try:
        with Flight(engine) as fl:
            engine.set_profiling(True)
            s0, s1 = fl.submit(IF.small()), fl.submit(IF.long_())
            assert fl.wait(s0)[0] == 0 and fl.wait(s1)[0] == 0
            rc, s = IF.decode_sync(engine, IF.small())
            s.check(rc)
            n = zk.lib.zk_engine_kernel_count()
            ms = (C.c_float * n)()
            assert zk.lib.zk_engine_kernel_times(engine._h, ms, n) == 0
            times = {zk.lib.zk_engine_kernel_name(k).decode(): float(ms[k]) for k in range(n)}
            print(times)
            assert all(np.isfinite(v) and v >= 0 for v in times.values()), times
            for name in ("zk_k_walk(count)", "zk_k_scan", "zk_k_walk(fill)", "zk_k_huf", "zk_k_fse", "zk_k_exec", "zk_k_xxh64", "zk_k_status"):
                assert times[name] > 0, (name, times)
    finally:
        engine.set_profiling(False)


def test_destroy_completes_outstanding_batches():
    """zk_engine_destroy with both contexts busy: the batches are completed first (their buffers hold the results; the return codes are lost)."""
    e = zk.Engine()
    a, b = Staged(IF.small()), Staged(IF.long_())
    try:
        assert {e.decode_submit_dev(*a.args()), e.decode_submit_dev(*b.args())} == {0, 1}
    finally:
        e.close()
    a.check(0, "destroyed"); b.check(0, "destroyed")


# ------------------------------------------------------------------------------------------------ f: with a dictionary
def test_two_unequal_spans_and_a_frame_list_against_a_dictionary(engine):
    """The trained dictionary of tests/golden/dict_archives.* (formatted: it lends tables, repeat offsets and content): two unequal spans of
    its case in flight -- tests/helpers/gen_batches.py has frames against its own dictionaries only --, in both wait orders; then
    zk_decode_frame_list_dev, synchronous, beside a batch on context 1."""
    import torch
    from test_gpu_dict import CASES, dict_bytes, expected
    comp, c, d, data = expected(CASES["trained"])
    n = len(c) - 1
    sizes = list(zip(np.diff(c.astype(np.int64)).tolist(), np.diff(d.astype(np.int64)).tolist()))
    batch = IF._batch("dict_trained", comp, sizes, [data[int(d[i]):int(d[i + 1])] for i in range(n)])
    third = max(1, n // 3)
    assert third != n - third
    rng = np.random.RandomState(5)
    ids = np.concatenate([rng.permutation(n), rng.randint(0, n, 9)]).astype(np.uint32)
    oo = np.concatenate([[0], np.cumsum((d[1:] - d[:-1])[ids])]).astype(np.uint64)
    listed = b"".join(data[int(d[i]):int(d[i + 1])] for i in ids)
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(IF.dev())
    d_oo = torch.from_numpy(oo.view(np.int64).copy()).to(IF.dev())
    with Flight(engine) as fl:
        engine.set_dictionary(zk.Dictionary(dict_bytes("trained")))
        for reverse in (False, True):
            spans = [Staged(batch, 0, third), Staged(batch, third, n - third)]
            slots = [fl.submit(s) for s in spans]
            assert set(slots) == {0, 1}
            for slot in slots[::-1 if reverse else 1]:
                assert fl.wait(slot, reverse)[0] == 0
        fl.reach("ctx1", Staged(batch, third, n - third), Staged(batch, 0, third))
        out, st = IF.poisoned(len(listed)), IF.minus_ones(len(ids))
        IF.settle()
        arch = IF.uploaded(batch)
        assert engine.decode_frame_list_dev(*arch, d_ids, d_oo, len(ids), out, len(listed), True, st) == 0
        got = out.cpu().numpy()
        assert not st.cpu().numpy().any() and got[:len(listed)].tobytes() == listed and (got[len(listed):] == IF.POISON).all()
        fl.wait_all()

"""The decoder's six XXH64 kernels (zeekstd_amd/csrc/zk_xxh64.h, the source hipcc compiles as part of zk_decode.hip) on the CPU: workgroup
after workgroup under tests/sim/hip_wg_emu.h, in both lane orders, with the launchers' grids (tests/sim/zk_xxh_sim.cpp), on the batches of
tests/helpers/xxh_inputs.py -- the kernels' own step sizes, ragged waves, every tail, every placement -- against the oracle's XXH64.
  The two followers (zk_k_xxh64_follow, zk_k_xxh64_follow1) hash a frame WHILE its executor writes it; which of their branches run on the
device is the dispatcher's business.  Here a SCRIPT stands in the executor's place: per frame the XCD it runs on, the steps in which its
bytes become final, whether and when it aborts or falls silent.  Bytes that are not yet published hold poison, so a wave that reads ahead
of a progress word finds a wrong hash; every scripted case asserts the exact words the followers leave.  The emulated clock moves with
the wave's polls, and a poll counter bounds every run: a kernel that would spin fails its test.
  The same under AddressSanitizer + UBSan as a program of its own (tests/sim/xxh_san.cpp), every buffer an exact heap allocation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import zko
from helpers import xxh_inputs as X

V, M, A = X.PROG_VERIFIED, X.PROG_MISMATCH, X.PROG_ABORT
BATCHES = {k: X.batches(k) for k in X.KERNELS}


def test_the_helper_knows_the_kernels_constants():
    """xxh_inputs' copies of ZK_XXW, the lean and follow widths, ZK_XF_CHUNK, D and ZK_FOLLOW_PATIENCE, the progress word's bits and the
    status a wrong checksum gets are the header's; the plans name the kernels the batches are built for."""
    c = X.consts()
    assert c[:6] == [X.ZK_XXW, X.ZK_XXL, X.ZK_FOLLOW_W, X.ZK_XF_CHUNK, X.ZK_XF_DEPTH, X.ZK_FOLLOW_PATIENCE]
    assert [1 << (c[6] >> s & 255) for s in (0, 8, 16)] == [A, V, M] and c[7] == X.CHECKSUM_WRONG
    assert [X.step_bytes(k) for k in ("wide", "lean", "follow", "frame", "follow1", "fed4")] == [1536, 768, 448, 1024, 1024, 1024]
    assert [X.pass_plan(100, ch, False) for ch in (0, 1, 2, 3, 5)] == ["frame", "frame", "wide", "lean", "fed4"]
    assert [X.pass_plan(100, ch, True) for ch in (0, 4, 2)] == ["fed4", "fed4", "wide"]
    assert [X.follow_plan(n) for n in (1, 8, 9, 32, 33, 128, 129)] == [("follow1", 8), ("follow1", 8), ("follow1", 16), ("follow1", 32), ("follow", 8), ("follow", 8), ("follow", 16)]


@pytest.mark.parametrize("kernel", list(X.KERNELS))
def test_the_batches_are_the_edges_they_claim(kernel):
    """every batch's facts (least, common, leftover stripes, tails, which frames begin on a 16-byte boundary) on the helper's model of
    the kernel's split alone; and the lengths and counts the batches are to cover are there"""
    bs = BATCHES[kernel]
    for b in bs:
        X.check_facts(b)
    u = X.step_bytes(kernel)
    lens = {x for b in bs for x in b.lens}
    assert set(X.edge_lengths(u)) <= lens and max(lens) <= 40 << 10
    # (16 KiB holds every length but the ring's: the issue's own U = 13 x 1 KiB with 3 U - 1 is 39 935 bytes, and one frame of each
    #  ring group is a chunk of 1 KiB longer than its neighbours)
    assert {1, 15, 17, 65} <= {b.count for b in bs} and {(b.start, b.align) for b in bs} >= {(s, a) for s in (0, 1, 4097) for a in (0, 1, 8, 15)}
    m = [w for b in bs for w in X.model(kernel, b.lens)]
    if X.KERNELS[kernel][1] > 1:          # the batched loop runs on mixed lengths, with leftovers for some lanes only
        assert any(w.common > 0 and len(set(w.leftover)) > 1 and min(w.leftover) == 0 for w in m)
    if kernel == "fed4":
        assert {w.common // 32 for w in m} >= set(X.FED_CHUNKS) and {b.count % 4 for b in bs} == {0, 1, 2, 3}


def test_known_answer():
    """XXH64 of the 2 MiB text is 0xAD0311EAAD1ED582 -- the oracle's and every pass's"""
    text = zko.gen_text(2 << 20, 0x5EED0002)
    assert zko.xxh64(text) == 0xAD0311EAAD1ED582
    for k in X.PASSES:
        b = X.Batch("kat", k, [len(text)], align=0)
        b._data = np.frombuffer(text, np.uint8)
        h, _ = X.sim_pass(k, b)
        assert int(h[0]) == 0xAD0311EAAD1ED582, k


@pytest.mark.parametrize("kernel", X.PASSES)
def test_passes_hash_every_batch(kernel):
    """hashes only (infos == nullptr): every frame's hash is the oracle's, in both lane orders; once behind three entries of the offset
    table the kernel must not read (first = 3)"""
    for b in BATCHES[kernel]:
        for desc in (False, True):
            h, _ = X.sim_pass(kernel, b, descending=desc)
            assert [int(x) for x in h] == b.want(), (b, desc)
    b = BATCHES[kernel][0]
    h, _ = X.sim_pass(kernel, b, first=3)
    assert [int(x) for x in h] == b.want()


def _checksums(b, wrong):
    ck = np.array([x & 0xFFFFFFFF for x in b.want()], np.uint32)
    ck[wrong] ^= np.uint32(0x00010000)
    return ck


@pytest.mark.parametrize("kernel", X.PASSES)
def test_passes_verify_every_batch(kernel):
    """the decoder form (infos; skip where the kernel takes it): ZK_E_CHECKSUM_WRONG lands exactly on the live frames whose stored
    checksum was changed; a frame that is not live -- no checksum flag, a status that is not ZK_OK, verified by a follower, a whole wave of
    them, all but the last frame -- keeps its status and its (poisoned) hash slot; every live frame's hash is right"""
    takes_skip = kernel in ("wide", "fed4")
    for b in BATCHES[kernel]:
        wrong = np.zeros(b.count, bool)
        wrong[::3] = True
        ck = _checksums(b, wrong)
        for name, st, fl, ve in X.decoder_forms(b):
            if not takes_skip and ve.any():
                st = np.where(ve == 1, 70, st).astype(np.uint32)
            live = (st == 0) & (fl == 1) & ((ve == 0) | (not takes_skip))
            skip = (ve.astype(np.uint64) * np.uint64(V) | np.uint64(5 << 32)) if takes_skip else None
            for desc in (False, True):
                h, got = X.sim_pass(kernel, b, infos=(st, fl, ck), skip=skip, descending=desc)
                assert got.tolist() == np.where(live & wrong, X.CHECKSUM_WRONG, st).tolist(), (b, name, desc)
                assert [int(x) for x in h] == [w if l else X.POISON for w, l in zip(b.want(), live)], (b, name, desc)
            # ... and without a hash buffer
            _, got = X.sim_pass(kernel, b, infos=(st, fl, ck), skip=skip, hashes=False)
            assert got.tolist() == np.where(live & wrong, X.CHECKSUM_WRONG, st).tolist(), (b, name)


# ------------------------------------------------------------------------------------------------------------------ the followers
def _follow_batch(count=128, seed=7, align=1, lens=None):
    """frames of one to three of zk_k_xxh64_follow's steps; wave c of a group of 128 takes the frames c, c + 8, ..."""
    return X.Batch(f"follow_{count}_{seed}", "follow" if count > 32 else "follow1", lens if lens is not None else X._ragged(X.step_bytes("follow"), count, seed), start=1, align=align)


def _infos(b, wrong=(), no_flag=(), bad=()):
    w = np.zeros(b.count, bool)
    w[list(wrong)] = True
    st, fl = np.zeros(b.count, np.uint32), np.ones(b.count, np.uint32)
    fl[list(no_flag)] = 0
    st[list(bad)] = 20
    return (st, fl, _checksums(b, w)), w


def _benign(b, rot=0):
    """every frame complete before the waves start, frame f on XCD (f + rot) % 8 -- where the waves expect it"""
    return [(0, f, b.lens[f], (f + rot) % 8, 0) for f in range(b.count)]


def _word(b, ev, f):
    """the frame's word as the script leaves it"""
    last = [e for e in sorted(ev, key=lambda e: e[0]) if e[1] == f]
    if not last:
        return 0
    _, _, nbytes, xcd, ab = last[-1]
    return (A if ab else 0) | (xcd + 1) << 32 | (0 if ab else nbytes)


def _expect(b, ev, infos, wrong, unmarked=()):
    """every live frame VERIFIED or MISMATCH by its checksum, but for `unmarked`; nothing else touched"""
    st, fl, _ = infos
    return [_word(b, ev, f) | (0 if f in unmarked or st[f] != 0 or fl[f] != 1 else M if wrong[f] else V) for f in range(b.count)]


def _run(b, infos, ev, wg_xcd, **kw):
    """both lane orders; no wave may be cancelled for polling beyond its patience"""
    out = []
    for desc in (False, True):
        rc, prog, polls = X.sim_follow(b, infos, ev, wg_xcd, descending=desc, **kw)
        assert rc == 0, ("a wave polled beyond the bound", polls)
        out.append(([int(x) for x in prog], polls))
    assert out[0] == out[1], "the lane order changes what the followers leave"
    return out[0]


def _wave_of(f):
    return [(f >> 7) * 128 + (f & 7) + 8 * j for j in range(16)]


@pytest.mark.parametrize("count,rot,rot2", [(128, 0, 0), (128, 3, 6), (130, 5, 1), (33, 1, 4), (257, 7, 7)])
def test_follow_benign_script(count, rot, rot2):
    """BRANCH: none of the exits.  Every frame complete, on the XCD the wave order expects (frame f on (f + rot) % 8, wave g on (g + rot2) % 8),
    no stall: every live frame with the right checksum is VERIFIED, every one with a wrong checksum MISMATCH, frames without a flag or
    with a status keep their words, and no wave polls.  (130, 257: groups of 2 and 1 frames -- waves without a frame.)"""
    b = _follow_batch(count, seed=count)
    infos, wrong = _infos(b, wrong=range(2, count, 7), no_flag=range(5, count, 11), bad=range(9, count, 13))
    ev = _benign(b, rot)
    prog, polls = _run(b, infos, ev, [(g + rot2) % 8 for g in range(X.follow_plan(count)[1])])
    assert prog == _expect(b, ev, infos, wrong) and sum(polls) == 0


@pytest.mark.parametrize("kernel", ["follow", "follow1"])
def test_followers_hash_every_batch(kernel):
    """BRANCH: none of the exits, on the batches built for the follower's own step (2 x 7 stripes; 1 KiB chunks) -- the wave shapes laid out
    by class for zk_k_xxh64_follow, which zk_xxh_follow_plan takes above 32 frames (a smaller batch goes to zk_k_xxh64_follow1 under
    either name).  Behind a script that has everything ready, and behind one that publishes a step of U per poll: every frame ends
    VERIFIED, or MISMATCH where its checksum was changed."""
    u = X.step_bytes(kernel)
    for b in BATCHES[kernel]:
        infos, wrong = _infos(b, wrong=range(1, b.count, 6))
        grid = X.follow_plan(b.count)[1]
        stepwise = [(s, f, min((s + 1) * u, b.lens[f]), (f + 5) % 8, 0) for f in range(b.count) for s in range(b.lens[f] // u + 1)]
        for ev in (_benign(b, 5), stepwise):
            prog, _ = _run(b, infos, ev, [(g + 5) % 8 for g in range(grid)])
            assert prog == _expect(b, ev, infos, wrong), b


def test_follow_first_frame_on_a_foreign_xcd():
    """BRANCH: the rotation is read from a frame that breaks the habit.  Frame 0 runs three XCDs from where the others' order puts it: every
    wave then follows a class whose executors run elsewhere (each word's XCD is checked again: not live) -- but for the wave on frame 0's
    XCD, which verifies frame 0 alone."""
    b = _follow_batch(128, seed=11)
    infos, wrong = _infos(b)
    ev = _benign(b, 2)
    ev[0] = (0, 0, b.lens[0], 5, 0)
    prog, _ = _run(b, infos, ev, list(range(8)))
    assert prog == _expect(b, ev, infos, wrong, unmarked=set(range(1, 128)))


def _long_waves(seed):
    """128 frames of four to five of zk_k_xxh64_follow's steps, none ending with a step: every wave has four double batches (1792 bytes)
    in common and every frame stripes and a tail of its own behind them"""
    lens = [4 * 448 + 32 * (1 + (f + seed) % 5) + (7 * f + seed) % 31 + 1 for f in range(128)]
    b = _follow_batch(128, seed=seed, lens=lens)
    for w in X.model("follow", lens):
        assert w.common * 32 == 4 * 448 and all(lens[f] > w.common * 32 for f in w.frames)
    return b


@pytest.mark.parametrize("case", ["foreign", "abort_before_a", "abort_at_zero_in_a", "abort_during_a", "abort_after_a"])
def test_follow_one_frame_drops_out(case):
    """BRANCHES: `live = false` in news().  Every wave has four double batches in common (_long_waves); frame F
      foreign             publishes everything from another XCD than its class's;
      abort_before_a      has ZK_PROG_ABORT in its word before the wave starts;
      abort_at_zero_in_a  publishes one stripe at step 1 and aborts at step 2, its fifteen wave-mates complete from the start: the wave
                          is in phase A with s == 0 and polls twice;
      abort_during_a      publishes ONE double batch of the four and aborts at step 2: the wave has hashed that batch, s == 14 stripes
                          < common == 56, and polls twice inside phase A;
      abort_after_a       publishes all the common stripes but not its end and aborts at step 3: the wave leaves phase A without a poll
                          and polls three times in phase B.
    That frame gets neither bit; its wave-mates -- and every other wave -- exactly what the benign script gives them, and only F's wave
    polls, exactly as often as said."""
    b = _long_waves(21)
    infos, wrong = _infos(b, wrong=[5, 29, 60])
    F, u, rot, rot2 = 21, X.step_bytes("follow"), 4, 1
    common = next(w for w in X.model("follow", b.lens) if F in w.frames).common * 32
    assert 2 * u <= common < b.lens[F]                        # one double batch is not all of phase A; the common stripes are not the frame's end
    ev = _benign(b, rot)
    xcd = (F + rot) % 8
    if case == "foreign":
        ev[F], polls_f = (0, F, b.lens[F], (xcd + 3) % 8, 0), 0
    elif case == "abort_before_a":
        ev[F], polls_f = (0, F, 0, xcd, 1), 0
    elif case == "abort_at_zero_in_a":
        ev[F], polls_f = (1, F, 32, xcd, 0), 2
        ev.append((2, F, 0, xcd, 1))
    elif case == "abort_during_a":
        ev[F], polls_f = (0, F, u, xcd, 0), 2
        ev.append((2, F, 0, xcd, 1))
    else:
        ev[F], polls_f = (0, F, common, xcd, 0), 3
        ev.append((3, F, 0, xcd, 1))
    prog, polls = _run(b, infos, ev, [(g + rot2) % 8 for g in range(8)])
    assert prog == _expect(b, ev, infos, wrong, unmarked={F})
    g_f = (F + rot - rot2) % 8                                # the wave on F's XCD
    assert polls == [polls_f if g == g_f else 0 for g in range(8)]


@pytest.mark.parametrize("case", ["before_the_first_word", "in_phase_a", "in_phase_b"])
def test_follow_silence_beyond_the_patience(case):
    """BRANCHES: the three `waited` exits.
      before_the_first_word  no word at all: every wave returns from the rotation loop and sets no bit;
      in_phase_a             frame F publishes ONE double batch of the four its wave has in common and falls silent: the wave hashes it
                             (s == 14 stripes < common == 56) and gives up in phase A's loop;
      in_phase_b             F publishes all the common stripes, not its end, and falls silent: the wave leaves phase A without a poll and
                             gives up in phase B's loop.
    F's WAVE returns and sets no bit on any of its sixteen frames; every other wave does what it does under the benign script and does
    not poll.  A wave that gives up has polled PATIENCE / TICK + 1 times behind its last news, never more (xxh_inputs.max_polls: with
    either exit missing the run is cancelled at that bound and _run fails)."""
    b = _long_waves(31)
    infos, wrong = _infos(b, wrong=[3, 70])
    F, u = 42, X.step_bytes("follow")
    give_up = X.ZK_FOLLOW_PATIENCE // X.TICK + 1
    if case == "before_the_first_word":
        prog, polls = _run(b, infos, [], list(range(8)))
        assert prog == [0] * 128 and polls == [give_up] * 8
        return
    common = next(w for w in X.model("follow", b.lens) if F in w.frames).common * 32
    assert 2 * u <= common < b.lens[F]
    ev = _benign(b, 0)
    ev[F] = (0, F, u if case == "in_phase_a" else common, F % 8, 0)
    prog, polls = _run(b, infos, ev, list(range(8)))
    assert prog == _expect(b, ev, infos, wrong, unmarked=set(_wave_of(F)))
    assert polls == [give_up if g == F % 8 else 0 for g in range(8)]


def test_follow_progress_in_uneven_steps():
    """BRANCH: `upto` behind the slowest executor, step after step.  Every frame becomes final in steps of its own -- one stripe, U - 32,
    U, several U at once, everything at once -- so that the sixteen frames of a wave are never equally far.  Everything is VERIFIED in
    the end: a wave that read a byte before its word announced it would have hashed poison (MISMATCH)."""
    b = _follow_batch(128, seed=41, lens=[3 * 448 + 32 * (f % 5) + f % 32 for f in range(128)])
    infos, wrong = _infos(b, wrong=[17])
    u, ev = 448, []
    plans = [[32, u - 32, u, 3 * u], [u, 10 ** 9], [10 ** 9], [32, 64, 2 * u + 32], [u - 32, u + 32, 2 * u - 32, 2 * u]]
    for f in range(128):
        p = plans[f % 5]
        for s, x in enumerate(p):
            ev.append((s + f % 3, f, min(x, b.lens[f]), f % 8, 0))
        ev.append((len(p) + f % 3 + 1, f, b.lens[f], f % 8, 0))
    prog, polls = _run(b, infos, ev, list(range(8)))
    assert prog == _expect(b, ev, infos, wrong) and min(polls) > 0


@pytest.mark.parametrize("count", [1, 7, 8, 9, 32])
def test_follow1_groups(count):
    """zk_k_xxh64_follow1, BRANCHES: a group of fewer than eight frames (lanes beyond `count` neither pending nor mine; the waves whose
    XCD has no frame return: `!mm`), full groups, a second group of one.  Frames become final in uneven steps across the 1 KiB chunks
    (wait_for): all live frames end VERIFIED / MISMATCH by their checksums."""
    lens = [X.edge_lengths(1024)[(3 * f + count) % 14] for f in range(count)]
    b = _follow_batch(count, lens=lens)
    infos, wrong = _infos(b, wrong=range(1, count, 4), no_flag=range(3, count, 9))
    ev = []
    for f in range(count):
        steps = sorted({min(x, lens[f]) for x in (32, 1024 - 32, 1024, 2048 + 5, 10 ** 9)}) if f % 2 else [lens[f]]
        ev += [(s + f % 3, f, x, (f + 3) % 8, 0) for s, x in enumerate(steps)]
    grid = X.follow_plan(count)[1]
    prog, _ = _run(b, infos, ev, [(g + 3) % 8 for g in range(grid)])
    assert prog == _expect(b, ev, infos, wrong)


def test_follow1_two_waves_on_one_xcd_and_none():
    """BRANCHES: `(g & 7) % popc(mm)` with two waves of a group on one XCD -- both hash the same frame (the second atomicOr changes nothing)
    and the frame whose XCD got no wave stays unmarked; a wave on an XCD where no frame of its group runs returns at once (`!mm`); a
    frame that aborts while its wave waits for its second chunk, and one on an XCD twice, of which wave k takes number k mod 2."""
    lens = [2048 + 17, 1024, 3000, 40, 0, 5000, 1025, 2047]
    b = _follow_batch(8, lens=lens)
    infos, wrong = _infos(b, wrong=[2])
    # frames 0 ... 7 on XCDs 0 1 2 3 4 5 5 7 (two frames on XCD 5, none on 6); waves on XCDs 0 0 2 3 4 5 5 6
    fx = [0, 1, 2, 3, 4, 5, 5, 7]
    ev = [(0, f, lens[f], fx[f], 0) for f in range(8)]
    ev[3] = (0, 3, 32, 3, 0)
    ev.append((2, 3, 0, 3, 1))                                # frame 3 aborts mid-way
    prog, _ = _run(b, infos, ev, [0, 0, 2, 3, 4, 5, 5, 6])
    # frame 1 (XCD 1: no wave) and frame 7 (XCD 7: no wave) unmarked, frame 3 aborted; waves 5 and 6 on XCD 5 take frames 5 (5 % 2 = 1 -> the second: 6) and 6 (6 % 2 = 0 -> 5)
    assert prog == _expect(b, ev, infos, wrong, unmarked={1, 3, 7})


def test_follow1_silence():
    """BRANCHES: a word of the group that never speaks (`pending` beyond the patience: every wave of the group returns), and a frame that
    falls silent between two chunks (wait_for's own patience): no bit for it, its neighbours unaffected."""
    lens = [1500, 4096, 2048, 3100]
    b = _follow_batch(4, lens=lens)
    infos, wrong = _infos(b)
    ev = [(0, f, lens[f], f, 0) for f in (0, 1, 3)]
    prog, polls = _run(b, infos, ev, list(range(8)))
    assert prog == _expect(b, ev, infos, wrong, unmarked={0, 1, 2, 3}) and polls == [X.ZK_FOLLOW_PATIENCE // X.TICK + 1] * 8
    ev = [(0, f, lens[f], f, 0) for f in (0, 2, 3)] + [(0, 1, 2048, 1, 0)]
    prog, polls = _run(b, infos, ev, list(range(8)))
    assert prog == _expect(b, ev, infos, wrong, unmarked={1}) and polls[1] == X.ZK_FOLLOW_PATIENCE // X.TICK + 1


def test_a_wave_that_polls_too_often_is_cancelled():
    """the poll bound itself: with a bound below what the patience needs the run is cancelled and says so (what a kernel that spins would get)"""
    b = _follow_batch(4, lens=[100, 200, 300, 400])
    infos, _ = _infos(b)
    rc, _, polls = X.sim_follow(b, infos, [], list(range(8)), limit=2)
    assert rc == 1 and polls[0] == 3


def _random_script(r, b):
    n = b.count
    rot = int(r.randint(8))
    st, fl = np.zeros(n, np.uint32), np.ones(n, np.uint32)
    wrong = r.rand(n) < 0.15
    fl[r.rand(n) < 0.1] = 0
    st[r.rand(n) < 0.1] = 20
    ev, fate = [], []
    for f in range(n):
        xcd = (f + rot) % 8 if r.rand() < 0.85 else int(r.randint(8))
        kind = r.choice(["complete", "abort", "silent", "never"], p=[0.8, 0.08, 0.08, 0.04])
        cuts = sorted({int(x) for x in r.randint(0, b.lens[f] + 1, r.randint(0, 4))} | ({b.lens[f]} if kind == "complete" else set()))
        if kind in ("abort", "silent"):
            cuts = [c for c in cuts if c < b.lens[f]] or [0]
        step = int(r.randint(3))
        if kind != "never":
            for c in cuts:
                ev.append((step, f, c, xcd, 0))
                step += int(r.randint(3))
            if kind == "abort":
                ev.append((step + 1, f, 0, xcd, 1))
        fate.append((kind, xcd))
    grid = X.follow_plan(n)[1]
    wg = [(g + int(r.randint(8))) % 8 for g in range(grid)] if r.rand() < 0.3 else [(g + rot + (0 if r.rand() < 0.7 else 1)) % 8 for g in range(grid)]
    return (st, fl, _checksums(b, wrong)), wrong, ev, fate, wg


def test_random_scripts():
    """PROPERTY, a few hundred seeded scripts over both followers (frames on expected and foreign XCDs; complete, aborting, silent or never
    starting executors; waves dealt round the XCDs, shifted, or at random): no run is cancelled; a frame is VERIFIED only if it is live,
    its checksum right and its executor completed it without an abort -- never from bytes that were not final --, MISMATCH only with a
    wrong checksum; and behind the follower the pass the engine runs (zk_xxh_plan(count, k, skip = true): zk_k_xxh64_fed<4>, or
    zk_k_xxh64_wide when pinned) leaves every frame's final status right whatever the script did."""
    r = np.random.RandomState(0x22E)
    pool = [_follow_batch(n, seed=n, align=a) for n, a in ((40, 0), (128, 15), (131, 8))] + \
           [_follow_batch(n, lens=[int(x) for x in np.random.RandomState(n).randint(0, 4200, n)], align=n % 16) for n in (1, 5, 8, 13, 32)]
    followed = 0
    for i in range(300):
        b = pool[i % len(pool)] if i % 3 else pool[3 + i % 5]
        infos, wrong, ev, fate, wg = _random_script(r, b)
        st, fl, ck = infos
        rc, prog, _ = X.sim_follow(b, infos, ev, wg, descending=bool(i & 1))
        assert rc == 0, i
        for f in range(b.count):
            w = int(prog[f])
            live = st[f] == 0 and fl[f] == 1
            assert (w & ~(V | M)) == _word(b, ev, f), (i, f)
            if w & V:
                assert live and not wrong[f] and fate[f][0] == "complete", (i, f, fate[f])
            if w & M:
                assert live and wrong[f] and fate[f][0] == "complete", (i, f, fate[f])
            followed += bool(w & V)
        # the executors are done: a frame that aborted has a status of its own by now
        st2 = np.where([k == "abort" for k, _ in fate], 20, st).astype(np.uint32)
        kernel = X.pass_plan(b.count, 2 if i % 4 == 0 else 4, True)
        _, got = X.sim_pass(kernel, b, infos=(st2, fl, ck), skip=prog, hashes=False, descending=bool(i & 2))
        assert got.tolist() == np.where((st2 == 0) & (fl == 1) & wrong, X.CHECKSUM_WRONG, st2).tolist(), i
    assert followed > 1000


# ------------------------------------------------------------------------------------------------------------------ sanitizers
def test_kernels_under_sanitizers(tmp_path):
    """The same kernels under the emulator, built with AddressSanitizer + UBSan (tests/sim/xxh_san.cpp, a program of its own): every batch
    of every pass with hashes only and in the decoder form, and a dozen scripts for the followers.  The frames' bytes, the offsets, infos,
    hashes and words are heap allocations of exactly their sizes, so "a lane without a frame reads frame 0", "the last round reads the
    first batch again" and the 16-byte loads are held against the buffers' real ends; the program also compares every result."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "xxhsan")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wno-attributes", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         os.path.join(X.SIM, "xxh_san.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    jobs = []
    for k in X.PASSES:
        for b in BATCHES[k]:
            jobs.append(X.pack_job(b, k, expect_hash=b.want()))
            wrong = np.zeros(b.count, bool)
            wrong[::3] = True
            ck = _checksums(b, wrong)
            for name, st, fl, ve in X.decoder_forms(b)[1:]:
                if k not in ("wide", "fed4"):
                    st = np.where(ve == 1, 70, st).astype(np.uint32)
                live = (st == 0) & (fl == 1) & ((ve == 0) | (k not in ("wide", "fed4")))
                skip = (ve.astype(np.uint64) * np.uint64(V)) if k in ("wide", "fed4") else None
                jobs.append(X.pack_job(b, k, infos=(st, fl, ck), skip=skip, expect_status=np.where(live & wrong, X.CHECKSUM_WRONG, st)))
    # the scripts: benign, a foreign frame, aborts, silences and uneven steps for zk_k_xxh64_follow; groups and a doubled XCD for _follow1
    r = np.random.RandomState(5)
    for n, align in ((128, 1), (130, 15), (33, 0), (1, 8), (7, 15), (9, 1), (32, 0)):
        b = _follow_batch(n, seed=n, align=align)
        infos, wrong = _infos(b, wrong=range(1, n, 5))
        ev = _benign(b, 2)
        grid = X.follow_plan(n)[1]
        jobs.append(X.pack_job(b, None, infos=infos, events=ev, wg_xcd=[(g + 2) % 8 for g in range(grid)], expect_progress=_expect(b, ev, infos, wrong)))
    for i in range(6):
        b = _follow_batch((128, 40, 8, 13, 131, 5)[i], seed=50 + i, align=(0, 1, 8, 15, 7, 3)[i])
        infos, wrong, ev, fate, wg = _random_script(r, b)
        _, prog, _ = X.sim_follow(b, infos, ev, wg)
        jobs.append(X.pack_job(b, None, infos=infos, events=ev, wg_xcd=wg, expect_progress=prog))
    p = str(tmp_path / "jobs")
    with open(p, "wb") as f:
        f.write(b"".join(jobs))
    run = subprocess.run([exe, p], capture_output=True, text=True, timeout=900)
    if run.returncode != 0 and "AddressSanitizer" in run.stderr and "ERROR: AddressSanitizer:" not in run.stderr:
        pytest.skip("the sanitizer runtime cannot start here")
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert f"{len(jobs)} jobs" in run.stdout

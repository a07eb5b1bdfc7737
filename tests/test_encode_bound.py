"""zk_compress_bound() against what the encoder can write -- on the CPU twin (oracle/zstd_oracle_enc.c), whose frames the GPU encoder's are
compared with byte for byte in tests/test_gpu_encode_bound.py.  The host pipeline sizes its device output buffer by this bound and switches the
fit check off, so a bound that is one byte short for some input is an out-of-bounds write on the device.

Checked here, for every input of tests/helpers/enc_bound_inputs.py and for a seeded sweep of a thousand small frames:
  per frame      len(frame) <= d + 10 + 3 * (ceil(frame_size / 1024) + 8)          (the bound's per-frame term)
  summed         total <= zk_compress_bound(n, frame_size)                          (the library's own function)
  per block      Block_Size <= Block_Maximum_Size = min(Window_Size, 128 KiB)       (RFC 8878 3.1.1.2.3, the window read from the frame)
  the facts each input is there for, and that the oracle decoder and libzstd give the input back.
DESIGN.md 5.2f has the argument; what is observed rather than proven is the slack of frames below 37 889 bytes that have 256 or more
sequences (tables of their own), where the descriptions could in principle outweigh the spare block headers.

Observed on the twin (printed by the tests, asserted nowhere): the smallest per-frame slack under the bound is 24 bytes -- every frame of at
most 1024 bytes that is stored raw: the 3 * 8 spare block headers -- in the entries and in the sweep alike.  Among frames with tables of
their own the smallest is 771 bytes (def_outgrows/single/fs=3072/l1; 830 in the sweep): 256 sequences save far more than the descriptions
cost.  The largest def_outgrows is +51 (def_outgrows/fs=100000/l1)."""
import numpy as np
import pytest

from helpers import enc_bound_inputs as B
from helpers import enc_inputs as E
from oracle import zko
from oracle import libzstd_ref as Z

MIB = 1 << 20


def bound(n, frame_size):
    """zk_compress_bound restated (zk_engine_enc.hip): per frame the header (6), the checksum (4) and a 3-byte header for every block there
    can be -- blocks are at least 1 KiB except in frames below that, + 8 -- and 16 bytes on top"""
    if frame_size == 0:
        return 0
    nf = 1 if n == 0 else -(-n // frame_size)
    return n + nf * (6 + 4 + 3 * (-(-frame_size // 1024) + 8)) + 16


def frame_allowance(frame_size):
    return 10 + 3 * (-(-frame_size // 1024) + 8)


def lib_bound(n, frame_size):
    import zeekstd_amd as zk
    return int(zk.lib.zk_compress_bound(n, frame_size))


# ---------------------------------------------------------------------------------------------- the formula
FRAME_SIZES = (1, 1024, 1025, 2 * MIB, 1 << 31, (1 << 32) - 1)


def test_bound_formula_on_the_grid():
    for fs in FRAME_SIZES:
        ns = sorted({0, 1, fs - 1, fs, fs + 1, (1 << 32) - 1, 1 << 32, 1 << 40})
        got = [lib_bound(n, fs) for n in ns]
        for n, g in zip(ns, got):
            want = bound(n, fs)
            assert want < 1 << 64, "the grid stays inside 64 bits"
            assert g == want, (n, fs, g, want)                      # equal to the unbounded integers' value: nothing wrapped
            assert g >= n + 10 + 3 * 9 + 16
        assert got == sorted(got), ("non-decreasing in n", fs)
        # ... and across a frame boundary byte by byte
        for k in (1, 2, 1000):
            if k * fs < 1 << 41:
                around = [lib_bound(k * fs + x, fs) for x in (-1, 0, 1, 2) if k * fs + x >= 0]
                assert around == sorted(around), (k, fs)


def test_bound_of_frame_size_zero_is_zero():
    for n in (0, 1, 1 << 32, 1 << 40):
        assert lib_bound(n, 0) == 0


def test_restated_helpers_match_the_encoder():
    """block_max() of the helper is the twin's block size: the frames of the all_raw entries have exactly ceil(d / block_max(d)) blocks (asserted
    in defining_growth for every frame walked); here the values at the edges, and 16 -> 32 KiB at 512 KiB"""
    assert [B.block_max(d) for d in (1, 1024, 1025, 2048, 2049, 4096, 4097, 65536, 131071, 131072, 262144, 524287, 524288, 2 * MIB)] == \
        [1024, 1024, 2048, 2048, 4096, 4096, 4096, 4096, 4096, 8192, 16384, 16384, 32768, 32768]
    f = zko.frame_encode(zko.gen_random(5000, 1), 1, True)
    assert B.window_size(f) == 8192
    assert B.window_size(zko.frame_encode(b"", 1, True)) == 0          # Single_Segment, Frame_Content_Size 0


def test_the_arithmetic_of_the_argument():
    """a frame is at most d + 10 + 3 per block + (descriptions - 1), and the bound leaves 3 * (ceil(fs / 1024) + 8 - blocks) spare.
    Blocks are at least 4 KiB in frames above 4 KiB (a frame shorter than frame_size may have MORE blocks than a whole one -- 131 071 bytes
    are 32 blocks of 4 KiB, 131 072 are 16 of 8 KiB -- but never more than ceil(fs / 4096)), so from 37 889 bytes on the spare block headers
    alone cover the largest descriptions at accuracy log 6 (108 bytes), and from 65 536 on those at 9 / 8 / 9 (150 bytes; 16 384 sequences
    regenerate at least 4 bytes each)."""
    fs = np.arange(1, 1 << 21, dtype=np.int64)
    spare = 3 * (-(-fs // 1024) + 8 - np.maximum(1, -(-fs // 4096)))
    desc6 = sum(-(-(4 + 7 * nsym) // 8) for nsym in (36, 32, 53))
    desc9 = sum(-(-(4 + (al + 1) * nsym) // 8) for nsym, al in ((36, 9), (32, 8), (53, 9)))
    assert (desc6, desc9) == (108, 150)
    assert spare.min() == 24
    assert (spare[37889 - 1:] >= desc6 - 1).all() and spare[37888 - 1] < desc6 - 1
    assert (spare[65536 - 1:] >= desc9 - 1).all()
    for f in (1, 1024, 4096, 4097, 70000, 131072, 600000, 2 * MIB):
        assert max(-(-d // B.block_max(d)) for d in range(max(1, f - 9000), f + 1)) <= max(1, -(-f // 4096)), f
    assert -(-131071 // B.block_max(131071)) == 32 and -(-131072 // B.block_max(131072)) == 16


# ---------------------------------------------------------------------------------------------- every frame
def check_sizes(e, frames):
    """the bound per frame and summed, and the block rule; returns the smallest per-frame slack"""
    ds = B.frame_lengths(e)
    assert len(frames) == len(ds), e.name
    slack = None
    for i, (f, d) in enumerate(zip(frames, ds)):
        room = d + frame_allowance(e.frame_size) - len(f)
        assert room >= 0, (e.name, "frame", i, len(f), d)
        slack = room if slack is None else min(slack, room)
        bmax = min(B.window_size(f), 128 << 10)
        for k, b in enumerate(E.walk_frame(f)):
            assert b["size"] <= bmax, (e.name, "frame", i, "block", k, b["size"], bmax)
    total = sum(len(f) for f in frames)
    assert total <= lib_bound(len(e.data), e.frame_size), (e.name, total)
    assert total <= bound(len(e.data), e.frame_size)
    return slack


def check_roundtrip(e, frames):
    pos = 0
    for f, d in zip(frames, B.frame_lengths(e)):
        out, used = zko.frame_decode(f, d, True)
        assert used == len(f) and out == e.data[pos:pos + d], (e.name, pos)
        pos += d
    assert pos == len(e.data)
    if Z.load("system") is not None:
        assert Z.decode_stream(b"".join(frames), len(e.data), "system") == e.data, e.name


@pytest.mark.parametrize("name", B.NAMES)
def test_entry_stays_under_the_bound(name, capsys):
    e = B.get(name)
    assert len(e.data) <= 2 * MIB
    frames = B.twin_frames(e)
    slack = check_sizes(e, frames)
    facts = B.reached(frames, e)
    assert e.features <= facts, (name, sorted(e.features - facts))
    check_roundtrip(e, frames)
    grows = sorted(f for f in facts if f.startswith("def_outgrows"))
    with capsys.disabled():
        print(f"\n  {name} (level {e.level}, {len(e.data)} bytes in frames of {e.frame_size}): smallest slack {slack}; "
              + ", ".join(sorted(e.features) + [g for g in grows if g not in e.features]), end="")


def test_all_raw_frames_are_input_plus_headers():
    """the fact spelled out: a frame of random bytes is d + 6 (magic, descriptor, window) + 3 per block + 4 (checksum), and 4 less without"""
    for fs in (1, 1024, 1025, 4097, 65537):
        e = B.get(f"all_raw/fs={fs}")
        for checksum in (True, False):
            for f, d in zip(B.twin_frames(e, checksum), B.frame_lengths(e)):
                assert len(f) == d + 6 + 3 * max(1, -(-d // B.block_max(d))) + (4 if checksum else 0), (fs, d)


def test_largest_outgrow_is_the_recorded_one():
    got = max(int(f.split("+")[1]) for name in B.NAMES for f in B.get(name).features if f.startswith("def_outgrows=+"))
    assert got == B.DEF_OUTGROWS_MAX


# ---------------------------------------------------------------------------------------------- a sweep
def test_sweep_of_small_near_raw_frames(capsys):
    """A thousand seeded draws: one frame of 1..20000 bytes (half of the sizes uniform, half log-uniform) of random bytes with 1, 2, 50, 260, 280,
    330, 600 or 2000 planted matches of 5, 6 or 8 bytes, levels 1 and 3 in turn.  The assertion is the bound and the block rule; the
    smallest slack is printed.  Observed: 24 bytes (raw frames of at most 1024 bytes), and 830 among the 68 frames with tables of their own."""
    rng = np.random.default_rng(20240607)
    smallest, smallest_tabled, tabled = None, None, 0
    for i in range(1000):
        fs = int(rng.integers(1, 20001)) if i % 2 else int(np.exp(rng.uniform(0, np.log(20000))))
        count = int(rng.choice((1, 2, 50, 260, 280, 330, 600, 2000), p=(0.1, 0.1, 0.15, 0.15, 0.15, 0.15, 0.1, 0.1)))
        length = int(rng.choice((5, 6, 8)))
        level = 1 if i % 4 < 2 else 3
        data = B.planted(fs, 5000 + i, [(count, length, 0, fs, 0)], reach=int(rng.choice((64, 1024, 20000))))
        e = B.Entry(f"sweep/{i}/fs={fs}/l{level}/{count}x{length}", data, fs, level, frozenset())
        frames = B.twin_frames(e)
        slack = check_sizes(e, frames)
        smallest = slack if smallest is None else min(smallest, slack)
        if B.defining_growth(frames[0], fs) is not None:
            tabled += 1
            smallest_tabled = slack if smallest_tabled is None else min(smallest_tabled, slack)
        if i % 50 == 0:
            check_roundtrip(e, frames)
    assert tabled >= 50, "the sweep reaches frames with tables of their own"
    with capsys.disabled():
        print(f"\n  sweep: smallest slack under the per-frame bound {smallest} bytes; among the {tabled} frames with their own tables {smallest_tabled}", end="")

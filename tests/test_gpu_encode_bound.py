"""What the encoder's kernels write, and where: zk_compress_bound() and dst_cap are the encoder's memory-safety contract.

Every device case encodes into a tensor of cap + 4096 bytes filled with 0xA5, with d_dst `lead` bytes into it; after the call everything outside
[lead, lead + written) must still be 0xA5 -- the tail handling of zk_k_enc_assemble / zke_copy_wg (16-byte vector stores + per-lane tails, the
five-stream copy) decides the last byte written, and a refused call (-70) must not have written at all.  The inputs are those of
tests/helpers/enc_bound_inputs.py (frames that are input plus headers, blocks that hover around "compressed is smaller", defining blocks that
outgrow their input, thousands of tiny frames, the empty input); tests/test_encode_bound.py holds the bound itself against the CPU twin on a
machine without a GPU.

After a refusal (-70) the contents of d_c_sizes / d_d_sizes are unspecified (zk_k_enc_sizes has run: today they hold the sizes the frames would
have had) and nothing here asserts them.  On the host-pointer route a refused call may have written below dst_cap when the output travels in
pieces (the sink copies piece by piece and refuses the one that does not fit); nothing is written at or beyond dst_cap.

No test here tries to provoke the race the second-queue wait in zk_encode_enqueue closes (the checksum kernel reading the caller's source
after -70 has come back): that fix was made by reading.  What is tested is that the engine is whole after a refusal: the next encode on the same
engine, checksums on and off, equals the twin."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import enc_bound_inputs as B
from oracle import zko
from test_gpu_encode import check_payload

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 4096
DST_TOO_SMALL = -70

TEXT = B.Entry("text/300k", zko.gen_text(300000, 21), 70000, 3, frozenset({"frames=5", "block=comp"}))
NO_CHECKSUM = ("all_raw/fs=1", "all_raw/fs=4097", "all_raw/fs=524289", "near_raw/tie/fs=4096/l1", "near_raw/fs=65536/l3/600x6",
               "def_outgrows/fs=8192/l1", "def_outgrows/fs=65536/l1", "many_tiny/64", "many_tiny/1", "empty")


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _entry(name):
    return TEXT if name == TEXT.name else B.get(name)


@functools.lru_cache(maxsize=None)
def twin(name, checksum=True):
    """the twin's frames of an entry, encoded once per session"""
    return tuple(B.twin_frames(_entry(name), checksum))


def bound_of(e):
    import zeekstd_amd as zk
    return int(zk.lib.zk_compress_bound(len(e.data), e.frame_size))


class Encoded:
    pass


def dev_encode(engine, e, checksum=True, cap=None, lead=0, src_off=0):
    """One zk_encode_frames_dev call into a poisoned tensor -> rc, frames, sizes, and the bytes of the whole tensor"""
    import zeekstd_amd as zk
    torch, dev = _torch()
    n = len(e.data)
    nf = max(1, -(-n // e.frame_size))
    cap = bound_of(e) if cap is None else cap
    assert lead < GUARD
    buf = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device=dev)
    src = torch.zeros(n + src_off + 64, dtype=torch.uint8, device=dev)
    if n:
        src[src_off:src_off + n] = torch.from_numpy(np.frombuffer(e.data, np.uint8).copy()).to(dev)
    d_cs = torch.zeros(nf, dtype=torch.int32, device=dev)
    d_ds = torch.zeros(nf, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    r = Encoded()
    r.rc, r.nf, r.written = 0, 0, 0
    try:
        r.nf, r.written = engine.encode_frames_dev(src.data_ptr() + src_off, n, e.frame_size, e.level, checksum, buf.data_ptr() + lead, cap, d_cs, d_ds)
    except zk.ZkError as ex:
        r.rc = ex.code
    torch.cuda.synchronize()
    r.lead, r.cap = lead, cap
    r.all = buf.cpu().numpy()
    r.c_sizes = d_cs.cpu().numpy().astype(np.int64)
    r.d_sizes = d_ds.cpu().numpy().astype(np.int64)
    assert bytes(src[src_off:src_off + n].cpu().numpy()) == e.data, "the source is the caller's: untouched"
    return r


def assert_clean_outside(r, what):
    """everything outside [lead, lead + written) is still poison"""
    assert r.written <= r.cap, what
    outside = np.concatenate([r.all[:r.lead], r.all[r.lead + r.written:]])
    bad = np.flatnonzero(outside != POISON)
    assert bad.size == 0, (what, "stray write", int(bad[0]) + (0 if bad[0] < r.lead else r.written), "written", r.written, "lead", r.lead)


def frames_of(r, e):
    assert r.rc == 0 and r.nf == len(B.frame_lengths(e)), (e.name, r.rc, r.nf)
    assert int(r.c_sizes.sum()) == r.written and int(r.d_sizes.sum()) == len(e.data), e.name
    assert r.d_sizes.tolist() == B.frame_lengths(e), e.name
    comp = r.all[r.lead:r.lead + r.written].tobytes()
    pairs = list(zip(r.c_sizes.tolist(), r.d_sizes.tolist()))
    return comp, pairs, B.split_frames(comp, pairs)


def assert_equals_twin(r, e, checksum=True):
    comp, pairs, got = frames_of(r, e)
    want = twin(e.name, checksum)
    assert len(got) == len(want), e.name
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (e.name, "frame", i, len(g), len(w))
    return comp, pairs, got


def assert_refused(r, what):
    assert r.rc == DST_TOO_SMALL, (what, r.rc)
    bad = np.flatnonzero(r.all != POISON)
    assert bad.size == 0, (what, "a refused call wrote at", int(bad[0]) - r.lead, "of", r.cap)


# ---------------------------------------------------------------------------------------------- dst_cap == bound
def _at_the_bound(engine, name, checksum):
    e = B.get(name)
    r = dev_encode(engine, e, checksum, lead=5)
    comp, pairs, got = assert_equals_twin(r, e, checksum)
    assert_clean_outside(r, name)
    facts = B.reached(got, e)                                       # read from what the kernels wrote
    assert e.features <= facts, (name, sorted(e.features - facts))
    assert r.written <= bound_of(e)
    check_payload(engine, e.data, comp, pairs, e.frame_size, checksum)


@pytest.mark.parametrize("name", B.NAMES)
def test_entry_at_the_bound(engine, name):
    _at_the_bound(engine, name, True)


@pytest.mark.parametrize("name", NO_CHECKSUM)
def test_entry_at_the_bound_without_checksum(engine, name):
    _at_the_bound(engine, name, False)


# ---------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("name", ["all_raw/fs=4097", TEXT.name])
def test_bytes_do_not_depend_on_alignment(engine, name):
    """d_dst 0, 1, 3, 13 bytes and d_src 0, 1, 7 bytes off a 256-byte boundary: the vector copies' heads and tails"""
    e = _entry(name)
    for lead in (0, 1, 3, 13):
        for src_off in (0, 1, 7):
            r = dev_encode(engine, e, True, lead=lead, src_off=src_off)
            assert_equals_twin(r, e)
            assert_clean_outside(r, (name, lead, src_off))
    if name == TEXT.name:
        comp, pairs, got = frames_of(r, e)
        assert e.features <= B.reached(got, e)
        check_payload(engine, e.data, comp, pairs, e.frame_size, True)


# ---------------------------------------------------------------------------------------------- dst_cap == written
@pytest.mark.parametrize("name", ["all_raw/fs=4097", "def_outgrows/fs=8192/l1", "def_outgrows/fs=65536/l1", "def_outgrows/fs=100000/l3", "many_tiny/64",
                                  "many_tiny/1", TEXT.name])
def test_exactly_fitting_destination(engine, name):
    """cap below the bound, so zk_enc_fit_check decides: exactly the written size fits, and the byte behind it is not touched"""
    e = _entry(name)
    total = sum(len(f) for f in twin(name))
    assert total < bound_of(e)
    for lead in (0, 3):
        r = dev_encode(engine, e, True, cap=total, lead=lead)
        assert r.written == total
        assert_equals_twin(r, e)
        assert_clean_outside(r, (name, lead))


# ---------------------------------------------------------------------------------------------- dst_cap too small
def _too_small_caps(name):
    fr = twin(name)
    total = sum(len(f) for f in fr)
    return {"one_short": total - 1, "inside_frame_1": len(fr[0]) + len(fr[1]) // 2, "one_byte": 1, "zero": 0}


@pytest.mark.parametrize("checksum", [True, False], ids=["checksum", "no_checksum"])
@pytest.mark.parametrize("kind", ["one_short", "inside_frame_1", "one_byte", "zero"])
@pytest.mark.parametrize("name", ["all_raw/fs=4097", TEXT.name])
def test_too_small_destination_is_refused_unwritten(engine, name, kind, checksum):
    """-70 and not one byte written -- the total decides before anything is written -- for a destination one byte short, one that ends inside
    frame 1, one of a single byte and one of none (dst_cap is not validated as an argument: 0 is a destination that is too small, -70).  The
    refused call has checksums on (the second queue is in use when it returns); straight after it, on the same engine, another input encodes
    to the twin's bytes with checksums on and off."""
    e = _entry(name)
    assert len(twin(name)) >= 3
    cap = _too_small_caps(name)[kind]
    r = dev_encode(engine, e, True, cap=cap, lead=3)
    assert_refused(r, (name, kind, cap))
    nxt = B.get("def_outgrows/fs=8192/l1" if name != TEXT.name else "near_raw/fs=65536/l3/600x6")
    r2 = dev_encode(engine, nxt, checksum, lead=1)
    assert_equals_twin(r2, nxt, checksum)
    assert_clean_outside(r2, ("after", name, kind))


def test_refusal_without_checksums(engine):
    """the same refusal with nothing on the second queue"""
    e = B.get("all_raw/fs=4097")
    total = sum(len(f) for f in twin(e.name, False))
    assert_refused(dev_encode(engine, e, False, cap=total - 1), "no checksum, one short")
    r = dev_encode(engine, e, False, cap=total)
    assert_equals_twin(r, e, False)
    assert_clean_outside(r, "no checksum, exact")


# ---------------------------------------------------------------------------------------------- host pointers
def host_encode(engine, data, frame_size, level, cap, room):
    """zk_encode_frames into a numpy destination of `room` bytes of poison, told it has `cap` -> (rc, written, frames as (c, d), the destination)"""
    import zeekstd_amd as zk
    n = len(data)
    nf = max(1, -(-n // frame_size))
    src = np.frombuffer(data, np.uint8)
    dst = np.full(room, POISON, np.uint8)
    cs, ds = np.zeros(nf, np.uint32), np.zeros(nf, np.uint32)
    nfo, wr = C.c_uint32(), C.c_uint64()
    rc = zk.lib.zk_encode_frames(engine._h, src.ctypes.data, n, frame_size, level, 1, dst.ctypes.data, cap, cs.ctypes.data, ds.ctypes.data, nf,
                                 C.byref(nfo), C.byref(wr))
    return rc, wr.value, list(zip(cs[:nfo.value].tolist(), ds[:nfo.value].tolist())), dst


HOST_CASES = {
    "small/all_raw": lambda: (B.get("all_raw/fs=4097").data, 4097, 1),
    "small/text": lambda: (TEXT.data, TEXT.frame_size, TEXT.level),
    "pieces/random_6mib": lambda: (zko.gen_random(6 << 20, 9), 1 << 20, 1),             # beyond 4 MiB the output comes back in pieces
}


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_host_destination_with_a_guard(engine, case):
    import zeekstd_amd as zk
    data, fs, level = HOST_CASES[case]()
    want = [zko.frame_encode(data[o:o + fs], level, True) for o in range(0, len(data), fs)]
    total = sum(len(f) for f in want)
    room = int(zk.lib.zk_compress_bound(len(data), fs)) + GUARD
    assert total < room - GUARD
    # one byte short: refused, nothing at or beyond dst_cap (below it the pieces route may have delivered pieces)
    rc, _, _, dst = host_encode(engine, data, fs, level, total - 1, room)
    assert rc == DST_TOO_SMALL, rc
    assert (dst[total - 1:] == POISON).all(), case
    # the follow-up call, exactly fitting: the twin's bytes, and the guard intact
    rc, written, frames, dst = host_encode(engine, data, fs, level, total, room)
    assert rc == 0 and written == total, (rc, written, total)
    assert dst[:total].tobytes() == b"".join(want), case
    assert (dst[total:] == POISON).all(), case
    assert [c for c, _ in frames] == [len(f) for f in want]
    # ... and with the whole bound
    rc, written, _, dst = host_encode(engine, data, fs, level, room - GUARD, room)
    assert rc == 0 and written == total and dst[:total].tobytes() == b"".join(want) and (dst[total:] == POISON).all(), case

"""The tail every decode shares (segment scratch, the checksum follower's prepare / fork / finish, executor + checksums:
zk_dec_exec_checksums, zk_engine.hip) crossed over its entries -- zk_decode_frames on the small path, zk_decode_frames through the
general pipeline, zk_decode_frames_dev -- at the smallest shapes that reach every branch: three checksummed frames of 200 000, 1 and
70 000 bytes (a frame of several segments at 4 KiB per segment, and a single byte), the executor per frame and in segments, the
checksums behind the executor and beside it.  What the reference does with the same bytes: lib/src/decode.rs:242-256.

zk_engine_checksums_followed is set by zk_decode_finish (the device-pointer entries); the host-pointer entries leave it alone, both of
them alike -- that is what the comparison below holds on to."""
import itertools

import numpy as np
import pytest

import zeekstd_amd as zk
from conftest import offsets_from_frames
from helpers import dict_fixtures as df
from helpers.dev_decode import dev as _dev, upload as _upload
from oracle import zko
from oracle import libzstd_ref as Z

pytestmark = pytest.mark.gpu

SIZES = [200000, 1, 70000]
VARIANTS = [dict(exec_seg=s, seg_kib=4, xxh64=x) for s, x in itertools.product((1, 2), (1, 4))]
IDS = [f"seg{v['exec_seg']}_xxh{v['xxh64']}" for v in VARIANTS]
ENTRIES = ("small", "pipeline", "dev")


@pytest.fixture(scope="module")
def archive():
    """(input, compressed frames back to back, c_off, d_off, the same with one bit of the last frame's stored checksum flipped)"""
    data = zko.gen_chunks(sum(SIZES), 1618)
    comp, frames, pos = bytearray(), [], 0
    for n in SIZES:
        c, f = Z.encode_seekable_frames(data[pos:pos + n], n, 1, True)
        assert len(f) == 1
        comp += c
        frames += f
        pos += n
    c_off, d_off = offsets_from_frames(frames)
    bad = bytearray(comp)
    bad[-2] ^= 0x10                                      # the Content_Checksum is the frame's last four bytes
    return data, bytes(comp), c_off, d_off, bytes(bad)


@pytest.fixture
def choice(engine):
    engine.set_kernel_choice(reset=0)
    yield engine
    engine.set_dictionary(None)
    engine.set_kernel_choice(reset=0)


def decode(engine, entry, variant, comp, c, d):
    """-> (bytes, per-frame statuses, zk_engine_checksums_followed behind the call)"""
    import torch
    engine.set_kernel_choice(reset=0)
    engine.set_kernel_choice(**variant)
    if entry == "dev":
        n, total = len(c) - 1, int(d[-1])
        arch = _upload(comp, c, d)
        out = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device=_dev())
        st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
        engine.decode_frames_dev(arch[0], arch[1], arch[2], arch[3], 0, n, out, total, True, st)
        torch.cuda.synchronize()
        return out[:total].cpu().numpy().tobytes(), st.cpu().numpy().tolist(), engine.checksums_followed()
    engine.set_kernel_choice(small_path=0 if entry == "small" else 1)
    out, st = engine.decode_frames(comp + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    return out, st.tolist(), engine.checksums_followed()


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_intact_archive_through_every_entry(choice, archive, variant):
    data, comp, c, d, _ = archive
    got = {entry: decode(choice, entry, variant, comp, c, d) for entry in ENTRIES}
    for entry, (out, st, _) in got.items():
        assert st == [0, 0, 0], entry
        assert out == data, entry
    assert got["small"][2] == got["pipeline"][2]
    if variant["xxh64"] == 1:
        assert got["dev"][2] == 0                        # the pass behind the executor took every frame
    else:
        assert got["dev"][2] <= len(SIZES)


def test_damaged_checksum_gets_one_verdict(choice, archive):
    data, _, c, d, bad = archive
    verdicts = {}
    for variant, name in zip(VARIANTS, IDS):
        for entry in ENTRIES:
            out, st, _ = decode(choice, entry, variant, bad, c, d)
            verdicts[(name, entry)] = st
            assert out[:int(d[2])] == data[:int(d[2])], (name, entry)
    first = verdicts[(IDS[0], ENTRIES[0])]
    assert first[:2] == [0, 0] and first[2] != 0
    assert all(st == first for st in verdicts.values()), verdicts


def test_content_sizes(choice, archive):
    _, comp, c, _, _ = archive
    sizes, st = choice.frame_content_sizes(comp, c)
    assert sizes.tolist() == SIZES and not st.any()


def test_dictionary_batch_leaves_the_small_path(choice, archive):
    """<= 64 frames from host memory with a dictionary set: zk_host_decode hands them to the general pipeline (the small path's walk
    knows no dictionary) -- the same bytes as the device entry gives"""
    idx, blob = df.load()
    case = next(k for k in idx["cases"] if k["name"] == "mixed")
    comp, c, d = df.archive(blob, case)
    c, d = np.asarray(c, np.uint64), np.asarray(d, np.uint64)
    want = b"".join(df.plain(fr["recipe"]) for fr in case["frames"])
    choice.set_dictionary(zk.Dictionary(df.piece(blob, idx["dicts"][case["dict"]])))
    variant = dict(exec_seg=2, seg_kib=4, xxh64=4)
    small = decode(choice, "small", variant, comp, c, d)
    dev = decode(choice, "dev", variant, comp, c, d)
    assert small[1] == dev[1] == [0] * len(case["frames"])
    assert small[0] == dev[0] == want

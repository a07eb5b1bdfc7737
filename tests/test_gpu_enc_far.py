"""The encoder's far-history kernels (zeekstd_amd/csrc/zk_enc_far.h) on the GPU, on the inputs that tests/test_sim_enc_far.py holds them
to entry by entry on the CPU (tests/helpers/enc_far_inputs.py: window edges, frame starts and tails, segment seams, crowded chunks, byte
runs, launch shapes on both sides of the XCD remap, slices, short last frames, every dense level): the engine's frames are byte-identical
to the CPU twin's (oracle/zstd_oracle_enc.c) and decode back through the oracle, libzstd and the GPU decoder.  What the reference does here
is ZSTD_compressStream2 frame by frame (lib/src/encode.rs:340-346); compressed bytes are unpinned by it, so the twin is the yardstick."""
import functools

import pytest

from helpers import enc_far_inputs as I
from helpers import enc_far_sim as S
from oracle import zko
from test_gpu_encode import check_payload

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _twin(name, level, checksum):
    e = I.get(name)
    return b"".join(zko.frame_encode(e.data[o:o + e.frame_size], level, checksum) for o in range(0, len(e.data), e.frame_size))


def _equals_twin(engine, data, frame_size, level, checksum, prefix=None):
    comp, frames = engine.encode_frames(data, frame_size, level, checksum, prefix=prefix)
    pos = dpos = 0
    for c, d in frames:
        assert comp[pos:pos + c] == zko.frame_encode(data[dpos:dpos + d], level, checksum, prefix=prefix), (level, checksum, dpos)
        pos += c; dpos += d
    assert pos == len(comp) and dpos == len(data)
    return comp, frames


@pytest.mark.parametrize("name", I.NAMES)
def test_far_inputs_equal_twin_and_decode(engine, name):
    """every input at its levels, checksums on and off: the twin's bytes, frame by frame, and the input back out of them; the launch shapes
    also in slices of one and of three frames (set_kernel_choice(enc_dense_slice_kib=...))"""
    e = I.get(name)
    try:
        for level in e.levels:
            for checksum in (False, True):
                want = _twin(name, level, checksum)
                for sl in e.slices:
                    engine.set_kernel_choice(enc_dense_slice_kib=-(-sl // 1024))
                    comp, frames = engine.encode_frames(e.data, e.frame_size, level, checksum)
                    sizes = S.frame_sizes(len(e.data), e.frame_size)
                    assert [d for _, d in frames] == sizes
                    if comp != want:                                    # which frame
                        _equals_twin(engine, e.data, e.frame_size, level, checksum)
                    assert comp == want, (level, checksum, sl)
                    if sl == 0:
                        check_payload(engine, e.data, comp, frames, e.frame_size, checksum)
    finally:
        engine.set_kernel_choice(enc_dense_slice_kib=0)


def test_scratch_carried_over_between_calls():
    """one engine, one call after the other over the scratch the engine keeps (candidates, sorted positions, pass offsets, sampled tables;
    nothing of it is cleared between calls): 1.2 MiB at a dense level, 200 KB of other bytes at a dense level (the stale candidates of the
    first call lie behind and under it), level 2 (the sampled table only), a prefix beyond the ring's reach (the table over the prefix in
    the same buffer), and the first call again -- each equal to the twin"""
    import zeekstd_amd as zk
    big = zko.gen_chunks(1200 << 10, 21)
    small = zko.gen_text(100000, 22) * 2
    prefix = I.prefixes()["mod4=3"]
    new = prefix[500:30000] + zko.gen_text(4000, 23) + prefix[-20000:]
    eng = zk.Engine(0)
    try:
        first, _ = _equals_twin(eng, big, 400001, 3, True)
        _equals_twin(eng, small, 1 << 21, 9, False)
        _equals_twin(eng, big[:700000], 300000, 2, True)
        _equals_twin(eng, new, 1 << 21, 3, True, prefix=prefix)
        again, _ = _equals_twin(eng, big, 400001, 3, True)
        assert again == first
    finally:
        eng.close()


@pytest.mark.parametrize("level", [2, 3])
def test_sampled_table_inputs_equal_twin_and_decode(engine, level):
    """the in-frame sampled-table inputs -- two frames of different sizes per call (300 003 + 70 001, 300 003 + 57 281, 70 001 + 57 281 bytes),
    each with its own zke_ldm_log inside the call's common stride -- at level 2 (the sampled table alone) and 3 (with the dense candidates on
    top), checksums off and on: the twin's bytes, and the input back"""
    for name, data, fs in I.ldm_frames_inputs():
        for checksum in (False, True):
            comp, frames = _equals_twin(engine, data, fs, level, checksum)
            assert [d for _, d in frames] == S.frame_sizes(len(data), fs), name
            check_payload(engine, data, comp, frames, fs, checksum)


@pytest.mark.parametrize("level", [1, 3])
def test_prefix_table_inputs_equal_twin(engine, level):
    """the prefixes of the sampled-table test (every length mod 4, one byte beyond the ring's reach, a last sampled position at the very end)
    as the prefix of an encode whose input repeats their start, their middle and their last bytes: the twin's bytes, and the input back"""
    from conftest import offsets_from_frames
    for name, prefix in I.prefixes().items():
        new = prefix[100:20000] + zko.gen_text(3000, 31) + prefix[30000:45000] + prefix[-3000:]
        comp, frames = _equals_twin(engine, new, 1 << 21, level, True, prefix=prefix)
        c_off, d_off = offsets_from_frames(frames)
        out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True, prefix=prefix)
        assert not st.any() and out == new, name

"""The encoder's entropy stage on the device (zk_k_enc_fse_build, zk_k_enc_entropy, zk_k_enc_sizes, zk_k_enc_assemble) at the format's
literal and table edges: the inputs of tests/helpers/enc_inputs.py, each with the facts it is there for.  Per entry, checksum on: the
GPU's frames equal the CPU twin's byte for byte, decode with the oracle, libzstd and the GPU decoder (check_payload), and the facts
are read from the GPU's OWN frames with the block walker -- the coverage claim rests on what the kernels wrote.
tests/test_encode_edges.py holds the same facts against the twin on a machine without a GPU."""
import pytest

from conftest import offsets_from_frames
from helpers import enc_inputs as E
from oracle import zko
from test_gpu_encode import check_payload

pytestmark = pytest.mark.gpu

# the per-block-table decode kernels pinned, and the small-batch path: these read the tables and streams the encoder wrote another way
PINNED = ("lit_huf_5byte", "huf_depth_limit", "seq_over_4096/level1", "seq_over_4096/level3", "lit_rle/level1", "lit_rle/level3", "lit_none")
CHOICES = ({"fse_own": 1}, {"fse_own": 2}, {"small_path": 1})


def encode_and_check(engine, e):
    comp, frames = engine.encode_frames(e.data, e.frame_size, e.level, True)
    got = E.split_frames(comp, frames)
    want = E.twin_frames(e)
    assert len(got) == len(want), e.name
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (e.name, "frame", i)
    check_payload(engine, e.data, comp, frames, e.frame_size, True)
    facts = E.reached(got)
    assert e.features <= facts, (e.name, sorted(e.features - facts))
    return comp, frames


@pytest.mark.parametrize("name", E.NAMES)
def test_entry(engine, name):
    e = E.get(name)
    comp, frames = encode_and_check(engine, e)
    if name in PINNED:
        c_off, d_off = offsets_from_frames(frames)
        try:
            for choice in CHOICES:
                engine.set_kernel_choice(reset=0)
                engine.set_kernel_choice(**choice)
                out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True)
                assert not st.any() and out == e.data, (name, choice)
        finally:
            engine.set_kernel_choice(reset=0)


@pytest.mark.parametrize("many", [False, True], ids=["single", "40_frames"])
def test_huffman_edge_sweep(engine, many):
    """Every frame size from 56 to 200 and 1022 to 1026 bytes of match-free literals: the 63 / 64 gate and the 1023 / 1024 header edge.  As
    single frames, and as 40 frames per call, where one entropy workgroup holds 16 such blocks of 16 different frames."""
    for e in E.huf_edge_sweep(many):
        encode_and_check(engine, e)

"""The inputs of tests/helpers/enc_inputs.py reach what they claim -- on the CPU twin (oracle/zstd_oracle_enc.c), whose frames the GPU
encoder's are compared with byte for byte in tests/test_gpu_encode_edges.py.  Every entry is encoded frame by frame, the frames are
walked (RFC 8878 3.1.1.2 / 3.1.1.3) and the entry's facts must be among those read from them; the oracle decoder and libzstd must
give the input back.  This is the guard that keeps the GPU test from silently losing a path when the matcher changes: the facts fail
here first, on a machine without a GPU."""
import pytest

from helpers import enc_inputs as E
from oracle import zko
from oracle import libzstd_ref as Z


def check_entry(e, frames):
    """facts + round trip of an entry's frames; returns the facts that were asked for (all of them hold)"""
    facts = E.reached(frames)
    assert e.features <= facts, (e.name, sorted(e.features - facts))
    pos = 0
    for f in frames:
        d = min(e.frame_size, len(e.data) - pos)
        out, used = zko.frame_decode(f, d, True)
        assert used == len(f) and out == e.data[pos:pos + d], (e.name, pos)
        pos += d
    assert pos == len(e.data)
    if Z.load("system") is not None:
        assert Z.decode_stream(b"".join(frames), len(e.data), "system") == e.data, e.name
    return sorted(e.features)


@pytest.mark.parametrize("name", E.NAMES)
def test_input_reaches_its_facts(name, capsys):
    e = E.get(name)
    assert len(e.data) <= (1 << 20) + (64 << 10)
    got = check_entry(e, E.twin_frames(e))
    with capsys.disabled():
        print(f"\n  {name} (level {e.level}, {len(e.data)} bytes in frames of {e.frame_size}): " + ", ".join(got), end="")


@pytest.mark.parametrize("many", [False, True], ids=["single", "40_frames"])
def test_huffman_edge_sweep(many, capsys):
    """lit_huf_edges at every size from 56 to 200 and 1022 to 1026: raw below 64 bytes, Huffman from 64 on, the 3-byte header up to 1023
    literals and the 4-byte one from 1024 on -- with no sequence in the block, so that nlit is the frame's size."""
    kinds = set()
    for e in E.huf_edge_sweep(many):
        got = check_entry(e, E.twin_frames(e))
        kinds.update(g.split("/nlit=")[0] for g in got)
    assert kinds == {"block=raw", "lit=huf/sf=1", "lit=huf/sf=2"}
    with capsys.disabled():
        print(f"\n  lit_huf_edges/{'40x' if many else ''}n for n in 56..200, 1022..1026: block=raw below 64, lit=huf/sf=1/nlit=n/nseq=0 up to 1023, "
              "lit=huf/sf=2/nlit=n/nseq=0 from 1024", end="")


def test_the_three_huffman_header_forms_occur():
    forms = set()
    for name in ("lit_huf_edges/tail16383", "lit_huf_edges/tail16384"):
        for f in E.twin_frames(E.get(name)):
            forms.update(b["sf"] for b in E.walk_frame(f) if b.get("lit") == "huf")
    forms.update(b["sf"] for e in E.huf_edge_sweep() if len(e.data) in (1023,) for f in E.twin_frames(e) for b in E.walk_frame(f))
    assert forms == {1, 2, 3}


def test_walker_reads_what_the_decoder_counts():
    """the walker against the oracle decoder's own statistics on a frame with every block and literal type"""
    e = E.get("lit_none")
    f = E.twin_frames(e)[0]
    blocks = E.walk_frame(f)
    _, _, st = zko.frame_decode(f, len(e.data), True, want_stats=True)
    comp = [b for b in blocks if b["type"] == "comp"]
    assert (st.n_blocks, st.n_comp) == (len(blocks), len(comp))
    assert st.n_seq == sum(b["nseq"] for b in comp)
    assert (st.lit_raw, st.lit_rle, st.lit_huf4) == tuple(sum(1 for b in comp if b["lit"] == t) for t in ("raw", "rle", "huf"))
    assert E.huffman_depth([1, 1, 2, 4, 8, 16]) == 5 and E.huffman_depth([5, 5, 5, 5]) == 2

"""The batches of tests/helpers/xxh_inputs.py -- frames at the XXH64 kernels' own step sizes, ragged waves, every tail, every placement; the
facts that make them edges are asserted in tests/test_sim_xxh64.py -- on the device: through zk_xxh64_frames_dev under every kernel it can
take, and as archives through decode_frames_dev(verify=True) under every checksum pass and under the followers.  No test asks for a
particular number of followed frames: that is the dispatcher's business (the followers' branches are driven in tests/test_sim_xxh64.py)."""
import numpy as np
import pytest

from oracle import zko
from helpers import xxh_inputs as X

pytestmark = pytest.mark.gpu

BATCHES = [b for k in X.KERNELS for b in X.batches(k)]


def test_every_batch_under_every_kernel(engine):
    """zk_xxh64_frames_dev under ZK_CHOICE_XXH64 = 0 (by shape), 1 zk_k_xxh64, 2 _wide, 3 _lean, 5 _fed<4> against the oracle's XXH64: the
    batch's first byte at its alignment modulo 16 inside a larger (poisoned) tensor, its table beginning at off[0] = 0, 1 or 4097, the
    hash buffer poisoned before every call"""
    import torch
    dev = torch.device("cuda", 0)
    big = torch.empty((64 << 10) + max(sum(b.lens) + b.start for b in BATCHES), dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 16 == 0
    try:
        for b in BATCHES:
            k = 16 + (b.align - b.start) % 16                   # (view + off[0]) % 16 == align
            view = big[k:]
            n = sum(b.lens)
            big.fill_(0xEE)
            view[b.start:b.start + n] = torch.from_numpy(b.data().copy()).to(dev)
            assert (view.data_ptr() + b.start) % 16 == b.align
            d_off = torch.from_numpy(b.off().view(np.int64)).to(dev)
            d_h = torch.empty(b.count, dtype=torch.int64, device=dev)
            for choice in (0, 1, 2, 3, 5):
                engine.set_kernel_choice(reset=0)
                engine.set_kernel_choice(xxh64=choice)
                d_h.fill_(0x5A5A5A5A5A5A5A5A)
                engine.xxh64_frames_dev(view, d_off, b.count, d_h)
                assert [int(x) for x in d_h.cpu().numpy().view(np.uint64)] == b.want(), (b, choice)
    finally:
        engine.set_kernel_choice(reset=0)


@pytest.mark.parametrize("kernel", X.PASSES)
def test_the_decoder_form(engine, kernel):
    """Frames of the kernel's edge lengths and wave shapes from zko.frame_encode, with and without a Content_Checksum interleaved, some
    stored checksums changed; decode_frames_dev(verify=True) under ZK_CHOICE_XXH64 = 1, 2, 3, 5 (the passes behind the executor) and 4
    (the followers, then the pass that takes what they left): status 22 exactly where a checksum was changed, every byte right, and
    under 4 at most the intact checksummed frames count as followed."""
    import torch
    dev = torch.device("cuda", 0)
    names = ("edge_lengths", "equal_waves", "shortest_in_lane_group", "least_a_multiple", "least_zero_among_long", "count_17")
    lens = [x for b in X.batches(kernel) if b.name in names for x in b.lens]
    text = zko.gen_text(sum(lens), 0xE0 + len(lens))
    at = np.concatenate([[0], np.cumsum(lens)])
    srcs = [text[int(at[i]):int(at[i + 1])] for i in range(len(lens))]
    checksummed = [i % 3 != 1 for i in range(len(lens))]
    changed = [checksummed[i] and i % 7 == 3 for i in range(len(lens))]
    frames = []
    for i, s in enumerate(srcs):
        f = bytearray(zko.frame_encode(s, 1, checksummed[i]))
        if changed[i]:
            f[-2] ^= 0x10                                       # in the stored Content_Checksum
        frames.append(bytes(f))
    comp = b"".join(frames)
    c = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    d = at.astype(np.uint64)
    nf, total = len(lens), int(at[-1])
    d_comp = torch.from_numpy(np.frombuffer(comp + b"\0" * 64, np.uint8).copy()).to(dev)
    d_c, d_d = torch.from_numpy(c.view(np.int64)).to(dev), torch.from_numpy(d.view(np.int64)).to(dev)
    d_want = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    d_st = torch.empty(nf, dtype=torch.int32, device=dev)
    want_st = [22 if x else 0 for x in changed]
    intact = sum(1 for i in range(nf) if checksummed[i] and not changed[i])
    try:
        for choice in (1, 2, 3, 5, 4):
            engine.set_kernel_choice(reset=0)
            engine.set_kernel_choice(xxh64=choice)
            d_out.fill_(0xEE)
            d_st.fill_(-1)
            rc = engine.decode_frames_dev(d_comp, len(comp), d_c, d_d, 0, nf, d_out, total, True, d_st)
            assert rc < 0, (choice, rc)                         # (frames with a changed checksum are in the batch)
            assert d_st.cpu().numpy().tolist() == want_st, choice
            assert torch.equal(d_out[:total], d_want), choice
            if choice == 4:
                assert engine.checksums_followed() <= intact
    finally:
        engine.set_kernel_choice(reset=0)

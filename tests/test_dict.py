"""zk_dict_create (include/zeekstd_amd.h): a zstd dictionary parsed and validated on the host -- no GPU.  Checked against what libzstd 1.5.7
said about the same bytes when tools/make_dict_goldens.py made tests/golden/dict_archives.*: ZDICT_getDictID / ZDICT_getDictHeaderSize for the
dictionaries, ZSTD_DCtx_loadDictionary / ZSTD_decompress_usingDict for the damaged ones.  Where that libzstd is loadable the fixtures are
decoded with it again, so that they cannot go stale unnoticed."""
import ctypes as C

import pytest

import zeekstd_amd as zk
from oracle import libzstd_ref, zko
from tests.helpers import dict_fixtures as df

IDX, BLOB = df.load()


def dict_bytes(name):
    ent = IDX["dicts"][name]
    if "of" in ent:
        return df.patch_reps(dict_bytes(ent["of"]), ent["header_size"], ent["reps"])
    return df.piece(BLOB, ent)


@pytest.mark.parametrize("name", sorted(IDX["dicts"]))
def test_id_and_content_offset_are_what_zdict_reports(name):
    ent = IDX["dicts"][name]
    d = zk.Dictionary(dict_bytes(name))
    assert d.id == ent["id"]                                 # ZDICT_getDictID (0: raw content)
    assert d.content_offset == ent["header_size"]            # ZDICT_getDictHeaderSize (0: every byte is content)


@pytest.mark.parametrize("ent", IDX["dict_verdicts"], ids=lambda e: e["name"])
def test_damaged_dictionaries_get_libzstds_verdict(ent):
    data = df.piece(BLOB, ent)
    h = C.c_void_p()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    rc = zk.lib.zk_dict_create(buf, len(data), C.byref(h))
    assert rc == -ent["using_dict"]                          # 0, or -30 dictionary_corrupted
    assert (rc != 0) == (ent["load_dictionary"] != 0)        # ZSTD_DCtx_loadDictionary refuses exactly those
    assert bool(h.value) == (rc == 0)
    if rc == 0:
        if ent["name"] == "wrong_magic":                     # not a formatted dictionary: raw content
            assert zk.lib.zk_dict_id(h) == 0 and zk.lib.zk_dict_content_offset(h) == 0
        zk.lib.zk_dict_free(h)
    else:
        assert zk.error_name(rc) == "Dictionary is corrupted"


def test_arguments_and_empty_input():
    h = C.c_void_p()
    assert zk.lib.zk_dict_create(None, 4, C.byref(h)) == -2003
    assert zk.lib.zk_dict_create(None, 0, None) == -2003
    assert zk.lib.zk_dict_create(None, 0, C.byref(h)) == 0   # empty raw content
    assert zk.lib.zk_dict_id(h) == 0
    zk.lib.zk_dict_free(h)
    zk.lib.zk_dict_free(None)
    assert zk.lib.zk_dict_id(None) == 0


def test_frames_state_the_facts_the_cases_exist_for():
    """The recorded facts, read again from the frames' bytes (tests/helpers/dict_fixtures.frame_facts)."""
    did = IDX["dicts"]["trained"]["id"]
    for case in IDX["cases"]:
        for fr in case["frames"]:
            facts = df.frame_facts(df.piece(BLOB, fr))
            assert facts["dict_id"] == fr["dict_id"] and facts["checksum"] == fr["checksum"]
            if "blocks" in fr:
                assert [[b[0], b[1], list(b[2]) if b[2] else None] for b in facts["blocks"]] == fr["blocks"]
    by = {c["name"]: c["frames"] for c in IDX["cases"]}
    assert all(fr["dict_id"] == did for fr in by["trained"])
    small = [fr for fr in by["trained"] if fr["level"] in (1, 3)]
    assert all(fr["blocks"][0][2] == [3, 3, 3] for fr in small) and sum(fr["blocks"][0][1] == 3 for fr in small) >= 20
    l19 = [fr["blocks"][0] for fr in by["trained"] if fr["level"] == 19]
    assert any(b[2] and 2 in b[2] and 3 in b[2] for b in l19) and any(b[1] == 0 for b in l19) and any(b[1] == 2 for b in l19)
    big = max(by["trained"], key=lambda fr: fr["d_size"])["blocks"]
    assert big[0][1:] == [3, [3, 3, 3]] and big[1][1] == 3 and big[2][1:] == [2, [2, 2, 2]] and len(big) >= 4
    assert all(fr["dict_id"] is None for fr in by["no_id"] + by["raw"])
    assert [fr["dict_id"] == did for fr in by["mixed"]] == [i % 2 == 0 for i in range(len(by["mixed"]))]
    assert all(fr["expect"] != fr["unpatched"] for fr in by["rep"])


def test_fixtures_still_decode_under_libzstd_1_5_7():
    z = libzstd_ref.load("1.5.7")
    if z is None:
        pytest.skip("libzstd 1.5.7 is not in this image")
    z.ZSTD_decompress_usingDict.restype = C.c_size_t
    z.ZSTD_decompress_usingDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    z.ZSTD_isError.restype = C.c_uint
    z.ZSTD_isError.argtypes = [C.c_size_t]
    dctx = z.ZSTD_createDCtx()

    def dec(frame, cap, d):
        out = C.create_string_buffer(max(cap, 1))
        n = z.ZSTD_decompress_usingDict(dctx, out, cap, frame, len(frame), d, len(d) if d else 0)
        return None if z.ZSTD_isError(n) else out.raw[:n]
    for case in IDX["cases"]:
        d = dict_bytes(case["dict"])
        for fr in case["frames"]:
            f = df.piece(BLOB, fr)
            want = bytes.fromhex(fr["expect"]) if "expect" in fr else df.plain(fr["recipe"])
            assert dec(f, fr["d_size"], d) == want, (case["name"], fr["offset"])
            assert "%016x" % zko.xxh64(want) == fr["xxh64"]
            if "needs_dict" in fr:
                assert (dec(f, fr["d_size"], None) != want) == fr["needs_dict"]
    z.ZSTD_freeDCtx(dctx)

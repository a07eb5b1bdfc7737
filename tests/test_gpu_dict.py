"""Frames compressed with a zstd dictionary, on the device: every case of tests/golden/dict_archives.* (libzstd 1.5.7 made them;
tools/make_dict_goldens.py, facts re-checked in tests/test_dict.py) decodes bit-exact with checksums verified through the decode routes
that honour Engine.set_dictionary, under the pinned kernel variants, and the statuses around a dictionary are what libzstd's are.
No input here provokes a fault: every damaged or mismatched one is refused by the frame walk with a status."""
import numpy as np
import pytest

import zeekstd_amd as zk
from zeekstd_amd import DecodeOptions, SeekTable
from conftest import PREFIX_GOLDENS
from helpers import dict_fixtures as df
from helpers.dev_decode import dev as _dev, upload as _upload
from test_gpu_exec_seg import VARIANTS as SEG_VARIANTS
from test_gpu_kernel_choice import VARIANTS as KERNEL_VARIANTS

pytestmark = pytest.mark.gpu

IDX, BLOB = df.load()
CASES = {c["name"]: c for c in IDX["cases"]}
VARIANTS = {**KERNEL_VARIANTS, **SEG_VARIANTS, "fse_own1_shared1": dict(fse_own=1, fse_shared=1), "fse_own2_shared3": dict(fse_own=2, fse_shared=3),
            "entropy1": dict(entropy=1), "entropy2": dict(entropy=2)}
POISON = 0x5A


def dict_bytes(name):
    ent = IDX["dicts"][name]
    if "of" in ent:
        return df.patch_reps(dict_bytes(ent["of"]), ent["header_size"], ent["reps"])
    return df.piece(BLOB, ent)


_PLAIN = {}


def expected(case):
    """(compressed bytes, c_off, d_off, decoded bytes) of a case, made once"""
    if case["name"] not in _PLAIN:
        comp, c, d = df.archive(BLOB, case)
        data = b"".join(bytes.fromhex(fr["expect"]) if "expect" in fr else df.plain(fr["recipe"]) for fr in case["frames"])
        assert len(data) == d[-1]
        _PLAIN[case["name"]] = (comp, np.asarray(c, np.uint64), np.asarray(d, np.uint64), data)
    return _PLAIN[case["name"]]


@pytest.fixture
def with_dict(engine):
    """load(name) sets the case's dictionary on the session's engine; none is left behind"""
    engine.set_kernel_choice(reset=0)

    def load(name):
        engine.set_dictionary(zk.Dictionary(dict_bytes(name)) if name else None)
        return engine
    yield load
    engine.set_dictionary(None)
    engine.set_kernel_choice(reset=0)


def dev_decode(engine, case, first=0, count=None, verify=True):
    import torch
    comp, c, d, data = expected(case)
    count = len(c) - 1 - first if count is None else count
    arch = _upload(comp, c, d)
    total = int(d[first + count] - d[first])
    out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=_dev())
    st = torch.full((count,), -1, dtype=torch.int32, device=_dev())
    rc = engine.decode_frames_dev(arch[0], arch[1], arch[2], arch[3], first, count, out, total, verify, st)
    torch.cuda.synchronize()
    return rc, out[:total].cpu().numpy().tobytes(), st.cpu().numpy(), data[int(d[first]):int(d[first + count])]


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_decodes_from_hbm(with_dict, name):
    case = CASES[name]
    rc, out, st, want = dev_decode(with_dict(case["dict"]), case)
    assert rc == 0 and not st.any(), (rc, np.flatnonzero(st)[:5], st[st != 0][:5])
    assert out == want


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_decodes_from_host_memory(with_dict, name):
    """zk_decode_frames: up to 64 frames (the host shortcut hands a dictionary batch to the general pipeline), and 65 and more"""
    case = CASES[name]
    e = with_dict(case["dict"])
    comp, c, d, data = expected(case)
    n = len(c) - 1
    for first, count in ((0, n), (0, min(n, 3)), (n - 1, 1)):
        out, st = e.decode_frames(comp + b"\0" * 8, c, d, first, count, verify=True)
        assert not st.any(), (first, count, st)
        assert out == data[int(d[first]):int(d[first + count])]
    # the same frames three times over: more than 64
    comp3 = comp * 3
    c3 = np.concatenate([c[:-1], c[:-1] + c[-1], c + 2 * c[-1]])
    d3 = np.concatenate([d[:-1], d[:-1] + d[-1], d + 2 * d[-1]])
    if len(c3) - 1 > 64:
        out, st = e.decode_frames(comp3 + b"\0" * 8, c3, d3, verify=True)
        assert not st.any() and out == data * 3


@pytest.mark.parametrize("name", ["trained", "mixed", "rep"])
def test_frame_list_shuffled_with_repeats(with_dict, name):
    import torch
    case = CASES[name]
    e = with_dict(case["dict"])
    comp, c, d, data = expected(case)
    n = len(c) - 1
    rng = np.random.RandomState(5)
    ids = np.concatenate([rng.permutation(n), rng.randint(0, n, 17)]).astype(np.uint32)
    sizes = (d[1:] - d[:-1])[ids]
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    arch = _upload(comp, c, d)
    total = int(out_off[-1])
    out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=_dev())
    st = torch.full((len(ids),), -1, dtype=torch.int32, device=_dev())
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(_dev())
    d_oo = torch.from_numpy(out_off.view(np.int64).copy()).to(_dev())
    rc = e.decode_frame_list_dev(arch[0], arch[1], arch[2], arch[3], d_ids, d_oo, len(ids), out, total, True, st)
    torch.cuda.synchronize()
    assert rc == 0 and not st.cpu().numpy().any()
    assert out[:total].cpu().numpy().tobytes() == b"".join(data[int(d[i]):int(d[i + 1])] for i in ids)


def test_two_submitted_batches_and_no_new_dictionary_meanwhile(with_dict):
    import torch
    case = CASES["trained"]
    e = with_dict("trained")
    comp, c, d, data = expected(case)
    arch = _upload(comp, c, d)
    half = (len(c) - 1) // 2
    spans = [(0, half), (half, len(c) - 1 - half)]
    outs, sts, slots = [], [], []
    for first, count in spans:
        total = int(d[first + count] - d[first])
        outs.append(torch.full((total + 64,), POISON, dtype=torch.uint8, device=_dev()))
        sts.append(torch.full((count,), -1, dtype=torch.int32, device=_dev()))
        slots.append(e.decode_submit_dev(arch[0], arch[1], arch[2], arch[3], first, count, outs[-1], total, True, sts[-1]))
    other = zk.Dictionary(dict_bytes("raw"))
    assert zk.lib.zk_engine_set_dictionary(e._h, other._h) == -2003          # ZK_ERR_ARGUMENT: batches are outstanding
    assert zk.lib.zk_engine_set_dictionary(e._h, None) == -2003
    for (first, count), out, st, slot in zip(spans, outs, sts, slots):
        assert e.decode_wait(slot) == 0
        assert not st.cpu().numpy().any()
        assert out[:int(d[first + count] - d[first])].cpu().numpy().tobytes() == data[int(d[first]):int(d[first + count])]


def _ranges(d):
    """byte ranges of a case's decoded stream: inside the first frame, across the first boundary, two bytes around a boundary in the middle,
    several whole frames and a bit, the stream's tail, and an empty one"""
    n, total = len(d) - 1, int(d[-1])
    mid = n // 2
    at = [int(x) for x in d]
    r = [(0, min(50, total)), (at[1] - 7, min(300, total - at[1] + 7)), (at[mid] - 1, 2), (at[mid] + 3, at[min(n, mid + 4)] - at[mid] - 3),
         (total - 20, 20), (at[n - 1], 0)]
    return np.array([o for o, _ in r], np.uint64), np.array([k for _, k in r], np.uint64)


@pytest.mark.parametrize("name", list(CASES))
def test_read_ranges_that_straddle_frames(with_dict, name):
    """zk_read_ranges_dev on device buffers (packed destinations), then the host wrapper zk_read_ranges on the same ranges"""
    import torch
    case = CASES[name]
    e = with_dict(case["dict"])
    comp, c, d, data = expected(case)
    offs, lens = _ranges(d)
    want = b"".join(data[int(o):int(o + k)] for o, k in zip(offs, lens))
    arch = _upload(comp, c, d)
    dst = torch.full((len(want) + 64,), POISON, dtype=torch.uint8, device=_dev())
    st = torch.full((len(offs),), -1, dtype=torch.int32, device=_dev())
    d_o = torch.from_numpy(offs.view(np.int64).copy()).to(_dev())
    d_l = torch.from_numpy(lens.view(np.int64).copy()).to(_dev())
    rc = e.read_ranges_dev(arch[0], arch[1], arch[2], arch[3], len(c) - 1, d_o, d_l, None, len(offs), dst, len(want), True, st)
    torch.cuda.synchronize()
    assert rc == 0 and not st.cpu().numpy().any(), (rc, st.cpu().numpy())
    got = dst.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all()
    got, st = e.read_ranges(comp, c, d, offs, lens, verify=True)
    assert not np.asarray(st).any()
    assert b"".join(bytes(g) for g in got) == want


@pytest.mark.parametrize("name", list(CASES))
def test_frame_content_sizes(with_dict, name):
    """zk_frame_content_sizes_dev on device buffers, then the host wrapper"""
    import torch
    case = CASES[name]
    e = with_dict(case["dict"])
    comp, c, d, _ = expected(case)
    n = len(c) - 1
    arch = _upload(comp, c, d)
    d_sizes = torch.full((n,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    rc = zk.lib.zk_frame_content_sizes_dev(e._h, arch[0].data_ptr(), arch[1], arch[2].data_ptr(), 0, n, d_sizes.data_ptr(), d_st.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and not d_st.cpu().numpy().any(), (rc, d_st.cpu().numpy())
    assert np.array_equal(d_sizes.cpu().numpy().view(np.uint64), d[1:] - d[:-1])
    sizes, st = e.frame_content_sizes(comp, c)
    assert not st.any() and np.array_equal(sizes, d[1:] - d[:-1])


def _seekable(comp, c, d):
    st = SeekTable.new()
    for i in range(len(c) - 1):
        st.log_frame(int(c[i + 1] - c[i]), int(d[i + 1] - d[i]))
    return comp + st.to_bytes()


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_through_a_decoder_handle(with_dict, name):
    """zk_decoder_* opened on the engine: the whole archive read to its end, then reads after seeks (inside one frame, across frames)"""
    case = CASES[name]
    e = with_dict(case["dict"])
    comp, c, d, data = expected(case)
    dec = DecodeOptions(_seekable(comp, c, d)).engine(e).into_decoder()
    try:
        assert dec.read_to_end() == data
        offs, lens = _ranges(d)
        for a, k in zip(offs, lens):
            a, b = int(a), int(a + k)
            dec.set_offset_limit(len(data)); dec.set_offset(a); dec.set_offset_limit(b)
            buf, got = bytearray(b - a), 0
            while got < b - a:
                m = dec.decompress(memoryview(buf)[got:])
                assert m > 0
                got += m
            assert bytes(buf) == data[a:b]
            assert dec.decompress(bytearray(8)) == 0
    finally:
        dec.close()


def test_a_decoder_handle_refuses_what_the_engine_refuses(with_dict):
    """no dictionary on the engine: the handle fails with the frame's status"""
    e = with_dict(None)
    comp, c, d, data = expected(CASES["trained"])
    dec = DecodeOptions(_seekable(comp, c, d)).engine(e).into_decoder()
    try:
        with pytest.raises(zk.Error) as err:
            dec.decompress(bytearray(len(data)))
        assert err.value.code == -32
    finally:
        dec.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trained_and_mixed_under_every_pinned_variant(with_dict, variant):
    """both batches whole from HBM (where the sequence kernels, the executor's tile and the checksum kernels are what the variant pins) and
    through the host pipeline; the fused entropy kernel has to carry the dictionary itself"""
    e = with_dict("trained")
    for name in ("trained", "mixed"):
        case = CASES[name]
        e.set_kernel_choice(reset=0)
        e.set_kernel_choice(**VARIANTS[variant])
        rc, out, st, want = dev_decode(e, case)
        assert rc == 0 and not st.any(), (name, rc, np.flatnonzero(st)[:5])
        assert out == want, name
        if VARIANTS[variant].get("entropy") == 2:
            # (every frame but the multi-block one defines at most one set of tables; that one is left out: the batch qualifies)
            count = len(case["frames"]) - (1 if name == "trained" else 0)
            rc, out, st, want = dev_decode(e, case, 0, count)
            assert rc == 0 and not st.any() and out == want
            assert e.entropy_fused(), name
        comp, c, d, data = expected(case)
        got, st = e.decode_frames(comp + b"\0" * 8, c, d, verify=True)
        assert not st.any() and got == data, name


# ------------------------------------------------------------------------------------------------ statuses
def test_wrong_id_is_refused_for_those_frames_only(with_dict):
    """a copy of the trained dictionary under another ID: its frames are -32, the plain ones between them are delivered"""
    case = CASES["mixed"]
    d0 = dict_bytes("trained")
    other = d0[:4] + (IDX["dicts"]["trained"]["id"] ^ 0x55).to_bytes(4, "little") + d0[8:]
    e = with_dict(None)
    e.set_dictionary(zk.Dictionary(other))
    rc, out, st, want = dev_decode(e, case)
    comp, c, d, _ = expected(case)
    assert rc == -32 and list(st) == [32 if i % 2 == 0 else 0 for i in range(len(st))]
    for i in range(1, len(st), 2):
        assert out[int(d[i]):int(d[i + 1])] == want[int(d[i]):int(d[i + 1])]


def test_without_a_dictionary_nothing_changed(with_dict):
    e = with_dict(None)
    for name, want in (("trained", 32), ("no_id", 20), ("raw", None)):
        rc, out, st, _ = dev_decode(e, CASES[name])
        if want is not None:
            assert rc == -want and (st == want).all(), (name, rc, st)
        else:
            # offsets below the frame's first byte are corruption: exactly the frames the generator found to need the dictionary fail
            case = CASES[name]
            comp, c, d, data = expected(case)
            need = np.array([fr["needs_dict"] for fr in case["frames"]])
            assert need.any() and rc != 0 and np.array_equal(st != 0, need), (name, rc, st)
            for i in np.flatnonzero(~need):
                assert out[int(d[i]):int(d[i + 1])] == data[int(d[i]):int(d[i + 1])]
    # ... and again after a dictionary was set and taken away
    with_dict("trained")
    rc, out, st, want = dev_decode(e, CASES["trained"])
    assert rc == 0 and out == want
    with_dict(None)
    rc, out, st, _ = dev_decode(e, CASES["trained"])
    assert rc == -32 and (st == 32).all()
    # plain frames decode the same with and without
    case = CASES["mixed"]
    rc, out, st, want = dev_decode(e, case)
    comp, c, d, _ = expected(case)
    assert list(st) == [32 if i % 2 == 0 else 0 for i in range(len(st))]
    for i in range(1, len(st), 2):
        assert out[int(d[i]):int(d[i + 1])] == want[int(d[i]):int(d[i + 1])]


def test_raw_content_dictionary_lends_no_tables(with_dict):
    """Treeless literals / Repeat_Mode in a first block stay corruption under a raw-content dictionary (no_id: frames without an ID field
    whose first blocks repeat the trained dictionary's tables)"""
    rc, out, st, _ = dev_decode(with_dict("raw"), CASES["no_id"])
    assert rc == -20 and (st == 20).all()
    # ... and frames that name an ID are refused by it
    rc, out, st, _ = dev_decode(with_dict("raw"), CASES["trained"])
    assert rc == -32 and (st == 32).all()


def test_repeat_offsets_come_from_the_dictionary(with_dict):
    """the hand-made frames under the UNPATCHED dictionary: what libzstd recorded for it, which differs"""
    case = CASES["rep"]
    e = with_dict("trained")
    comp, c, d, _ = expected(case)
    for i, fr in enumerate(case["frames"]):
        out, st = e.decode_frames(comp + b"\0" * 8, c, d, i, 1, verify=True, raise_on_error=False)
        if isinstance(fr["unpatched"], str):
            assert st[0] == 0 and out == bytes.fromhex(fr["unpatched"]) and out != bytes.fromhex(fr["expect"])
        else:
            assert st[0] == fr["unpatched"]


def test_an_explicit_prefix_overrides_the_dictionary(with_dict):
    e = with_dict("trained")
    g = PREFIX_GOLDENS[0]
    c, d = g.offsets()
    out, st = e.decode_frames(g.comp + b"\0" * 8, c, d, verify=True, prefix=g.prefix())
    assert not st.any() and out == g.input()
    # ... and through a handle: zk_decoder_decompress_with_prefix
    dec = DecodeOptions(_seekable(g.comp, c, d)).engine(e).into_decoder()
    try:
        pre, want = g.prefix(), g.input()
        buf, got = bytearray(len(want)), 0
        while got < len(want):
            m = dec.decompress_with_prefix(memoryview(buf)[got:], pre)
            assert m > 0
            got += m
        assert bytes(buf) == want
    finally:
        dec.close()

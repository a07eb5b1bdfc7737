"""tests/test_generated_dict.py on the device: dictionaries nobody trained (tests/helpers/zstd_gen.py: make_dictionary -- content of 1, 7, 8,
9 bytes and of more than 128 KiB, direct and FSE-compressed weights, the tables' accuracy logs at both ends, IDs for every width of the
Dictionary_ID field and 0) and frames no encoder writes against them: every table independently the dictionary's, predefined, RLE or the
block's own, Treeless literals in a first block, the dictionary's repeat offsets through all four indices, matches from the dictionary's
first byte and across the frame's first byte.  The expectation is the generator's model, which libzstd 1.5.7, the oracle and the lane code
confirm on the CPU for these very seeds (tests/test_generated_dict.py: test_the_gpu_tests_frames_mean_what_libzstd_says), and the facts
about the batches that these tests take for granted are asserted there (test_premises_of_the_gpu_batches).  Every decode goes into a
poisoned buffer, with checksums verified and every status 0 unless a test says otherwise."""
import numpy as np
import pytest

import zeekstd_amd as zk
from zeekstd_amd import DecodeOptions
from helpers import gen_batches as G
from helpers.dev_decode import dev as _dev, upload as _upload
from test_gpu_dict import POISON, VARIANTS, _ranges, _seekable

pytestmark = pytest.mark.gpu

_ARCH = {}


def arch(key, batch=None):
    """(compressed bytes, c_off, d_off, decoded bytes) of a batch, laid out once: key is a dictionary's name (its default frames) or a
    batch's own, "batch:..." (no dictionary's name: DICTS has a "big" too)"""
    assert (batch is None) == (key in G.DICTS)
    if key not in _ARCH:
        comp, sizes, data = G.archive(G.dict_frames(key) if batch is None else batch)
        c = np.concatenate([[0], np.cumsum([s[0] for s in sizes])]).astype(np.uint64)
        d = np.concatenate([[0], np.cumsum([s[1] for s in sizes])]).astype(np.uint64)
        _ARCH[key] = (comp, c, d, data)
    return _ARCH[key]


@pytest.fixture
def with_dict(engine):
    """load(name) sets a dictionary of G.DICTS on the session's engine; none is left behind, and no kernel choice"""
    engine.set_kernel_choice(reset=0)

    def load(name):
        engine.set_dictionary(zk.Dictionary(G.dictionary(name)[0]) if name else None)
        return engine
    yield load
    engine.set_dictionary(None)
    engine.set_kernel_choice(reset=0)


def dev_decode(engine, a, first=0, count=None, verify=True):
    """-> (rc, bytes, statuses, expected bytes) of frames [first, first + count) from HBM to a poisoned buffer in HBM"""
    import torch
    comp, c, d, data = a
    count = len(c) - 1 - first if count is None else count
    up = _upload(comp, c, d)
    total = int(d[first + count] - d[first])
    out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=_dev())
    st = torch.full((count,), -1, dtype=torch.int32, device=_dev())
    rc = engine.decode_frames_dev(up[0], up[1], up[2], up[3], first, count, out, total, verify, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == POISON).all()
    return rc, got[:total].tobytes(), st.cpu().numpy(), data[int(d[first]):int(d[first + count])]


def clean(rc, out, st, want):
    assert rc == 0 and not st.any(), (rc, np.flatnonzero(st)[:5], st[st != 0][:5])
    assert out == want


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("name", G.ROUTE_DICTS)
def test_frames_decode_from_hbm(with_dict, name):
    clean(*dev_decode(with_dict(name), arch(name)))


@pytest.mark.parametrize("name", G.ROUTE_DICTS)
def test_frames_decode_from_host_memory(with_dict, name):
    """zk_decode_frames whole (more than 64 frames: the pipeline), and in sub-ranges of at most 64 frames (what the host shortcut would
    take without a dictionary)"""
    e = with_dict(name)
    comp, c, d, data = arch(name)
    n = len(c) - 1
    out, st = e.decode_frames(comp + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    assert not st.any() and out == data
    rng = np.random.default_rng(7)
    for first, count in [(0, 1), (0, 64), (n - 1, 1), (n - 17, 17)] + [(int(rng.integers(0, n - 64)), int(rng.integers(1, 65))) for _ in range(6)]:
        out, st = e.decode_frames(comp + b"\0" * 8, c, d, first, count, verify=True, raise_on_error=False)
        assert not st.any() and out == data[int(d[first]):int(d[first + count])], (first, count)


@pytest.mark.parametrize("name", G.ROUTE_DICTS)
def test_frame_list_shuffled_with_repeats(with_dict, name):
    import torch
    e = with_dict(name)
    comp, c, d, data = arch(name)
    n = len(c) - 1
    rng = np.random.RandomState(5)
    ids = np.concatenate([rng.permutation(n), rng.randint(0, n, 17)]).astype(np.uint32)
    out_off = np.concatenate([[0], np.cumsum((d[1:] - d[:-1])[ids])]).astype(np.uint64)
    up = _upload(comp, c, d)
    total = int(out_off[-1])
    out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=_dev())
    st = torch.full((len(ids),), -1, dtype=torch.int32, device=_dev())
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(_dev())
    d_oo = torch.from_numpy(out_off.view(np.int64).copy()).to(_dev())
    rc = e.decode_frame_list_dev(up[0], up[1], up[2], up[3], d_ids, d_oo, len(ids), out, total, True, st)
    torch.cuda.synchronize()
    assert rc == 0 and not st.cpu().numpy().any()
    assert out[:total].cpu().numpy().tobytes() == b"".join(data[int(d[i]):int(d[i + 1])] for i in ids)


@pytest.mark.parametrize("name", G.ROUTE_DICTS)
def test_read_ranges_that_straddle_frames(with_dict, name):
    """zk_read_ranges_dev with the ranges of tests/test_gpu_dict.py: inside the first frame, across boundaries, the tail, an empty one"""
    import torch
    e = with_dict(name)
    comp, c, d, data = arch(name)
    offs, lens = _ranges(d)
    want = b"".join(data[int(o):int(o + k)] for o, k in zip(offs, lens))
    up = _upload(comp, c, d)
    dst = torch.full((len(want) + 64,), POISON, dtype=torch.uint8, device=_dev())
    st = torch.full((len(offs),), -1, dtype=torch.int32, device=_dev())
    d_o = torch.from_numpy(offs.view(np.int64).copy()).to(_dev())
    d_l = torch.from_numpy(lens.view(np.int64).copy()).to(_dev())
    rc = e.read_ranges_dev(up[0], up[1], up[2], up[3], len(c) - 1, d_o, d_l, None, len(offs), dst, len(want), True, st)
    torch.cuda.synchronize()
    assert rc == 0 and not st.cpu().numpy().any(), (rc, st.cpu().numpy())
    got = dst.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all()


@pytest.mark.parametrize("name", G.ROUTE_DICTS)
def test_frames_through_a_decoder_handle(with_dict, name):
    """zk_decoder_* opened on the engine: read to the end, then reads after seeks"""
    e = with_dict(name)
    comp, c, d, data = arch(name)
    dec = DecodeOptions(_seekable(comp, c, d)).engine(e).into_decoder()
    try:
        assert dec.read_to_end() == data
        for a, k in zip(*_ranges(d)):
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


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mixed_batch_under_every_pinned_variant(with_dict, variant):
    """default and shared_tables frames against one dictionary, from HBM (where the variant's kernels run) and through the host pipeline"""
    e = with_dict(G.BIG_DICT)
    a = arch("batch:mixed", G.dict_batch_mixed())
    e.set_kernel_choice(**VARIANTS[variant])
    clean(*dev_decode(e, a))
    comp, c, d, data = a
    out, st = e.decode_frames(comp + b"\0" * 8, c, d, verify=True, raise_on_error=False)
    assert not st.any() and out == data


def test_shared_table_kernels_by_the_engines_own_choice(with_dict):
    """no kernel pinned: more than 4096 blocks (zk_launch_fse takes the shared-table kernels: runs of 64 blocks whose reference keys are
    the dictionary's entry, that entry beside predefined tables, or a block's own), then 4096 or fewer drawn from the same frames (every
    block builds its own copy) -- the same bytes either side of the threshold"""
    e = with_dict(G.BIG_DICT)
    big, small = G.dict_batch_big(), G.dict_batch_small()
    rc, out, st, want = dev_decode(e, arch("batch:big", big))
    clean(rc, out, st, want)
    rc, out2, st, want2 = dev_decode(e, arch("batch:small", small))
    clean(rc, out2, st, want2)
    at, pos = {}, 0
    for f in big:
        at[(f.kind, f.seed)] = out[pos:pos + len(f.data)]; pos += len(f.data)
    pos = 0
    for f in small:
        assert out2[pos:pos + len(f.data)] == at[(f.kind, f.seed)]; pos += len(f.data)


def test_fused_entropy_kernel_carries_the_dictionary(with_dict):
    """blocks that describe a table <= frames: under entropy=2 the fused kernel runs, and follows the dictionary's entry itself"""
    e = with_dict(G.BIG_DICT)
    e.set_kernel_choice(entropy=2)
    clean(*dev_decode(e, arch("batch:fused", G.dict_batch_fused())))
    assert e.entropy_fused()


def test_frame_content_sizes_without_frame_content_size(with_dict):
    """zk_frame_content_sizes_dev and the host wrapper on frames that do not state their size: it is learnt from sequences decoded with
    the dictionary's tables"""
    import torch
    e = with_dict(G.BIG_DICT)
    comp, c, d, _ = arch("batch:sizes", G.dict_batch_sizes())
    n = len(c) - 1
    up = _upload(comp, c, d)
    d_sizes = torch.full((n,), -1, dtype=torch.int64, device=_dev())
    d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    rc = zk.lib.zk_frame_content_sizes_dev(e._h, up[0].data_ptr(), up[1], up[2].data_ptr(), 0, n, d_sizes.data_ptr(), d_st.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and not d_st.cpu().numpy().any(), (rc, d_st.cpu().numpy())
    assert np.array_equal(d_sizes.cpu().numpy().view(np.uint64), d[1:] - d[:-1])
    sizes, st = e.frame_content_sizes(comp, c)
    assert not st.any() and np.array_equal(sizes, d[1:] - d[:-1])


# ------------------------------------------------------------------------------------------------ more than one dictionary in an engine's life
def test_a_then_b_then_a(with_dict):
    for name in ("few_kib", "nine", "few_kib", "big", "one_byte", "big"):
        clean(*dev_decode(with_dict(name), arch(name), 0, 60))


def test_two_dictionaries_with_one_id(with_dict):
    """the same Dictionary_ID, other tables, other content: each decodes its own frames, one after the other and back"""
    assert G.dictionary("same_id_a")[1].id == G.dictionary("same_id_b")[1].id
    for name in ("same_id_a", "same_id_b", "same_id_a"):
        clean(*dev_decode(with_dict(name), arch(name)))


def test_a_formatted_dictionary_with_id_0(with_dict):
    """frames whose Dictionary_ID field is absent or holds 0 in one, two or four bytes"""
    feats = set().union(*(f.feats for f in G.dict_frames("id0")))
    assert {"did_absent", "did_width1", "did_width2", "did_width4"} <= feats and G.dictionary("id0")[1].id == 0
    clean(*dev_decode(with_dict("id0"), arch("id0")))


def test_frames_that_name_another_dictionary_are_refused_and_only_those(with_dict):
    """frames of A that name A's ID between frames of B, under B: 32 for exactly A's, B's are delivered"""
    a = [f for f in G.dict_frames("few_kib") if "did_absent" not in f.feats][:40]
    b = G.dict_frames("nine")[:40]
    assert len(a) == 40 and G.dictionary("few_kib")[1].id != G.dictionary("nine")[1].id
    batch = [f for pair in zip(a, b) for f in pair]
    rc, out, st, want = dev_decode(with_dict("nine"), arch("batch:a_under_b", batch))
    assert rc == -32 and list(st) == [32, 0] * 40
    pos = 0
    for f in batch:
        if f.dict == "nine":
            assert out[pos:pos + len(f.data)] == f.data
        pos += len(f.data)


# ------------------------------------------------------------------------------------------------ damaged frames
@pytest.mark.parametrize("name", G.DAMAGED_DICTS)
def test_damaged_frames_against_the_oracle(with_dict, name):
    """one to three flipped bits in every other frame, checksums not verified: the kernels refuse exactly the frames the oracle (with the
    dictionary) refuses, and yield its bytes otherwise.  These very bytes went through the lane code on the CPU and through the
    AddressSanitizer + UBSan program tests/sim/dict_fuzz.cpp first, and left no buffer there
    (tests/test_generated_dict.py: test_damaged_generated_frames_the_lane_code_against_the_oracle,
    test_lane_code_with_a_dictionary_under_sanitizers): nothing here is meant to provoke a fault."""
    bad, sizes, hit, data = G.dict_damaged(name)
    c = np.concatenate([[0], np.cumsum([s[0] for s in sizes])]).astype(np.uint64)
    d = np.concatenate([[0], np.cumsum([s[1] for s in sizes])]).astype(np.uint64)
    rc, out, st, _ = dev_decode(with_dict(name), (bad, c, d, data), verify=False)
    G.dict_damaged_judge(name, out, st)

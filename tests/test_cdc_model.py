"""The rule zk_chunk_boundaries cuts by (include/zeekstd_amd.h), as the numpy model of tests/helpers/cdc_model.py states it: what the rule
promises -- a partition into frames of [min, max] bytes, the uniform grid for min == max, cuts that fall back onto the old ones after an
edit -- is asserted on the model, which is what the emulator (tests/test_sim_cdc.py) and the device (tests/test_gpu_cdc.py) are held to bit
for bit.  The parameter table is checked against the library where no device is needed: zk_compress_bound_chunked resolves the defaults
and gives 0 for what is refused.  What zk_chunk_boundaries[_dev] and zk_encode_chunked_dev make of the same table needs an engine:
tests/test_gpu_cdc.py."""
import ctypes as C

import numpy as np
import pytest

from helpers import cdc_model as M

CASES = M.cases()


def test_gear_table_and_dense_bytes():
    g = M.gear()
    assert len(set(g.tolist())) == 256
    x = (1 * 0x9E3779B1) & 0xFFFFFFFF                               # G[0] by hand
    x ^= x >> 16; x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(g[0]) == x
    dense = M.dense_bytes()
    assert len(dense) == 3
    for b in dense:
        c = M.candidates(np.full(1000, b, np.uint8), 8)
        assert c[31:].all()                                         # every position whose window is full
    # a position's hash depends on the 32 bytes that end there, and on nothing else
    a, b = M.rand(1, 500), M.rand(2, 500)
    b[200:232] = a[100:132]
    assert M.hashes(a)[131] == M.hashes(b)[231] and M.hashes(a)[132] != M.hashes(b)[232]


@pytest.mark.parametrize("name", list(CASES))
def test_cuts_partition_the_input(name):
    c = CASES[name]
    off = c.cuts().astype(np.int64)
    n = len(c.data)
    assert off[0] == 0 and off[-1] == n
    sizes = np.diff(off)
    if n == 0:
        assert off.tolist() == [0, 0]
        return
    assert (sizes[:-1] >= c.mn).all() and (sizes <= c.mx).all() and (sizes > 0).all()
    if name.startswith("short_last"):
        assert sizes[-1] == c.mn // 2 and len(sizes) > 1
    if name.startswith("on_lo"):
        assert sizes[0] == c.mn and M.candidates(c.data, c.bits)[c.mn - 1]
    if name.startswith("on_hi"):
        assert sizes[0] == c.mx and M.candidates(c.data, c.bits)[c.mx - 1] and not M.candidates(c.data, c.bits)[c.mn - 1:c.mx - 1].any()
    if name.startswith("zeros"):
        assert not M.candidates(c.data, c.bits).any() and (sizes[:-1] == c.mx).all()         # forced cuts only
    if name.startswith("dense_mid") and "long" not in name:
        assert M.candidates(c.data, 8)[30031:35000].all()


@pytest.mark.parametrize("size", [256, 1024, 4096])
def test_equal_sizes_are_the_uniform_grid(size):
    for n in (1, size - 1, size, size + 1, 10 * size + 77):
        got = M.cuts(M.rand(n, n), size, size.bit_length() - 1, size)
        want = list(range(0, n, size)) + [n]
        assert got.tolist() == want, n


def test_mean_frame_size_on_random_bytes():
    """about min + avg when max is far away: 316, 1306 and 5243 bytes were measured"""
    data = M.rand(5, 1 << 20)
    for (mn, avg, _), seen in zip(M.SETTINGS, (316, 1306, 5243)):
        sizes = np.diff(M.cuts(data, mn, avg.bit_length() - 1, 64 * avg).astype(np.int64))
        assert abs(sizes.mean() - (mn + avg)) < 0.15 * (mn + avg), (avg, sizes.mean(), seen)


@pytest.mark.parametrize("setting", M.SETTINGS)
def test_cuts_fall_back_after_an_insertion(setting):
    """at most 8 frames of the edited input fail to be frames of the original (measured worst cases: 7, 2 and 2)"""
    mn, avg, mx = setting
    bits = avg.bit_length() - 1
    data = M.rand(11, 1 << 20)
    n = len(data)
    off = M.cuts(data, mn, bits, mx)
    old = {data[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])}
    rng = np.random.default_rng(12)
    worst = 0
    for k in (1, 3, 33, 1000):
        ins = rng.integers(0, 256, k, dtype=np.uint8)
        for at in (0, 1, 5000, 300000, 1 << 19, n - 40, n):
            edited = np.concatenate([data[:at], ins, data[at:]])
            o2 = M.cuts(edited, mn, bits, mx)
            new = sum(edited[int(a):int(b)].tobytes() not in old for a, b in zip(o2[:-1], o2[1:]))
            worst = max(worst, new)
            assert new <= 8, (k, at, new)
    print("worst case for", setting, ":", worst)


def _params(mn, avg, mx, flags=0):
    import zeekstd_amd as zk
    return zk._lib.ChunkParams(mn, avg, mx, flags)


@pytest.mark.parametrize("row", M.PARAM_TABLE)
def test_parameter_table(row):
    import zeekstd_amd as zk
    mn, avg, mx, flags = row
    want = M.resolve(mn, avg, mx, flags)
    p = _params(mn, avg, mx, flags)
    for n in (0, 1, 12345, 10 << 20):
        for with_dict in (0, 1):
            got = int(zk.lib.zk_compress_bound_chunked(n, C.byref(p), with_dict))
            assert got == (int(zk.lib.zk_compress_bound_list(n, n // want[0] + 1, with_dict)) if want else 0), (row, n)


def test_null_parameters_are_the_defaults():
    import zeekstd_amd as zk
    assert M.resolve() == (1 << 19, 21, 1 << 23)
    for n in (0, 1 << 19, (1 << 30) + 5):
        assert int(zk.lib.zk_compress_bound_chunked(n, None, 0)) == int(zk.lib.zk_compress_bound_list(n, n // (1 << 19) + 1, 0))
    assert M.resolve(0, 1 << 24, 0) == (1 << 22, 24, 1 << 26) and M.resolve(0, 256, 0) == (64, 8, 1024)

"""The rule of zk_compact_archive_dev as tests/helpers/compact_model.py states it in numpy, against a plain Python loop on the cases the
emulator and the GPU tests share; remap is a bijection from the kept frames onto 0 .. n_kept - 1, the offsets are prefix sums.  No GPU."""
import numpy as np
import pytest

from helpers import compact_model as K

CASES = K.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_model_equals_the_loop(name):
    c = CASES[name]
    m, w = c.model(), K.model_loop(c.comp, c.c_off, c.d_off, c.live)
    assert m["n_kept"] == w["n_kept"] and m["written"] == w["written"]
    for key in ("remap", "c_off_out", "d_off_out", "dst"):
        assert m[key].dtype == w[key].dtype and len(m[key]) == len(w[key]) and K.first_diff(m[key], w[key]) is None, (name, key)


@pytest.mark.parametrize("name", list(CASES))
def test_remap_is_a_bijection_and_offsets_are_prefix_sums(name):
    c = CASES[name]
    m = c.model()
    kept = np.nonzero(c.live)[0]
    assert m["n_kept"] == len(kept)
    assert (m["remap"][kept] == np.arange(len(kept))).all()                          # onto 0 .. n_kept - 1, in order
    assert (m["remap"][c.live == 0] == K.REMOVED).all()
    assert m["c_off_out"][0] == c.c_off[0] and m["d_off_out"][0] == c.d_off[0]
    assert (np.diff(m["c_off_out"]) == np.diff(c.c_off)[kept]).all()
    assert (np.diff(m["d_off_out"]) == np.diff(c.d_off)[kept]).all()
    assert m["written"] == int(m["c_off_out"][-1]) == int(c.c_off[0]) + len(m["dst"])
    # every destination byte is the payload of its frame at its position
    for k in (0, len(kept) // 2, len(kept) - 1) if len(kept) else ():
        s = int(kept[k])
        a, b = int(m["c_off_out"][k] - c.c_off[0]), int(m["c_off_out"][k + 1] - c.c_off[0])
        assert (m["dst"][a:b] == K.payload(s, b - a)).all(), (name, s)


def test_the_cases_are_the_ones_the_kernel_needs():
    e = CASES["sizes_edges"]
    sizes = np.diff(e.c_off).astype(np.int64)
    for want in K.EDGE_SIZES:
        assert sorted(e.live[sizes == want].tolist()) == [0, 1], want                # once kept, once removed
    assert 600 << 10 < e.comp_size < 800 << 10 and max(K.EDGE_SIZES) > 3 * K.TILE
    assert CASES["sizes_edges_base"].c_off[0] != 0
    assert all(CASES[p].n == 400 for p in K.PATTERNS[:-1])
    assert CASES["empty_only"].model()["n_kept"] > 10 and len(CASES["empty_only"].model()["dst"]) == 0
    r10, r90 = CASES["random_10"].live, CASES["random_90"].live
    assert 0.05 < 1 - r10.mean() < 0.15 and 0.85 < 1 - r90.mean() < 0.95
    c = CASES["empty_runs"]
    runs = [(c.live[s], int(c.c_off[s + 1] - c.c_off[s])) for s in range(c.n)]
    assert (1, 0) in runs and any(l and z for l, z in runs)

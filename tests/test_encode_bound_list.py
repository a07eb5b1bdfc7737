"""zk_compress_bound_list(n, count, with_dictionary) = n + 3 * (n / 1024) + (53 + (dict ? 4 : 0)) * count is an upper bound of the sum of
the frames' own bounds -- zk_compress_bound(s, max(s, 1)), + 4 per frame with a dictionary -- since a frame's bound is
s + 3 * ceil(max(s, 1) / 1024) + 50 and the ceilings sum to at most n / 1024 + count.  Checked on random lists and on the edge list, where
the twin's frames also stay below it."""
import random

import zeekstd_amd as zk
from helpers import enc_list_inputs as E
from oracle import zko


def frame_bound(s, with_dict):
    return int(zk.lib.zk_compress_bound(s, max(s, 1))) + (4 if with_dict else 0)


def check(sizes):
    n = sum(sizes)
    for with_dict in (0, 1):
        b = int(zk.lib.zk_compress_bound_list(n, len(sizes), with_dict))
        assert b == n + 3 * (n // 1024) + (53 + 4 * with_dict) * len(sizes)
        assert b >= sum(frame_bound(s, with_dict) for s in sizes), (with_dict, sizes[:8], len(sizes))
    assert frame_bound(0, 1) == int(zk.lib.zk_compress_bound_dict(0, 1))
    return n


def test_a_frame_bound_is_what_the_derivation_says():
    for s in (0, 1, 1023, 1024, 1025, 4096, 57281, 262145, 1 << 30):
        assert int(zk.lib.zk_compress_bound(s, max(s, 1))) == s + 3 * -(-max(s, 1) // 1024) + 50, s
        assert int(zk.lib.zk_compress_bound_dict(s, max(s, 1))) == int(zk.lib.zk_compress_bound(s, max(s, 1))) + 4


def test_bound_covers_the_frames_bounds_on_random_lists():
    rng = random.Random(20)
    for trial in range(3000):
        count = rng.randint(1, 60)
        top = rng.choice((2, 300, 1023, 1025, 5000, 70000, 3 << 20))
        sizes = [0 if rng.random() < 0.15 else rng.choice((top, rng.randint(0, top), 1024 * rng.randint(0, 4) + rng.choice((0, 1, 1023)))) for _ in range(count)]
        check(sizes)
    check([1] * 5000)                       # the worst case of the ceilings: every frame rounds up a whole KiB
    check([1025] * 3000)
    check([0] * 100)
    assert int(zk.lib.zk_compress_bound_list(0, 0, 0)) == 0


def test_edge_list_and_the_twins_frames():
    data, off = E.edge_list()
    sizes = [len(f) for f in E.frames_of(data, off)]
    n = check(sizes)
    for level in (1, 3):
        total = sum(len(zko.frame_encode(f, level, True)) for f in E.frames_of(data, off))
        assert total <= int(zk.lib.zk_compress_bound_list(n, len(sizes), 0))
    # incompressible records at the smallest sizes: raw blocks, where a frame is largest against its input
    noise = [zko.gen_random(s, 40 + s) for s in (0, 1, 2, 3, 7, 100, 1024, 1025, 4097)]
    total = sum(len(zko.frame_encode(f, 1, True)) for f in noise)
    assert total <= int(zk.lib.zk_compress_bound_list(sum(map(len, noise)), len(noise), 0))

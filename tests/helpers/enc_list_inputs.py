"""The frame list the tests of zk_encode_frame_list* share: sizes at the encoder's own edges, shuffled, over mixed contents.

Sizes: 0, 1, 7, 255; 4096 / 4097 (the block cut); 57 280 / 57 281 (ZKE_WINDOW: in-frame far history starts); 262 144 / 262 145 (ZKE_SEGMENT: a
second matcher segment); 600 001 (three segments, odd); a run of three more empty frames.  Contents: generated text, random bytes, zero bytes,
and inside every frame beyond the window a far repeat (a piece of the frame's start copied beyond the ring's reach)."""
import functools
import random

import numpy as np

from oracle import zko

WINDOW, SEGMENT = 57280, 262144
EDGE_SIZES = (0, 1, 7, 255, 4096, 4097, WINDOW, WINDOW + 1, SEGMENT, SEGMENT + 1, 600001, 0, 0, 0)


def _content(size, k):
    kind = k % 4
    if size > WINDOW:
        body = bytearray(zko.gen_text(size, 100 + k))
        if kind == 1:
            body[size // 3:size // 3 + 5000] = zko.gen_random(5000, k)
        if kind == 2:
            body[size // 2:size // 2 + 3000] = bytes(3000)
        far = min(4000, size - WINDOW - 1)                   # a repeat the ring cannot reach
        body[size - far:] = body[100:100 + far] if size - far - 100 > WINDOW else body[:far]
        return bytes(body[:size])
    if kind == 0: return zko.gen_text(size, 100 + k)
    if kind == 1: return zko.gen_random(size, 100 + k)
    if kind == 2: return bytes(size)
    return (zko.gen_text(max(size // 2, 1), 100 + k) * 3)[:size]


@functools.lru_cache(maxsize=None)
def edge_list(seed=7, lead=0):
    """(data, offsets): offsets[0] == lead, frame i = data[offsets[i]:offsets[i + 1]] (data holds `lead` bytes in front that belong to no frame)"""
    sizes = list(EDGE_SIZES)
    random.Random(seed).shuffle(sizes)
    parts = [_content(s, k) for k, s in enumerate(sizes)]
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum(sizes)
    data = zko.gen_random(lead, 1) + b"".join(parts)
    assert len(data) < 2_000_000
    return data, off


def frames_of(data, off):
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def small_list(seed, count=40, lo=0, hi=3000, gen=None):
    """a list of small records (sizes drawn evenly from lo..hi, a few empty ones among them)"""
    rng = random.Random(seed)
    sizes = [0 if rng.random() < 0.1 else rng.randint(lo, hi) for _ in range(count)]
    off = np.zeros(count + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    data = (gen or zko.gen_text)(int(off[-1]), seed)
    return data, off

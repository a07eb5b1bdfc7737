"""TEST INFRASTRUCTURE -- frames whose blocks carry the Huffman trees a test asks for, block by block, written with the pieces of
tests/helpers/zstd_gen.py (HufCode, FrameGen.sequences_section, BackBits): what zk_huf_group's pool, passes and tree descriptions depend on
is pinned here, where the random generator only reaches it by chance.

A frame is a list of block specs (depth, streams, form):
  depth    the depth of the block's own tree (a chain code: depth + 1 symbols with code lengths 1, 2, ..., depth, depth, the symbols drawn
           from 0 ... 127), or None for Treeless literals on the tree of the last block that described one
  streams  1 or 4
  form     "direct" | "fse": how the tree description carries the weights (None with Treeless)
Every block has 300 ... 700 literals over all symbols of its tree and one to three sequences on the predefined tables (so that no block
defines a table and zk_k_entropy_frame's walker takes every block), and every frame a 4-byte Frame_Content_Size and a checksum.  The model of
what a frame decodes to is the one the sequences are written from; tests/test_gpu_entropy_passes.py asks the oracle about every frame."""
import random
import struct

from helpers import zstd_gen
from oracle import zko


class _Deepest(random.Random):
    """HufCode splits the leaf this picks: always the last one, which is a deepest one -- a chain of the depth the symbol count gives"""

    def choice(self, seq):
        return seq[-1]


def chain_code(rng, depth):
    huf = zstd_gen.HufCode(_Deepest(rng.getrandbits(32)), rng.sample(range(128), depth + 1))
    assert huf.maxbits == depth
    return huf


def _literals(huf, lits, streams, desc):
    n = len(lits)
    if streams == 1:
        payload, fmt = desc + huf.stream(lits), 0
    else:
        q = (n + 3) // 4
        parts = [huf.stream(lits[i * q:(i + 1) * q]) for i in range(3)] + [huf.stream(lits[3 * q:])]
        payload, fmt = desc + struct.pack("<HHH", *(len(p) for p in parts[:3])) + b"".join(parts), 1
    c = len(payload)
    assert n < 1024 and c < 1024
    return ((2 if desc else 3) | (fmt << 2) | (n << 4) | (c << 14)).to_bytes(3, "little") + payload


def frame(seed, specs):
    """-> (frame bytes, decoded bytes, [offset in the frame of every block's tree description, None for Treeless])"""
    rng = random.Random(seed)
    g = zstd_gen.FrameGen(seed, shared_tables=True)
    g.tables, g.features, g.fact, g.tab_src, g.of_codes = {}, set(), {}, {}, 18
    g.shared_wants = lambda: [0, 0, 0]                           # Predefined_Mode for all three tables, every block
    out, body, huf, desc_at = bytearray(), bytearray(), None, []
    hdr_len = 4 + 1 + 1 + 4
    for i, (depth, streams, form) in enumerate(specs):
        desc = b""
        if depth is not None:
            huf = chain_code(rng, depth)
            d = huf.description(rng, form) or huf.description(rng, "direct")
            assert d is not None, (i, depth, form)               # (form is a wish: weights no FSE description was found for go direct)
            desc = d[0]
        symbols = sorted(huf.code)
        nlit = rng.randint(300, 700)
        lits = bytearray(symbols)                                # every symbol at least once: the deepest cells of the table are read
        # (short codes mostly, as a stream with this tree would have them: the payload stays below 1 KiB)
        by_len = sorted(symbols, key=lambda s: huf.code[s][1])
        while len(lits) < nlit:
            lits.append(by_len[min(int(rng.expovariate(0.7)), len(by_len) - 1)])
        rng.shuffle(lits)
        seqs, used = [], 0
        for _ in range(rng.randint(1, 3)):
            ll = rng.randint(1, 60)
            ml = rng.randint(3, 40)
            out += lits[used:used + ll]; used += ll
            off = rng.randint(1, min(len(out), 200))
            for _ in range(ml): out.append(out[len(out) - off])
            seqs.append((ll, ml, off + 3))
        out += lits[used:]
        block = _literals(huf, bytes(lits), streams, desc) + g.sequences_section(seqs)
        desc_at.append(hdr_len + len(body) + 3 + 3 if desc else None)            # behind the block header and the literals header
        body += ((len(block) << 3) | (2 << 1) | (1 if i + 1 == len(specs) else 0)).to_bytes(3, "little") + block
    assert {x for x in g.features if "_mode" in x} <= {"ll_mode0", "of_mode0", "ml_mode0"}, "predefined tables only"
    exp = 7                                                      # a window of 128 KiB
    assert len(out) <= 1 << (10 + exp)
    f = bytes.fromhex("28B52FFD") + bytes([(2 << 6) | 4, exp << 3]) + struct.pack("<I", len(out)) + bytes(body)
    f += (zko.xxh64(bytes(out)) & 0xFFFFFFFF).to_bytes(4, "little")
    return f, bytes(out), desc_at

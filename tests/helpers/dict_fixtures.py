"""TEST INFRASTRUCTURE -- what tools/make_dict_goldens.py and the dictionary tests share: the record generator behind
tests/golden/dict_archives.*, a reader of the facts a frame's bytes state (header fields, block types, literal types, sequence modes), the
hand-assembled frames whose meaning depends on a dictionary's repeat offsets, and the loader of the fixture pair.

libzstd 1.5.7 made the fixtures; nothing here decodes.  Nothing of the product imports this."""
import json
import os
import struct

from . import zstd_gen as zg

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BIN = os.path.join(ROOT, "tests", "golden", "dict_archives.bin")
IDX = os.path.join(ROOT, "tests", "golden", "dict_archives.json")
DICT_MAGIC = 0xEC30A437
PATCHED_REPS = (24, 57, 131)          # the repeat offsets of the "patched" copy of the trained dictionary


# ---------------------------------------------------------------- records
class Lcg:
    """The generator's only source of randomness (stable whatever Python's random does between versions)."""

    def __init__(self, seed):
        self.s = (seed * 2862933555777941757 + 3037000493) & (2 ** 64 - 1)

    def next(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.s >> 33) % n


_WORDS = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel", "india", "juliet", "kilo", "lima", "mike", "november",
          "oscar", "papa", "quebec", "romeo", "sierra", "tango", "uniform", "victor", "whiskey", "xray", "yankee", "zulu"]
_PATHS = ["/api/v1/items", "/api/v1/users", "/api/v2/search", "/healthz", "/static/app.js", "/login", "/api/v1/orders/history"]
_METHODS = ["GET", "POST", "PUT", "DELETE"]
_STATUS = ["ok", "retry", "timeout", "denied", "ok", "ok"]
_REGIONS = ["eu-west-1", "us-east-2", "ap-south-1", "us-west-1"]


def record(rng):
    """One JSON-like record of 150 ... 400 bytes."""
    f = ['"id": %d' % rng.next(10 ** 9), '"user": "%s_%s%d"' % (_WORDS[rng.next(26)], _WORDS[rng.next(26)], rng.next(1000)),
         '"timestamp": "2024-%02d-%02dT%02d:%02d:%02dZ"' % (1 + rng.next(12), 1 + rng.next(28), rng.next(24), rng.next(60), rng.next(60)),
         '"status": "%s"' % _STATUS[rng.next(6)], '"region": "%s"' % _REGIONS[rng.next(4)], '"latency_ms": %d' % rng.next(5000),
         '"path": "%s"' % _PATHS[rng.next(7)], '"method": "%s"' % _METHODS[rng.next(4)], '"bytes": %d' % rng.next(1 << 20)]
    if rng.next(3) == 0:
        f.append('"tags": [%s]' % ", ".join('"%s"' % _WORDS[rng.next(26)] for _ in range(1 + rng.next(5))))
    if rng.next(4) == 0:
        f.append('"trace": "%016x%016x"' % (rng.next(2 ** 31) * 2654435761, rng.next(2 ** 31) * 40503))
    if rng.next(5) == 0:
        f.append('"error": "%s %s %s"' % (_WORDS[rng.next(26)], _WORDS[rng.next(26)], _WORDS[rng.next(26)]))
    return ("{" + ", ".join(f) + "}\n").encode()


def records(seed, nbytes):
    """Exactly nbytes of records (the last one cut)."""
    rng = Lcg(seed)
    out = bytearray()
    while len(out) < nbytes:
        out += record(rng)
    return bytes(out[:nbytes])


def noise(seed, nbytes):
    rng = Lcg(seed)
    return bytes(rng.next(256) for _ in range(nbytes))


def plain(recipe):
    """The bytes a frame decodes to, from its recipe [kind, seed, nbytes]."""
    kind, seed, n = recipe
    return {"records": records, "noise": noise}[kind](seed, n)


# ---------------------------------------------------------------- what a frame's bytes state
def _lit_header(c):
    t, sf = c[0] & 3, (c[0] >> 2) & 3
    if t < 2:
        if sf in (0, 2):
            hdr, regen = 1, c[0] >> 3
        elif sf == 1:
            hdr, regen = 2, (c[0] >> 4) + (c[1] << 4)
        else:
            hdr, regen = 3, (c[0] >> 4) + (c[1] << 4) + (c[2] << 12)
        return t, hdr, regen, (regen if t == 0 else 1)
    if sf < 2:
        v = int.from_bytes(c[:3], "little"); return t, 3, (v >> 4) & 0x3FF, (v >> 14) & 0x3FF
    if sf == 2:
        v = int.from_bytes(c[:4], "little"); return t, 4, (v >> 4) & 0x3FFF, v >> 18
    v = int.from_bytes(c[:5], "little"); return t, 5, (v >> 4) & 0x3FFFF, (v >> 22) & 0x3FFFF


def frame_facts(f):
    """{"dict_id": the Dictionary_ID field's value or None when there is no field, "checksum": bool, "fcs": int or None,
    "blocks": [(block type, literal type or None, (LL, OF, ML modes) or None)]} of one zstd frame."""
    assert struct.unpack_from("<I", f, 0)[0] == 0xFD2FB528
    fhd = f[4]
    single, did, fcsf = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    p = 5 + (0 if single else 1)
    dl = 4 if did == 3 else did
    dict_id = int.from_bytes(f[p:p + dl], "little") if dl else None
    p += dl
    fl = (1 << fcsf) if fcsf else single
    fcs = (int.from_bytes(f[p:p + fl], "little") + (256 if fl == 2 else 0)) if fl else None
    p += fl
    blocks = []
    while True:
        bh = int.from_bytes(f[p:p + 3], "little"); p += 3
        last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        if bt == 2:
            c = f[p:p + bs]
            lt, hdr, _regen, comp = _lit_header(c)
            q = hdr + comp
            nseq = c[q]
            q += 1 if nseq < 128 else 2 if nseq < 255 else 3
            modes = None
            if c[hdr + comp] != 0:
                m = c[q]
                modes = ((m >> 6) & 3, (m >> 4) & 3, (m >> 2) & 3)
            blocks.append((bt, lt, modes))
        else:
            blocks.append((bt, None, None))
        p += 1 if bt == 1 else bs
        if last:
            break
    if (fhd >> 2) & 1:
        p += 4
    assert p == len(f), (p, len(f))
    return {"dict_id": dict_id, "checksum": bool((fhd >> 2) & 1), "fcs": fcs, "blocks": blocks}


# ---------------------------------------------------------------- dictionaries
def patch_reps(d, header_size, reps=PATCHED_REPS):
    """A copy of formatted dictionary d (Content at header_size) with its three repeat offsets replaced."""
    return d[:header_size - 12] + struct.pack("<3I", *reps) + d[header_size:]


# ---------------------------------------------------------------- frames that mean what the dictionary's repeat offsets say
def rep_frame(dict_id, lits, ofv, ml):
    """One frame, one compressed block: Raw literals `lits` (the sequence takes all of them: Literals_Length = len(lits) <= 15), Predefined
    tables, ONE sequence with offset_value ofv (1, 2 or 3: a repeat code) and Match_Length ml (3 ... 34).  What the match copies depends
    on the repeat offsets the frame starts with -- 1 / 4 / 8 without a dictionary, the dictionary's three with one."""
    ll = len(lits)
    assert ll <= 15 and 3 <= ml <= 34 and ofv in (1, 2, 3)
    llc, mlc = ll, ml - 3
    ofc, ofx = (0, 0) if ofv == 1 else (1, ofv - 2)
    state = lambda norm, al, sym: next(i for i, c in enumerate(zg.fse_cells(norm, al)) if c[0] == sym)
    b = zg.BackBits()
    b.add(state(zg.LL_DEF, 6, llc), 6)
    b.add(state(zg.OF_DEF, 5, ofc), 5)
    b.add(state(zg.ML_DEF, 6, mlc), 6)
    b.add(ofx, ofc)                                   # Offset extra bits; Match_Length / Literals_Length codes below 32 / 16 have none
    content = bytes([ll << 3]) + bytes(lits) + bytes([1, 0]) + b.bytes()
    size = ll + ml
    return (struct.pack("<IB", 0xFD2FB528, 0x23) + struct.pack("<I", dict_id) + bytes([size])      # Single_Segment, 4-byte Dictionary_ID, 1-byte FCS
            + (1 | (2 << 1) | (len(content) << 3)).to_bytes(3, "little") + content)


REP_CASES = [("rep1", b"abcde", 1, 20), ("rep2", b"fghij", 2, 20), ("rep3", b"klmno", 3, 20), ("rep1_minus_1", b"", 3, 20)]


# ---------------------------------------------------------------- the fixture pair
def load():
    with open(IDX) as fh:
        idx = json.load(fh)
    with open(BIN, "rb") as fh:
        blob = fh.read()
    return idx, blob


def piece(blob, ent):
    return blob[ent["offset"]:ent["offset"] + ent["length"]]


def archive(blob, case):
    """(compressed bytes of the case's frames back to back, c_off, d_off) -- prefix sums as Python lists."""
    comp = bytearray()
    c, d = [0], [0]
    for fr in case["frames"]:
        comp += piece(blob, fr)
        c.append(len(comp)); d.append(d[-1] + fr["d_size"])
    return bytes(comp), c, d

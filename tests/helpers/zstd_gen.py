"""TEST INFRASTRUCTURE -- a generator of VALID zstd frames that no encoder here would write: every choice the format leaves open (RFC 8878) is
drawn at random, so that the decoders meet corners the libzstd-made goldens only reach by chance:

  frame header   Single_Segment or a Window_Descriptor (exponent + mantissa), Frame_Content_Size of 0 / 1 / 2 / 4 / 8 bytes, checksum or not,
                 a Dictionary_ID field of any width holding 0, the Unused_Bit
  blocks         Raw, RLE, Compressed in any order; empty blocks; a last block of any type
  literals       Raw / RLE (1-, 2-, 3-byte headers), Huffman with 1 or 4 streams (a random complete code of depth <= 11; weights direct or FSE-compressed),
                 Treeless (the table of an earlier block)
  sequences      0 ... a few hundred per block; Predefined / RLE / FSE_Compressed (random normalised counts, "less than 1" probabilities,
                 zero runs, any legal accuracy log) / Repeat mode per table, independently; 1-, 2-, 3-byte Number_of_Sequences
  offsets        new offsets up to the window, the three repeat codes with and without Literals_Length 0 (incl. "Repeated_Offset1 - 1")

It writes the bytes AND runs the sequences on a model of its own; what the frame MEANS is still decided by the real libzstd 1.5.7 in the tests that
use it (tests/test_generated_frames.py: libzstd, the oracle, the lane code on the CPU; tests/test_gpu_generated_frames.py: the kernels) -- the
model's output only has to agree with it, which checks the generator.  Nothing of the product imports this.

Keywords beyond the defaults (with the defaults a seed gives the bytes it always gave: every further draw sits behind its keyword):
  stats=True       generate() also returns the facts of every block of the frame, in order, as dicts: type ("raw" | "rle" | "comp"), and for a
                   compressed block lit ("raw" | "rle" | "huf" | "treeless"), streams (0 | 1 | 4), nlit, huf_depth and huf_def (the longest code of
                   the tree the literals use and the index IN THE FRAME of the block that carries its description; None without Huffman), nseq,
                   modes (the Symbol_Compression_Modes byte; None without sequences), ll_codes / ml_codes (sets), max_ll, max_ml, max_ml_off1
  shared_tables    frames of 16 ... 80 blocks whose first block with sequences describes all three tables over every code the frame may use;
                   later blocks mostly say Repeat_Mode (or Predefined_Mode) for all three, seldom redefine one table, use RLE_Mode or mix
  max_ll / max_ml  upper ends of a long tail of literal lengths / match lengths (drawn by code, so the codes with 11 ... 16 extra bits come up),
                   up to the block size; long matches mostly at offset 1.  max_lit has to allow the literals
  dictionary       a Dictionary (the model make_dictionary / raw_dictionary return): the frame is written against it -- its content lies below
                   the frame's first byte, and with a formatted one the frame starts from its repeat offsets, its Huffman tree (Treeless
                   literals in a first block) and its three tables (Repeat_Mode per table, independently, until a block says otherwise);
                   the Dictionary_ID field has any width that holds the ID, or is absent.  Offsets stay within the window and within what
                   is available, as with a prefix.  Features (they count for blocks the frame keeps): dict_treeless_first_1stream /
                   _4streams (the frame's first compressed block), dict_ll_repeat / dict_of_repeat / dict_ml_repeat and, with the mode of
                   each other table, dict_ll_repeat_of_mode0 ..., dict_table_after_redefine (another table was described or set by an
                   earlier block), dict_first_comp_not_block0 (the first compressed block uses the dictionary and is not the frame's
                   first block), dict_rep_first_idx0 ... 3 (the frame's first sequence takes a repeat offset of the dictionary; 3 is
                   Repeated_Offset1 - 1), off_into_dict, off_dict_first_byte, match_straddles_frame_start, did_width1 / 2 / 4, did_absent.
                   stats=True: huf_def is "dict" where the tree in use is the dictionary's"""
import random
import struct

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEF) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEF) == 53 and len(OF_DEF) == 29


class BackBits:
    """A backward bitstream (RFC 8878 4.1): fields are added in the order the READER meets them."""

    def __init__(self):
        self.acc, self.n = 1, 0

    def add(self, v, w):
        assert 0 <= v < (1 << w) or (w == 0 and v == 0)
        self.acc = (self.acc << w) | v
        self.n += w

    def bytes(self):
        return self.acc.to_bytes((self.n + 1 + 7) // 8, "little")


class FwdBits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def add(self, v, w):
        assert 0 <= v < (1 << w)
        self.acc |= v << self.n
        self.n += w

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def fse_cells(norm, al):
    """The decoding table of RFC 8878 4.1.1 as [(symbol, number of bits, baseline)]"""
    size, high = 1 << al, (1 << al) - 1
    sym = [0] * size
    nxt = []
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s; high -= 1; nxt.append(1)
        else:
            nxt.append(c)
    step, pos, mask = (size >> 1) + (size >> 3) + 3, 0, size - 1
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0
    cells = []
    for i in range(size):
        s = sym[i]
        x = nxt[s]; nxt[s] += 1
        nb = al - (x.bit_length() - 1)
        cells.append((s, nb, (x << nb) - size))
    return cells


def write_ncount(norm, al):
    """FSE table description (RFC 8878 4.1.1): the mirror of the oracle's fse_read_ncount"""
    f = FwdBits()
    f.add(al - 5, 4)
    remaining, threshold, nb = (1 << al) + 1, 1 << al, al + 1
    s = 0
    while remaining > 1:
        cnt = norm[s]; s += 1
        v, mx = cnt + 1, 2 * threshold - 1 - remaining
        if v < mx: f.add(v, nb - 1)
        elif v < threshold: f.add(v, nb)
        else: f.add(v + mx, nb)
        remaining -= abs(cnt)
        if cnt == 0:
            z = 0
            while s + z < len(norm) and norm[s + z] == 0: z += 1
            s += z
            while z >= 3: f.add(3, 2); z -= 3
            f.add(z, 2)
        while remaining < threshold:
            nb -= 1; threshold >>= 1
    assert remaining == 1 and all(c == 0 for c in norm[s:])
    return f.bytes()


def random_norm(rng, used, nsym, al_lo, al_hi):
    """normalised counts over symbols 0..nsym-1 with every symbol of `used` present: (norm, accuracy log)"""
    used = sorted(set(used) | ({rng.randrange(nsym)} if rng.random() < 0.5 else set()))
    lo = al_lo
    while (1 << lo) < len(used): lo += 1
    al = rng.randint(lo, al_hi)
    size = 1 << al
    norm = [0] * nsym
    left = size
    for s in used:
        if rng.random() < 0.3: norm[s] = -1
        else: norm[s] = 1
        left -= 1
    while left:                                              # the rest to random symbols (not the "less than 1" ones), in lumps
        s = rng.choice(used)
        if norm[s] == -1:
            if all(norm[u] == -1 for u in used): norm[s] = 1
            continue
        k = rng.randint(1, max(1, left // 2)) if rng.random() < 0.5 else 1
        norm[s] += k; left -= k
    while norm and norm[-1] == 0: norm.pop()
    return norm, al


def code_of(v, base, bits):
    c = len(base) - 1
    while base[c] > v: c -= 1
    assert v - base[c] < (1 << bits[c])
    return c, v - base[c], bits[c]


class HufCode:
    """a random complete prefix code of depth <= 11 over `symbols` (>= 2 of them; the largest symbol's weight is the implied one)"""

    def __init__(self, rng, symbols):
        symbols = sorted(symbols)
        assert len(symbols) >= 2
        depths = [1, 1]
        while len(depths) < len(symbols):
            cand = [i for i, d in enumerate(depths) if d < 11]
            i = rng.choice(cand)
            d = depths.pop(i) + 1
            depths += [d, d]
        rng.shuffle(depths)
        self.maxbits = max(depths)
        self.weights = [0] * (symbols[-1] + 1)
        for s, d in zip(symbols, depths): self.weights[s] = self.maxbits + 1 - d
        pos, self.code = 0, {}
        for wt in range(1, self.maxbits + 1):
            for s, w in enumerate(self.weights):
                if w == wt:
                    nb = self.maxbits + 1 - wt
                    self.code[s] = (pos >> (self.maxbits - nb), nb)
                    pos += 1 << (wt - 1)
        assert pos == 1 << self.maxbits

    def description(self, rng, form=None):
        """-> (bytes, "direct" | "fse") or None: four bits per weight, or the weights as an FSE stream on two interleaved states (RFC 8878 4.2.1.2).
        form: the one to take (None where the weights do not allow it); drawn without"""
        w = self.weights[:-1]
        if form == "direct" and len(w) > 128 or form == "fse" and len(w) < 2: return None
        if form == "direct" or (form is None and len(w) <= 128 and (len(w) < 2 or rng.random() < 0.5)):
            out = bytearray([127 + len(w)])
            for i in range(0, len(w), 2):
                out.append((w[i] << 4) | (w[i + 1] if i + 1 < len(w) else 0))
            return bytes(out), "direct"
        for _ in range(8):
            norm, al = random_norm(rng, w, 12, 5, 6)
            cells = fse_cells(norm, al)
            # state A decodes w[0], w[2], ..., state B w[1], w[3], ...; the reader stops when the state that gave w[n - 2] cannot be
            # updated any more (it would read past the start) -- so that state's last cell has to ask for at least one bit
            n = len(w)
            chains = []
            for start in (0, 1):
                idx = list(range(start, n, 2))
                last = [k for k, c in enumerate(cells) if c[0] == w[idx[-1]] and (c[1] > 0 or idx[-1] != n - 2)]
                if not last: break
                states, bits = [rng.choice(last)], []
                for i in reversed(idx[:-1]):
                    nxt = states[0]
                    k = next(k for k, c in enumerate(cells) if c[0] == w[i] and c[2] <= nxt < c[2] + (1 << c[1]))
                    bits.insert(0, (nxt - cells[k][2], cells[k][1])); states.insert(0, k)
                chains.append((states, bits))
            if len(chains) < 2: continue
            b = BackBits()
            b.add(chains[0][0][0], al); b.add(chains[1][0][0], al)
            for k in range(n - 2):
                b.add(*chains[k & 1][1][k >> 1])
            body = write_ncount(norm, al) + b.bytes()
            if 2 <= len(body) < 128: return bytes([len(body)]) + body, "fse"
        return None

    def stream(self, data):
        b = BackBits()
        for x in data:                                      # symbols are decoded first to last, each from the top of what is left
            c, nb = self.code[x]
            b.add(c, nb)
        return b.bytes()


class FrameGen:
    def __init__(self, seed, max_blocks=6, max_seq=300, max_lit=3000, prefix=b"", dense=False, shared_tables=False, max_ll=None, max_ml=None, dictionary=None):
        self.rng = random.Random(seed)
        self.want_dense = dense                              # one block of the frame with more than 0x7F00 sequences
        self.prefix = bytes(prefix)                          # a raw-content prefix the frame is written against (ZSTD_CCtx_refPrefix): offsets reach into it
        self.dict = dictionary                               # a Dictionary (make_dictionary): its content is the prefix, the frame starts from its tree, tables, offsets
        if dictionary is not None:
            assert not prefix
            self.prefix = dictionary.content
        self.bfeat = set()                                   # dictionary features of the block being written (they count once the block is kept)
        self.max_blocks, self.max_seq, self.max_lit = max_blocks, max_seq, max_lit
        self.features = set()
        self.shared, self.max_ll, self.max_ml = shared_tables, max_ll, max_ml
        self.fact = {}                                       # the facts of the block being written (module docstring: stats=True)

    # ---- literals
    def literals_section(self, lits):
        rng = self.rng
        n = len(lits)
        alphabet = sorted(set(lits))
        kinds = ["raw"]
        if n and len(alphabet) == 1: kinds += ["rle"] * 3
        if n >= 2 and len(alphabet) >= 2: kinds += ["huf"] * 4
        if n >= 1 and self.huf is not None and all(x in self.huf.code for x in alphabet): kinds += ["treeless"] * 8
        kind = rng.choice(kinds)
        self.features.add("lit_" + kind)
        self.fact.update(lit=kind, nlit=n, streams=0, huf_depth=None, huf_def=None)
        if kind in ("raw", "rle"):
            t = 0 if kind == "raw" else 1
            fmts = [f for f, cap in ((1, 1 << 12), (3, 1 << 20)) if n < cap] + ([0, 0] if n < 32 else [])
            f = rng.choice(fmts)
            if f == 0: hdr = bytes([t | (n << 3)])          # Size_Format ?0: one bit, the size's five bits start at bit 3
            elif f == 1: hdr = struct.pack("<H", t | (1 << 2) | (n << 4))
            else: hdr = (t | (3 << 2) | (n << 4)).to_bytes(3, "little")
            self.features.add("lit_hdr%d" % len(hdr))
            return hdr + (bytes(lits) if kind == "raw" else bytes(lits[:1]))
        if kind == "huf":
            extra = set(rng.sample(range(0, 256), rng.randint(0, 3))) if rng.random() < 0.3 else set()
            huf = HufCode(rng, set(alphabet) | extra)
            d = huf.description(rng)
            if d is None: return None
            self.huf, desc = huf, d[0]
            huf.block = self.block_index                     # (rides on the object: a block that is given up restores the code before it)
            self.features.add("huf_weights_" + d[1])
        else:
            desc = b""
        one = n < 1024 and (n < 8 or rng.random() < 0.4)
        if kind == "treeless" and self.huf.block == "dict":
            self.bfeat.add("dict_treeless")
            if not self.comp_seen: self.bfeat.add("dict_treeless_first_%s" % ("1stream" if one else "4streams"))
        if one:
            payload = desc + self.huf.stream(lits)
            streams_fmt = [0]
        else:
            q = (n + 3) // 4
            parts = [self.huf.stream(lits[i * q:(i + 1) * q]) for i in range(3)] + [self.huf.stream(lits[3 * q:])]
            if any(len(p) > 0xFFFF for p in parts[:3]): return None
            payload = desc + struct.pack("<HHH", *(len(p) for p in parts[:3])) + b"".join(parts)
            streams_fmt = [1, 2, 3]
        c = len(payload)
        self.fact.update(streams=1 if one else 4, huf_depth=self.huf.maxbits, huf_def=self.huf.block)
        fmts = [f for f in streams_fmt if (f <= 1 and n < 1024 and c < 1024) or (f == 2 and n < 16384 and c < 16384) or (f == 3 and n < (1 << 18) and c < (1 << 18))]
        if not fmts: return None
        f = rng.choice(fmts)
        t = 2 if kind == "huf" else 3
        self.features.add("huf_streams%d" % (1 if one else 4)); self.features.add("huf_fmt%d" % f)
        if f <= 1: hdr = (t | (f << 2) | (n << 4) | (c << 14)).to_bytes(3, "little")
        elif f == 2: hdr = (t | (2 << 2) | (n << 4) | (c << 18)).to_bytes(4, "little")
        else: hdr = (t | (3 << 2) | (n << 4) | (c << 22)).to_bytes(5, "little")
        return hdr + payload

    # ---- sequences
    def table_for(self, which, codes, nsym, al_lo, al_hi, default, default_al, want=None, full=None):
        """-> (mode, description bytes, cells, accuracy log) for the table `which` given the codes this block uses.
        want (shared_tables): the mode to take if the codes allow it, FSE_Compressed otherwise; full: the codes a description then covers"""
        rng = self.rng
        modes = []
        if all(c < len(default) and default[c] != 0 for c in codes): modes += [0, 0]
        if len(set(codes)) == 1: modes += [1, 1]
        modes += [2, 2]
        prev = self.tables.get(which)
        if prev is not None and all(any(cell[0] == c for cell in prev[0]) for c in set(codes)): modes += [3, 3]
        if want is None: mode = rng.choice(modes)
        else:
            mode = want if want in modes else 2
            if mode == 2: codes = sorted(set(codes) | set(full))
        self.features.add("%s_mode%d" % (which, mode))
        if mode == 0: cells, al, desc = fse_cells(default, default_al), default_al, b""
        elif mode == 1: cells, al, desc = [(codes[0], 0, 0)], 0, bytes([codes[0]])
        elif mode == 2:
            norm, al = random_norm(rng, codes, nsym, al_lo, al_hi)
            if -1 in norm: self.features.add("fse_lowprob")
            cells, desc = fse_cells(norm, al), write_ncount(norm, al)
        else: cells, al = prev; desc = b""
        if self.dict is not None:
            if mode != 3: self.tab_src[which] = self.block_index
            elif self.tab_src[which] == "dict": self.bfeat.add("dict_%s_repeat" % which)
        self.tables[which] = (cells, al)
        return mode, desc, cells, al

    def shared_wants(self):
        """shared_tables: the three modes this block would like (table_for takes FSE_Compressed over all codes where the block's codes forbid one)"""
        rng = self.rng
        if not self.tables: return [2, 2, 2]                 # the frame's first block with sequences describes all three
        r = rng.random()
        if r < 0.90: return [3, 3, 3]
        if r < 0.93: return [0, 0, 0]                         # (a Repeat_Mode behind it repeats the predefined table)
        if r < 0.96: return [rng.choice([0, 3]) for _ in range(3)]
        w = [3, 3, 3]
        w[rng.randrange(3)] = 2 if r < 0.98 else 1
        return w

    def sequences_section(self, seqs):
        """seqs: [(ll, ml, offset_value)] -> bytes"""
        rng = self.rng
        n = len(seqs)
        self.fact.update(nseq=n, modes=None, ll_codes=set(), ml_codes=set(), max_ll=max([s[0] for s in seqs], default=0), max_ml=max([s[1] for s in seqs], default=0))
        if n == 0: return b"\x00"
        form = 3 if n >= 0x7F00 else 2 if n >= 128 else rng.choice([1, 1, 1, 2])       # (the two-byte form may carry a small count)
        if form == 1: hdr = bytes([n])
        elif form == 2: hdr = bytes([128 + (n >> 8), n & 255])
        else: hdr = bytes([255]) + struct.pack("<H", n - 0x7F00)
        self.features.add("nseq_form%d" % form)
        ll = [code_of(s[0], LL_BASE, LL_BITS) for s in seqs]
        ml = [code_of(s[1], ML_BASE, ML_BITS) for s in seqs]
        of = []
        for s in seqs:
            c = s[2].bit_length() - 1
            of.append((c, s[2] - (1 << c), c))
        wants, full = self.shared_wants() if self.shared else (None, None, None), (range(36), range(self.of_codes), range(53))
        src_before = dict(self.tab_src) if self.dict is not None else {}
        m_ll, d_ll, c_ll, a_ll = self.table_for("ll", [x[0] for x in ll], 36, 5, 9, LL_DEF, 6, wants[0], full[0])
        m_of, d_of, c_of, a_of = self.table_for("of", [x[0] for x in of], 32, 5, 8, OF_DEF, 5, wants[1], full[1])
        m_ml, d_ml, c_ml, a_ml = self.table_for("ml", [x[0] for x in ml], 53, 5, 9, ML_DEF, 6, wants[2], full[2])
        self.fact.update(modes=(m_ll << 6) | (m_of << 4) | (m_ml << 2), ll_codes={x[0] for x in ll}, ml_codes={x[0] for x in ml})
        now = {"ll": m_ll, "of": m_of, "ml": m_ml}
        for t in now:                                        # a table of the dictionary repeated: beside what, and behind what
            if "dict_%s_repeat" % t in self.bfeat:
                for o in now:
                    if o != t: self.bfeat.add("dict_%s_repeat_%s_mode%d" % (t, o, now[o]))
                if any(src_before[o] != "dict" for o in now if o != t): self.bfeat.add("dict_table_after_redefine")

        def chain(cells, codes):
            """states[i] of a decoder that sees codes[i] in state i, and the bits that take it from i to i + 1"""
            by_sym = {}
            for k, cell in enumerate(cells): by_sym.setdefault(cell[0], []).append(k)
            states, bits = [rng.choice(by_sym[codes[-1]])], []
            for c in reversed(codes[:-1]):
                nxt = states[-1]
                k = next(k for k in by_sym[c] if cells[k][2] <= nxt < cells[k][2] + (1 << cells[k][1]))
                bits.append((nxt - cells[k][2], cells[k][1]))
                states.append(k)
            states.reverse(); bits.reverse()
            return states, bits
        s_ll, b_ll = chain(c_ll, [x[0] for x in ll])
        s_of, b_of = chain(c_of, [x[0] for x in of])
        s_ml, b_ml = chain(c_ml, [x[0] for x in ml])
        b = BackBits()
        b.add(s_ll[0], a_ll); b.add(s_of[0], a_of); b.add(s_ml[0], a_ml)
        for i in range(n):
            b.add(of[i][1], of[i][2]); b.add(ml[i][1], ml[i][2]); b.add(ll[i][1], ll[i][2])
            if i + 1 < n:
                b.add(*b_ll[i]); b.add(*b_ml[i]); b.add(*b_of[i])
        return hdr + bytes([(m_ll << 6) | (m_of << 4) | (m_ml << 2)]) + d_ll + d_of + d_ml + b.bytes()

    # ---- a compressed block: sequences on the model, then the two sections
    def compressed_block(self, out, rep, window, block_max):
        rng = self.rng
        nseq = 0 if rng.random() < 0.15 else rng.randint(1, rng.choice([3, 20, self.max_seq]))
        style = rng.random()
        dense = self.dense and block_max == 1 << 17 and len(out) >= 8
        if dense: nseq = rng.randint(0x7F00, 0x7F00 + 6000)     # the three-byte Number_of_Sequences: matches of 3 ... 4 bytes back to back
        self.dense = self.dense and not dense
        if self.alpha is not None and rng.random() < 0.4: alpha = bytes(rng.sample(list(self.alpha), rng.randint(1, len(self.alpha))))   # (a block the table of the one before fits: Treeless)
        else: alpha = bytes(rng.sample(range(0, rng.choice([129, 256])), rng.randint(1, rng.choice([2, 6, 40, 100])))) if rng.random() < 0.8 else bytes(range(256))
        self.alpha = alpha
        lits, seqs = bytearray(), []
        produced = max_ml_off1 = 0
        start = len(out)
        for _ in range(nseq):
            ll = 0 if rng.random() < 0.3 else rng.choice([rng.randint(1, 8), rng.randint(1, 40), rng.randint(1, 2000 if style < 0.1 else 60)])
            ml = rng.choice([3, rng.randint(3, 12), rng.randint(3, 130), rng.randint(3, 3000 if style < 0.1 else 200)])
            if dense: ll, ml = (1 if rng.random() < 0.02 else 0), (3 if rng.random() < 0.9 else 4)
            off1 = False
            if self.max_ll is not None and rng.random() < 0.08:          # the long tail, by code: 16 ... 35, cut to what the block still holds
                c = rng.choice([rng.randint(16, 35), rng.randint(27, 35), 35])
                ll = min(LL_BASE[c] + rng.randrange(1 << LL_BITS[c]), self.max_ll, self.max_lit - len(lits), block_max - produced - 3)
                if ll < 0: break
            if self.max_ml is not None and rng.random() < 0.08:          # codes 32 ... 52
                c = rng.choice([rng.randint(32, 52), rng.randint(46, 52), 52])
                ml = min(ML_BASE[c] + rng.randrange(1 << ML_BITS[c]), self.max_ml, block_max - produced - ll)
                if ml < 3: break
                off1 = rng.random() < 0.6
            if len(lits) + ll > self.max_lit or produced + ll + ml > block_max: break
            here = len(self.prefix) + len(out) + ll           # bytes available behind the literals
            reach = min(here, window)                         # (an offset beyond the window into a prefix: libzstd takes it until its ring wraps -- not valid zstd, not drawn)
            r = rng.random() if not (off1 and here) else 1.0
            ofv = None
            if off1 and here: off, ofv = 1, 4                 # (a long match of one byte's run)
            if r < 0.45:                                      # a repeat code
                code = rng.randint(1, 3)
                idx = code - 1 + (1 if ll == 0 else 0)
                off = rep[0] if idx == 0 else (rep[0] - 1 if idx == 3 else rep[idx])
                if 0 < off <= reach: ofv = code
            if ofv is None:
                if here == 0: continue
                hi = reach
                off = rng.choice([1, rng.randint(1, min(hi, 16)), rng.randint(1, hi), hi, max(1, min(hi, len(out) + ll + rng.randint(0, 40)))])   # (the last: around the frame's first byte, where a prefix begins)
                ofv = off + 3
            if ofv > 3: rep = [ofv - 3, rep[0], rep[1]]; self.features.add("off_new")
            else:
                idx = ofv - 1 + (1 if ll == 0 else 0)
                self.features.add("rep_idx%d" % idx)
                if self.dict is not None and self.dict.formatted and not self.seq_seen and not seqs: self.bfeat.add("dict_rep_first_idx%d" % idx)
                if idx:
                    off = rep[0] - 1 if idx == 3 else rep[idx]
                    rep = [off, rep[0], rep[1]] if idx > 1 else [off, rep[0], rep[2]]
            new = bytes(rng.choice(alpha) for _ in range(ll))
            lits += new; out += new
            self.max_off = max(self.max_off, off)
            if off > len(out): self.features.add("off_into_prefix")
            if self.dict is not None and off > len(out):
                self.bfeat.add("off_into_dict")
                if off == len(out) + len(self.prefix): self.bfeat.add("off_dict_first_byte")
                if ml > off - len(out): self.bfeat.add("match_straddles_frame_start")
            for _ in range(ml):
                i = len(out) - off
                out.append(out[i] if i >= 0 else self.prefix[len(self.prefix) + i])
            produced += ll + ml
            seqs.append((ll, ml, ofv))
            if off == 1: max_ml_off1 = max(max_ml_off1, ml)
        tail = rng.randint(0, min(self.max_lit - len(lits), block_max - produced, rng.choice([0, 5, 300, 3000])))
        new = bytes(rng.choice(alpha) for _ in range(tail))
        lits += new; out += new
        lit = self.literals_section(lits)
        if lit is None: return None, rep
        body = lit + self.sequences_section(seqs)
        self.fact.update(max_ml_off1=max_ml_off1)
        if len(body) > block_max or len(body) >= (1 << 21): return None, rep
        return body, rep

    def frame(self):
        """-> (frame bytes, decoded bytes, features)"""
        rng = self.rng
        while True:
            self.huf, self.tables, self.alpha = None, {}, None
            self.features = set()
            self.tab_src, self.comp_seen, self.seq_seen = {}, 0, 0
            if self.dict is not None and self.dict.formatted:
                self.huf, self.tables, self.alpha = self.dict.huf, dict(self.dict.tables), bytes(sorted(self.dict.huf.code))
                self.tab_src = {"ll": "dict", "of": "dict", "ml": "dict"}
            self.max_off = 0
            self.dense = self.want_dense
            exp, mant = rng.choice([0, 0, 1, 3, 7, rng.randint(0, 10)]), rng.randint(0, 7)
            if (self.max_ll is not None or self.max_ml is not None) and rng.random() < 0.7: exp = rng.randint(7, 10)     # blocks of 128 KiB
            window = (1 << (10 + exp)) + ((1 << (10 + exp)) >> 3) * mant
            block_max = min(window, 1 << 17)
            self.of_codes = (window + 3).bit_length()         # offset codes 0 ... log2 of the largest Offset_Value
            out, rep = bytearray(), (list(self.dict.rep) if self.dict is not None else [1, 4, 8])
            blocks, facts = [], []
            ok = True
            nblocks = rng.randint(16, 80) if self.shared else rng.randint(1, self.max_blocks)
            for _ in range(2 * nblocks if self.shared else nblocks):        # (shared_tables: a block that is given up is drawn again)
                if len(blocks) == nblocks: break
                r = rng.random()
                self.block_index = len(blocks)
                if r < 0.15:
                    n = rng.choice([0, rng.randint(0, 40), rng.randint(0, min(block_max, 5000))])
                    data = bytes(rng.randrange(256) for _ in range(n))
                    blocks.append((0, n, data)); out += data; self.features.add("raw"); facts.append({"type": "raw"})
                elif r < 0.3:
                    n = rng.choice([0, 1, rng.randint(0, 300), rng.randint(0, block_max)])
                    v = rng.randrange(256)
                    blocks.append((1, n, bytes([v]))); out += bytes([v]) * n; self.features.add("rle"); facts.append({"type": "rle"})
                else:
                    snap = (len(out), list(rep), self.huf, dict(self.tables), dict(self.tab_src))
                    self.fact = {"type": "comp"}
                    self.bfeat = set()
                    body, rep2 = self.compressed_block(out, rep, window, block_max)
                    if body is None:
                        del out[snap[0]:]; rep, self.huf, self.tables, self.tab_src = snap[1], snap[2], snap[3], snap[4]
                        continue
                    rep = rep2
                    if self.dict is not None:
                        if not self.comp_seen and blocks and any(x.startswith("dict_") for x in self.bfeat): self.bfeat.add("dict_first_comp_not_block0")
                        self.features |= self.bfeat
                        self.comp_seen += 1; self.seq_seen += self.fact["nseq"]
                    blocks.append((2, len(body), body)); self.features.add("compressed"); facts.append(self.fact)
            if not blocks or self.dense: continue               # (a dense block was asked for and did not come about: window too small, ...)
            total = len(out)
            # Single_Segment: the window IS the content size, and Block_Maximum_Size follows it -- also for what a block holds
            single = total <= window and rng.random() < 0.4 and all(n <= min(total, 1 << 17) for t, n, _ in blocks if t == 2) and self.max_off <= total
            cks = rng.random() < 0.5
            if single:
                flags = [f for f, lo, hi in ((0, 0, 255), (1, 256, 65791), (2, 0, (1 << 32) - 1), (3, 0, (1 << 64) - 1)) if lo <= total <= hi]
                fcs_flag = rng.choice(flags)
            else:
                fcs_flag = rng.choice([0, 0] + [f for f, lo, hi in ((1, 256, 65791), (2, 0, (1 << 32) - 1), (3, 0, (1 << 64) - 1)) if lo <= total <= hi])
            if self.dict is None:
                did, idv = rng.choice([0, 0, 0, 1, 2, 3]), 0  # a Dictionary_ID field of 1 / 2 / 4 bytes holding 0 = "no dictionary" (RFC 8878 3.1.1.1.3)
            else:                                            # no field, or one of any width that holds the dictionary's ID
                idv = self.dict.id
                did = rng.choice([0] + [f for f, w in ((1, 1), (2, 2), (3, 4)) if idv < (1 << (8 * w))])
                self.features.add("did_width%d" % (0, 1, 2, 4)[did] if did else "did_absent")
            unused = 0x10 if rng.random() < 0.2 else 0         # Unused_Bit: a decoder shall not interpret it
            fhd = (fcs_flag << 6) | (0x20 if single else 0) | unused | (4 if cks else 0) | did
            hdr = bytes.fromhex("28B52FFD") + bytes([fhd]) + (b"" if single else bytes([(exp << 3) | mant])) + (idv if did else 0).to_bytes((0, 1, 2, 4)[did], "little")
            if did: self.features.add("did_field")
            if unused: self.features.add("unused_bit")
            if single and fcs_flag == 0: hdr += bytes([total])
            elif fcs_flag == 1: hdr += struct.pack("<H", total - 256)
            elif fcs_flag == 2: hdr += struct.pack("<I", total)
            elif fcs_flag == 3: hdr += struct.pack("<Q", total)
            self.features.add("single" if single else "windowed"); self.features.add("fcs%d" % fcs_flag)
            body = bytearray()
            for i, (t, n, payload) in enumerate(blocks):
                body += ((n << 3) | (t << 1) | (1 if i + 1 == len(blocks) else 0)).to_bytes(3, "little") + payload
            self.facts = facts
            return bytes(hdr + body), bytes(out), cks, set(self.features)


class Dictionary:
    """what make_dictionary returns beside the bytes: the model a frame written against the dictionary starts from.
    formatted (False: raw content, every byte is content and nothing else is lent), id, content, content_offset, rep (three offsets),
    huf (a HufCode whose `block` is "dict"), huf_form ("direct" | "fse"), tables {"ll" | "of" | "ml": (cells, accuracy log)},
    norms {"ll" | "of" | "ml": normalised counts}, spans {"huf" | "of" | "ml" | "ll" | "rep": (offset, length) in the bytes}"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def raw_dictionary(content):
    """-> (bytes, Dictionary) of a raw-content dictionary: ID 0, no tables, repeat offsets 1 / 4 / 8"""
    content = bytes(content)
    assert len(content) < 8 or content[:4] != bytes.fromhex("37A430EC")
    return content, Dictionary(formatted=False, id=0, content=content, content_offset=0, rep=(1, 4, 8), huf=None, huf_form=None, tables={}, norms={}, spans={})


DICT_SIZES = (1, 7, 8, 9)


def make_dictionary(seed, dict_id=None, content_size=None, alphabet=None, weights=None, depth=None, als=None, reps=None, wide=False):
    """-> (bytes, Dictionary): a formatted dictionary (RFC 8878 5) nobody trained -- magic, Dictionary_ID, a Huffman tree description, FSE
    descriptions of the Offset, Match_Length and Literals_Length codes in that order, three repeat offsets, content -- with everything drawn:
      ID        0, below 256, below 65 536, any 32-bit value
      tree      2 ... 256 symbols, depth <= 11, weights direct (symbols below 129 then) or FSE-compressed
      tables    random_norm over any legal accuracy log (OF 5 ... 8, ML and LL 5 ... 9), "less than 1" entries, absent symbols
      offsets   1, the content size, anything between, equal ones
      content   1, 7, 8, 9, a few hundred bytes, a few KiB, more than 128 KiB of random bytes
    Keywords pin a draw: dict_id, content_size, alphabet (number of symbols), weights ("direct" | "fse"), depth (of the tree),
    als ({"ll" | "of" | "ml": accuracy log}), reps (three offsets), wide (every table covers every code its accuracy log has room for:
    with logs of 6 and more a frame can say Repeat_Mode whatever it holds)."""
    rng = random.Random(0x5EED0000 + seed)
    r = rng.random()
    idv = 0 if r < 0.04 else rng.randint(1, 255) if r < 0.3 else rng.randint(256, 65535) if r < 0.55 else rng.randint(65536, (1 << 32) - 1)
    if dict_id is not None: idv = dict_id
    n = rng.choice(list(DICT_SIZES) + [rng.randint(100, 900)] * 4 + [rng.randint(1024, 8192)] * 4 + [rng.randint((1 << 17) + 1, 200000)])
    if content_size is not None: n = content_size
    content = rng.randbytes(n)
    form = weights or rng.choice(["direct", "fse"])
    for _ in range(4000):
        nsym = alphabet or rng.choice([2, 3, rng.randint(4, 20), rng.randint(20, 128), rng.randint(129, 255), 256])
        pool = 129 if form == "direct" else 256
        if depth is not None and alphabet is None: nsym = max(nsym, 40)
        nsym = min(nsym, pool)
        huf = HufCode(rng, rng.sample(range(pool), nsym))
        if depth is not None and huf.maxbits != depth: continue
        d = huf.description(rng, form)
        if d is not None: break
    else:
        raise AssertionError("no tree description for these keywords")
    huf.block = "dict"
    tables, norms, descs = {}, {}, {}
    for which, nsym, hi in (("of", 32, 8), ("ml", 53, 9), ("ll", 36, 9)):
        al = (als or {}).get(which) or rng.randint(5, hi)
        cap = min(nsym, (1 << al) - 1)
        top = cap if which != "of" else min(cap, rng.randint(20, 31))      # (offset codes: at least what a window of a few MiB needs)
        used = range(top) if rng.random() < 0.7 else rng.sample(range(nsym), rng.randint(1, cap))
        if wide: used = range(cap)
        norm, al = random_norm(rng, used, nsym, al, al)
        tables[which], norms[which], descs[which] = (fse_cells(norm, al), al), norm, write_ncount(norm, al)
    if reps is None:
        reps = [rng.choice([1, n, rng.randint(1, n), rng.randint(1, min(n, 16))]) for _ in range(3)]
        if rng.random() < 0.2: reps[rng.randrange(3)] = reps[rng.randrange(3)]
    assert all(1 <= x <= n for x in reps)
    out, spans = bytearray(bytes.fromhex("37A430EC") + struct.pack("<I", idv)), {}
    for name, piece in (("huf", d[0]), ("of", descs["of"]), ("ml", descs["ml"]), ("ll", descs["ll"]), ("rep", struct.pack("<3I", *reps))):
        spans[name] = (len(out), len(piece)); out += piece
    return bytes(out) + content, Dictionary(formatted=True, id=idv, content=content, content_offset=len(out), rep=tuple(reps), huf=huf, huf_form=d[1],
                                            tables=tables, norms=norms, spans=spans)


def generate(seed, xxh64=None, stats=False, **kw):
    """-> (frame bytes, decoded bytes, features) and, with stats=True, the facts of every block (module docstring).
    xxh64: the caller's hash function (this file has none) -- without one no frame gets a checksum"""
    g = FrameGen(seed, **kw)
    f, out, cks, feats = g.frame()
    if cks and xxh64 is not None:
        f += (xxh64(out) & 0xFFFFFFFF).to_bytes(4, "little")
    elif cks:
        f = f[:4] + bytes([f[4] & ~4]) + f[5:]
    feats = feats | ({"checksum"} if cks and xxh64 is not None else set())
    return (f, out, feats, g.facts) if stats else (f, out, feats)


def own_blocks(facts):
    """blocks whose modes byte has a table in RLE_Mode or FSE_Compressed_Mode (the two bits of its field differ): what the engine counts as
    a frame's n_own_tables"""
    return sum(1 for b in facts if b.get("modes") is not None and (b["modes"] ^ (b["modes"] >> 1)) & 0x54)

// zk_enc_dict_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// The host side of encoding against a dictionary (zeekstd_amd/csrc/zk_enc_dict.h, the very header the engine and the kernels include) on the
// CPU: the Huffman code and the FSE compression tables a zk_cdict is made of, against the DECODER's lane code for the same descriptions
// (zk_huf_read_weights / zk_huf_fill_table, zk_fse_read_ncount / zk_fse_build), and the selection rules (zke_dict_choose, zke_dict_pick,
// zke_sym_cost, zke_dict_id_width, zke_treeless_size).  tests/test_enc_dict_rules.py drives it; tests/sim/enc_dict_san.cpp runs the same
// entry points under AddressSanitizer + UBSan.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../zeekstd_amd/csrc/zk_enc_dict.h"

// LSB-first forward bit writer / backward reader over a plain bit vector
struct ZkdBits {
    std::vector<uint8_t> b;
    void put(uint32_t v, uint32_t n) { for (uint32_t i = 0; i < n; i++) b.push_back((v >> i) & 1); }
    size_t at = 0;
    void rewind() { at = b.size(); }
    bool take(uint32_t n, uint32_t *v) { if (at < n) return false; uint32_t x = 0; for (uint32_t i = 0; i < n; i++) x = (x << 1) | b[--at]; *v = x; return true; }
};

extern "C" {
uint32_t zk_enc_dict_sim_id_width(uint32_t id) { return zke_dict_id_width(id) | zke_dict_id_flag(zke_dict_id_width(id)) << 8; }
uint32_t zk_enc_dict_sim_sym_cost(int norm, int al) { return zke_sym_cost(norm, al); }
int zk_enc_dict_sim_pick(uint64_t c_predef, int own_ok, uint64_t c_own, int dict_ok, uint64_t c_dict) { return zke_dict_pick(c_predef, own_ok != 0, c_own, dict_ok != 0, c_dict); }
uint32_t zk_enc_dict_sim_treeless_size(uint32_t nlit, const uint64_t *bits, uint32_t *z, uint8_t *head5)
{
    const uint32_t sz = zke_treeless_size(nlit, bits, z);
    if (sz) zke_treeless_header(head5, nlit, sz - (nlit < 1024 ? 3 : nlit < 16384 ? 4 : 5));
    return sz;
}

// The dictionary's tables as zk_cdict_create builds them.  Returns 0, or the negated error of zk_dict_parse / zke_dict_build; -1: raw content.
// len_out[256], code_out[256]: the Huffman code; cost_out[3 * 64]: per-symbol costs LL, OF, ML; al_out[3]
int zk_enc_dict_sim_build(const uint8_t *d, size_t n, uint8_t *len_out, uint16_t *code_out, uint32_t *cost_out, uint32_t *al_out, uint32_t *maxbits_out)
{
    ZkDictLayout L;
    const uint32_t r = zk_dict_parse(d, n, L);
    if (r) return -(int)r;
    if (!L.formatted) return -1;
    ZkEncTables predef; zk_build_enc_tables(&predef);
    std::vector<ZkEncDictDev> dev(1);
    const uint32_t r2 = zke_dict_build(d, L, predef, &dev[0]);
    if (r2) return -(int)r2;
    memcpy(len_out, dev[0].huf_len, 256); memcpy(code_out, dev[0].huf_code, 512);
    memcpy(cost_out, dev[0].cost, sizeof dev[0].cost);
    for (int t = 0; t < 3; t++) al_out[t] = dev[0].T.al[t];
    *maxbits_out = dev[0].huf_maxbits;
    return 0;
}

// What the DECODER derives from the same tree description: weights[256] (0 = absent), *n symbols, *maxbits.  0 or -1.
int zk_enc_dict_sim_huf_weights(const uint8_t *d, size_t n, uint8_t *weights, uint32_t *nsym, uint32_t *maxbits)
{
    ZkDictLayout L;
    if (zk_dict_parse(d, n, L) || !L.formatted) return -1;
    ZkHufHdr hd; ZkHufTmp tmp;
    memset(&hd, 0, sizeof hd);
    if (!zk_huf_read_weights(d + L.huf_off, L.huf_len, &hd, &tmp, nsym, maxbits)) return -1;
    memset(weights, 0, 256);
    memcpy(weights, hd.weights, *nsym);
    return 0;
}

// lits[n] (every byte has a weight) written with the dictionary's code as zk_k_enc_dict_lits writes a stream -- last literal first, LSB first,
// end mark -- and read back through the decoder's table (zk_huf_fill_table) from the stream's end.  0: the literals came back; 1: they did
// not; -1: setup failed; -2: a literal without a weight.
int zk_enc_dict_sim_huf_roundtrip(const uint8_t *d, size_t n, const uint8_t *lits, uint32_t nl)
{
    ZkDictLayout L;
    if (zk_dict_parse(d, n, L) || !L.formatted) return -1;
    std::vector<uint8_t> len(256); std::vector<uint16_t> code(256);
    uint32_t mb = 0;
    if (zke_dict_huf_code(d + L.huf_off, L.huf_len, len.data(), code.data(), &mb)) return -1;
    ZkHufHdr hd; ZkHufTmp tmp; uint32_t ns = 0, mb2 = 0;
    if (!zk_huf_read_weights(d + L.huf_off, L.huf_len, &hd, &tmp, &ns, &mb2) || mb2 != mb) return -1;
    std::vector<uint16_t> table((size_t)1 << mb);
    zk_huf_fill_table(table.data(), &hd, ns, mb);
    ZkdBits b;
    for (uint32_t i = nl; i-- > 0;) { if (!len[lits[i]]) return -2; b.put(code[lits[i]], len[lits[i]]); }
    b.rewind();
    for (uint32_t i = 0; i < nl; i++) {
        // the decoder looks at maxbits bits from the top (zeros below the stream's first bit)
        uint32_t idx = 0;
        for (uint32_t k = 0; k < mb; k++) idx = (idx << 1) | (b.at > k ? b.b[b.at - 1 - k] : 0);
        const uint16_t cell = table[idx];
        if ((cell & 0xFF) != lits[i]) return 1;
        const uint32_t nb = cell >> 8;
        if (b.at < nb) return 1;
        b.at -= nb;
    }
    return b.at == 0 ? 0 : 1;
}

// syms[n] (codes of table t = ZK_TAB_LL / _OF / _ML that the dictionary's table gives a probability) through the compression table a zk_cdict
// holds -- the state walk of zk_k_enc_entropy's chain wave: zke_cinit, then per symbol the state's low bits and the next state, the final
// state's accuracy-log bits last -- and back through the lane code's decoder table for the same description.  0 / 1 / -1 / -2 as above.
int zk_enc_dict_sim_fse_roundtrip(const uint8_t *d, size_t n, int t, const uint8_t *syms, uint32_t ns)
{
    ZkDictLayout L;
    if (zk_dict_parse(d, n, L) || !L.formatted || !ns) return -1;
    const uint32_t off = t == ZK_TAB_LL ? L.ll_off : t == ZK_TAB_OF ? L.of_off : L.ml_off, ln = t == ZK_TAB_LL ? L.ll_len : t == ZK_TAB_OF ? L.of_len : L.ml_len;
    std::vector<ZkEncTables> T(1);
    memset(&T[0], 0, sizeof T[0]);
    uint32_t cost[64];
    if (zke_dict_fse_table(d + off, ln, t, &T[0], cost)) return -1;
    const uint16_t *st = t == ZK_TAB_LL ? T[0].ll_state : t == ZK_TAB_OF ? T[0].of_state : T[0].ml_state;
    const uint32_t *dfs = t == ZK_TAB_LL ? T[0].ll_dfs : t == ZK_TAB_OF ? T[0].of_dfs : T[0].ml_dfs;
    const uint32_t *dnb = t == ZK_TAB_LL ? T[0].ll_dnb : t == ZK_TAB_OF ? T[0].of_dnb : T[0].ml_dnb;
    const uint32_t al = T[0].al[t];
    for (uint32_t i = 0; i < ns; i++) if (syms[i] >= 64 || cost[syms[i]] == ZKE_COST_NONE) return -2;
    ZkdBits b;
    uint32_t s = zke_cinit(st, dnb[syms[ns - 1]], dfs[syms[ns - 1]]);
    for (uint32_t i = ns - 1; i-- > 0;) {
        const uint32_t c = syms[i], nb = (s + dnb[c]) >> 16;
        b.put(s & ((1u << nb) - 1u), nb);
        s = st[(s >> nb) + dfs[c]];
    }
    b.put(s & ((1u << al) - 1u), al);
    // the decoder's table
    int16_t norm[64]; uint32_t nsym = 0, al2 = 0;
    if (!zk_fse_read_ncount(d + off, ln, zk_tab_maxsym(t), zk_tab_maxal(t), norm, &nsym, &al2) || al2 != al) return -1;
    std::vector<uint32_t> cells((size_t)1 << al); uint16_t next[64];
    if (!zk_fse_build<ZkCells32>(cells.data(), norm, nsym, al, next, nullptr)) return -1;
    b.rewind();
    uint32_t state = 0;
    if (!b.take(al, &state)) return 1;
    for (uint32_t i = 0; i < ns; i++) {
        const uint32_t c = cells[state];
        if (zk_cell_sym(c) != syms[i]) return 1;
        if (i + 1 == ns) break;
        uint32_t v = 0;
        if (!b.take(zk_cell_nb(c), &v)) return 1;
        state = zk_cell_base(c) + v;
    }
    return b.at == 0 ? 0 : 1;
}

// One table of one frame as the owning lane of zk_k_enc_fse_build_dict decides it (zke_dict_choose): hist[64] the frame's code counts,
// cost_dict[64] / dict_al the dictionary's table.  costs_out[3]: predefined, own, dictionary (~0: not legal).  Returns the pick.
int zk_enc_dict_sim_choose(const uint32_t *hist, int t, uint32_t nseq, uint32_t n_blocks, const uint32_t *cost_dict, uint32_t dict_al, uint64_t *costs_out,
                           uint32_t *dlen_out)
{
    uint32_t predef[3][64];
    zke_predef_costs(predef);
    int16_t norm[64]; uint8_t desc[ZKE_DESC_CAP];
    memset(norm, 0, sizeof norm);
    return zke_dict_choose(hist, t, nseq, n_blocks, ZKE_FSE_MIN_SEQ, predef[t], cost_dict, dict_al, norm, desc, dlen_out, costs_out);
}
}

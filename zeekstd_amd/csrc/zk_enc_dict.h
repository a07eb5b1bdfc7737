// zk_enc_dict.h -- encoding against a zstd dictionary (zk_cdict, zk_encode_frames_dict*): what is built once per dictionary on the host, and
// the rules a frame's tables are chosen by.  Everything here runs on the CPU too (tests/sim/zk_enc_dict_sim.cpp).
//
// A frame of the dictionary route is a frame of the prefix route with the dictionary's content as the prefix -- same staging, same match
// kernels, same sequences and literals -- whose header names the dictionary and whose entropy coding may lean on the dictionary's tables:
//   sequence tables   per frame and per table (LL / OF / ML) the cheapest of: predefined; the frame's own (under the conditions of the other
//                     routes: >= ZKE_FSE_MIN_SEQ sequences, two symbols, a description that fits); the dictionary's, which is Repeat_Mode in
//                     EVERY block of the frame that has sequences -- legal only when the table gives every code the frame uses a probability.
//                     Costs are estimates (zke_sym_cost: -log2 of the normalised probability in 1/256 bit, plus the description and the final
//                     state per block); ties keep the choice of the other routes, then predefined.
//   literals          the first block of a frame only: Treeless_Literals_Block under the dictionary's tree where that is smaller, in bytes
//                     actually produced, than what the block has (own tree, raw or RLE) -- legal only when every literal has a weight.
//                     Later blocks are coded as everywhere: a first block that keeps an own tree ends the dictionary's.
// The dictionary's three repeat offsets never enter: the matcher emits a repeat code only after a sequence of the same block.
#pragma once
#include <stdint.h>
#include <string.h>
#include "zk_device.h"
#include "zk_enc_device.h"
#include "zk_dict.h"

// ---------------------------------------------------------------- rules (host and device)
// bytes of the Dictionary_ID field: the smallest width that holds the ID; none for ID 0 (a raw-content dictionary)
ZK_HD uint32_t zke_dict_id_width(uint32_t id) { return id == 0 ? 0u : id < 256u ? 1u : id < 65536u ? 2u : 4u; }
// Frame_Header_Descriptor's Dictionary_ID_Flag for that width
ZK_HD uint32_t zke_dict_id_flag(uint32_t width) { return width == 4 ? 3u : width; }

constexpr uint32_t ZKE_COST_NONE = 0xFFFFFFFFu;          // the table gives the symbol no probability
// -log2(norm / 2^al) in 1/256 bit (norm -1 = "less than one": probability 1 / 2^al); ZKE_COST_NONE for norm 0.
// log2 by eight squarings of the mantissa: integers only, so that host, device and the tests' restatement agree to the bit.
ZK_HD uint32_t zke_sym_cost(int norm, int al)
{
    if (norm == 0) return ZKE_COST_NONE;
    const uint32_t p = norm < 0 ? 1u : (uint32_t)norm;
    const uint32_t hb = zk_highbit(p);
    uint64_t x = (uint64_t)p << (16 - hb);                // [1, 2) in 16.16 (p <= 512)
    uint32_t frac = 0;
    for (int i = 7; i >= 0; i--) {
        x = (x * x) >> 16;
        if (x >= (2u << 16)) { frac |= 1u << i; x >>= 1; }
    }
    return ((uint32_t)al << 8) - ((hb << 8) | frac);
}
// cost of coding a frame's codes (hist[nsym]) with a table of per-symbol costs, in 1/256 bit; false: the table lacks a code that occurs
ZK_HD bool zke_table_cost(const uint32_t *hist, int nsym, const uint32_t *cost, uint64_t *out)
{
    uint64_t c = 0;
    for (int s = 0; s < nsym; s++) {
        if (!hist[s]) continue;
        if (cost[s] == ZKE_COST_NONE) return false;
        c += (uint64_t)hist[s] * cost[s];
    }
    *out = c;
    return true;
}
// what a table adds besides the symbols: its description once (own tables) and its accuracy log per block (the final state)
ZK_HD uint64_t zke_table_overhead(uint32_t desc_bytes, uint32_t al, uint32_t n_blocks) { return ((uint64_t)desc_bytes * 8 + (uint64_t)al * n_blocks) << 8; }

enum { ZKE_PICK_PREDEF = 0, ZKE_PICK_OWN = 1, ZKE_PICK_DICT = 2 };
// The cheapest of the legal choices.  The predefined table is always legal (the matcher produces no code it lacks); own_ok / dict_ok say
// whether the other two are.  Ties: the choice of the other routes (own where own_ok, else predefined), then predefined, then the dictionary's.
ZK_HD int zke_dict_pick(uint64_t c_predef, bool own_ok, uint64_t c_own, bool dict_ok, uint64_t c_dict)
{
    int pick = own_ok ? ZKE_PICK_OWN : ZKE_PICK_PREDEF;
    uint64_t best = own_ok ? c_own : c_predef;
    if (own_ok && c_predef < best) { pick = ZKE_PICK_PREDEF; best = c_predef; }
    if (dict_ok && c_dict < best) pick = ZKE_PICK_DICT;
    return pick;
}

// One table of one frame, as the lane of zk_k_enc_fse_build_dict that owns it decides: hist = the frame's code counts of table t, nseq > 0 its
// sequences, n_blocks its blocks.  The frame's own table is normalised and described (norm[64], desc[ZKE_DESC_CAP], *dlen) under the other
// routes' conditions whether or not it is picked; the caller builds it when ZKE_PICK_OWN comes back.  costs[3] (optional): predefined, own,
// dictionary -- ~0 where the choice is not legal.
// zke_dict_choose_sums takes the symbols' cost under the predefined and the dictionary's table as sums (zke_table_cost; the kernel adds them
// up with a lane per code), zke_dict_choose makes them itself.
ZK_HD int zke_dict_choose_sums(const uint32_t *hist, int t, uint32_t nseq, uint32_t n_blocks, uint32_t min_seq, uint64_t c_predef, bool dict_ok,
                               uint64_t c_dict, uint32_t dict_al, int16_t *norm, uint8_t *desc, uint32_t *dlen, uint64_t *costs)
{
    const int nsym = t == 0 ? 36 : t == 1 ? 32 : 53, L = zke_fse_log(t, nseq);
    bool own_ok = false;
    uint64_t c_own = 0;
    *dlen = 0;
    if (nseq >= min_seq && zke_fse_normalize(hist, nsym, L, norm)) {
        int last = nsym;
        while (last > 0 && norm[last - 1] == 0) last--;
        const uint32_t d = zke_fse_write_ncount(desc, ZKE_DESC_CAP, norm, last, L);
        if (d) {
            own_ok = true; *dlen = d;
            for (int s = 0; s < nsym; s++) if (hist[s]) c_own += (uint64_t)hist[s] * zke_sym_cost(norm[s], L);
            c_own += zke_table_overhead(d, (uint32_t)L, n_blocks);
        }
    }
    c_predef += zke_table_overhead(0, t == 1 ? 5u : 6u, n_blocks);
    c_dict += zke_table_overhead(0, dict_al, n_blocks);
    if (costs) { costs[0] = c_predef; costs[1] = own_ok ? c_own : ~0ull; costs[2] = dict_ok ? c_dict : ~0ull; }
    return zke_dict_pick(c_predef, own_ok, c_own, dict_ok, c_dict);
}
ZK_HD int zke_dict_choose(const uint32_t *hist, int t, uint32_t nseq, uint32_t n_blocks, uint32_t min_seq, const uint32_t *cost_predef,
                          const uint32_t *cost_dict, uint32_t dict_al, int16_t *norm, uint8_t *desc, uint32_t *dlen, uint64_t *costs)
{
    const int nsym = t == 0 ? 36 : t == 1 ? 32 : 53;
    uint64_t c_predef = 0, c_dict = 0;
    (void)zke_table_cost(hist, nsym, cost_predef, &c_predef);       // (always legal: the matcher produces no code the predefined tables lack)
    const bool dict_ok = zke_table_cost(hist, nsym, cost_dict, &c_dict);
    return zke_dict_choose_sums(hist, t, nseq, n_blocks, min_seq, c_predef, dict_ok, c_dict, dict_al, norm, desc, dlen, costs);
}

// The literals section of a first block under the dictionary's tree: one stream below 256 literals, four above (libzstd's rule).
// bits[k]: the sum of the code lengths of stream k's literals.  Returns the section's bytes (header, jump table, streams) and the streams'
// sizes in z[]; 0: the format has no header for it (a stream of 64 KiB, a section beyond its size field).
ZK_HD uint32_t zke_treeless_size(uint32_t nlit, const uint64_t bits[4], uint32_t z[4])
{
    const bool single = nlit < 256;
    uint64_t comp = single ? 0 : 6;
    for (int k = 0; k < 4; k++) {
        const uint64_t b = single && k ? 0 : (bits[k] + 1 + 7) >> 3;       // + the end mark
        if (b >= 65536) return 0;
        z[k] = (uint32_t)b; comp += b;
    }
    const uint32_t hdr = nlit < 1024 ? 3 : nlit < 16384 ? 4 : 5, lim = hdr == 3 ? 1024u : hdr == 4 ? 16384u : 262144u;
    if (comp >= lim) return 0;
    return hdr + (uint32_t)comp;
}
// its header: Treeless (3), Size_Format 0 = one stream, 1 / 2 / 3 = four streams with 10 / 14 / 18-bit sizes
ZK_HD uint32_t zke_treeless_header(uint8_t *head, uint32_t nlit, uint32_t comp)
{
    const uint32_t hdr = nlit < 1024 ? 3 : nlit < 16384 ? 4 : 5;
    const uint64_t sf = nlit < 256 ? 0 : hdr == 3 ? 1 : hdr == 4 ? 2 : 3;
    const uint32_t sh = hdr == 3 ? 14 : hdr == 4 ? 18 : 22;
    const uint64_t h = 3ull | (sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)comp << sh);
    for (uint32_t i = 0; i < hdr; i++) head[i] = (uint8_t)(h >> (8 * i));
    return hdr;
}

// ---------------------------------------------------------------- the dictionary's tables as the kernels read them (one per zk_cdict, in HBM)
struct ZkEncDictDev {
    ZkEncTables T;                       // the three FSE compression tables (state / dfs / dnb / al); custom, dlen and desc stay 0
    uint32_t cost[3][64];                // zke_sym_cost per code under the dictionary's tables (LL, OF, ML)
    uint32_t cost_predef[3][64];         // ... under the predefined ones
    uint8_t huf_len[256];                // the dictionary's Huffman code: length 0 = the byte has no weight
    uint16_t huf_code[256];
    uint32_t huf_maxbits;
    uint32_t id, id_width;
};
// what the dictionary variants of zk_k_enc_sizes / zk_k_enc_assemble need of it
struct ZkEncDictId { uint32_t id, width; };

// ---------------------------------------------------------------- built once per dictionary (host)
// code lengths and canonical codes from the tree description's weights, assigned as the decoder's table fill assigns them
// (zk_huf_fill_table: weight 1 first, symbols ascending): code = table index >> (weight - 1).  0, or ZK_E_DICT_CORRUPTED.
static inline uint32_t zke_dict_huf_code(const uint8_t *desc, uint32_t len, uint8_t *huf_len, uint16_t *huf_code, uint32_t *maxbits_out)
{
    ZkHufHdr hd; ZkHufTmp tmp;
    uint32_t n = 0, mb = 0;
    if (!zk_huf_read_weights(desc, len, &hd, &tmp, &n, &mb)) return ZK_E_DICT_CORRUPTED;
    memset(huf_len, 0, 256); memset(huf_code, 0, 512);
    uint32_t pos = 0;
    for (uint32_t wt = 1; wt <= mb; wt++)
        for (uint32_t s = 0; s < n; s++)
            if (hd.weights[s] == wt) { huf_len[s] = (uint8_t)(mb + 1 - wt); huf_code[s] = (uint16_t)(pos >> (wt - 1)); pos += 1u << (wt - 1); }
    *maxbits_out = mb;
    return ZK_OK;
}

// one FSE compression table of the set from its description; norm_out[64] / nsym_out / al_out for the tests
static inline uint32_t zke_dict_fse_table(const uint8_t *desc, uint32_t len, int t, ZkEncTables *T, uint32_t *cost, int16_t *norm_out = nullptr,
                                          uint32_t *nsym_out = nullptr)
{
    int16_t norm[64];
    uint32_t nsym = 0, al = 0;
    if (!zk_fse_read_ncount(desc, len, zk_tab_maxsym(t), zk_tab_maxal(t), norm, &nsym, &al)) return ZK_E_DICT_CORRUPTED;
    uint8_t sym[512]; int32_t cumul[66];
    uint16_t *st = t == ZK_TAB_LL ? T->ll_state : t == ZK_TAB_OF ? T->of_state : T->ml_state;
    uint32_t *dfs = t == ZK_TAB_LL ? T->ll_dfs : t == ZK_TAB_OF ? T->of_dfs : T->ml_dfs;
    uint32_t *dnb = t == ZK_TAB_LL ? T->ll_dnb : t == ZK_TAB_OF ? T->of_dnb : T->ml_dnb;
    zke_build_ctable(norm, (int)nsym, (int)al, st, dfs, dnb, sym, cumul);
    T->al[t] = al;
    for (uint32_t s = 0; s < 64; s++) cost[s] = s < nsym ? zke_sym_cost(norm[s], (int)al) : ZKE_COST_NONE;
    if (norm_out) { memset(norm_out, 0, 64 * sizeof(int16_t)); memcpy(norm_out, norm, nsym * sizeof(int16_t)); }
    if (nsym_out) *nsym_out = nsym;
    return ZK_OK;
}

static inline void zke_predef_costs(uint32_t cost[3][64])
{
    static const int16_t ll[36] = ZK_LL_DEFNORM, of[29] = ZK_OF_DEFNORM, ml[53] = ZK_ML_DEFNORM;
    for (int s = 0; s < 64; s++) {
        cost[ZK_TAB_LL][s] = s < 36 ? zke_sym_cost(ll[s], 6) : ZKE_COST_NONE;
        cost[ZK_TAB_OF][s] = s < 29 ? zke_sym_cost(of[s], 5) : ZKE_COST_NONE;
        cost[ZK_TAB_ML][s] = s < 53 ? zke_sym_cost(ml[s], 6) : ZKE_COST_NONE;
    }
}

// The predefined FSE compression tables (host, once per engine): what every frame starts from, and what zke_dict_build takes its value tables from.
static inline void zk_build_enc_tables(ZkEncTables *t)
{
    static const int16_t ll[36] = ZK_LL_DEFNORM, of[29] = ZK_OF_DEFNORM, ml[53] = ZK_ML_DEFNORM;
    static const uint32_t llv[36] = ZK_LL_TABLE, mlv[53] = ZK_ML_TABLE;
    memset(t, 0, sizeof *t);
    uint8_t sym[512]; int32_t cumul[66];
    zke_build_ctable(ll, 36, 6, t->ll_state, t->ll_dfs, t->ll_dnb, sym, cumul);
    zke_build_ctable(of, 29, 5, t->of_state, t->of_dfs, t->of_dnb, sym, cumul);
    zke_build_ctable(ml, 53, 6, t->ml_state, t->ml_dfs, t->ml_dnb, sym, cumul);
    for (int i = 0; i < 36; i++) t->ll_val[i] = llv[i];
    for (int i = 0; i < 53; i++) t->ml_val[i] = mlv[i];
    t->al[0] = 6; t->al[1] = 5; t->al[2] = 6;
}

// The compression side of a formatted dictionary's four tables.  `predef` supplies the value tables (ll_val / ml_val), which are the same
// in every set.  0, or ZK_E_DICT_CORRUPTED (what zk_dict_create refuses too).
static inline uint32_t zke_dict_build(const uint8_t *d, const ZkDictLayout &L, const ZkEncTables &predef, ZkEncDictDev *out)
{
    memset(out, 0, sizeof *out);
    out->T = predef;
    out->T.custom = 0; memset(out->T.dlen, 0, sizeof out->T.dlen); memset(out->T.desc, 0, sizeof out->T.desc);
    uint32_t r;
    if ((r = zke_dict_huf_code(d + L.huf_off, L.huf_len, out->huf_len, out->huf_code, &out->huf_maxbits))) return r;
    if ((r = zke_dict_fse_table(d + L.ll_off, L.ll_len, ZK_TAB_LL, &out->T, out->cost[ZK_TAB_LL]))) return r;
    if ((r = zke_dict_fse_table(d + L.of_off, L.of_len, ZK_TAB_OF, &out->T, out->cost[ZK_TAB_OF]))) return r;
    if ((r = zke_dict_fse_table(d + L.ml_off, L.ml_len, ZK_TAB_ML, &out->T, out->cost[ZK_TAB_ML]))) return r;
    zke_predef_costs(out->cost_predef);
    out->id = L.id; out->id_width = zke_dict_id_width(L.id);
    return ZK_OK;
}

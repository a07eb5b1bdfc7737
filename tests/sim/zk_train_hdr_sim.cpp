// zk_train_hdr_sim.cpp -- TEST HARNESS (never shipped): the host writer of a trained dictionary's header (zeekstd_amd/csrc/zk_train_host.h)
// as a function tests/test_train_header.py calls, and the header read back with the DECODER's own parsers (zk_dict_parse of zk_dict.h over
// zk_huf_read_weights / zk_fse_read_ncount, which share nothing with the writer).
#include "../../zeekstd_amd/csrc/zk_train_host.h"
#include "../../zeekstd_amd/csrc/zk_dict.h"

extern "C" uint64_t zk_train_hdr_sim_write(const uint64_t *lit, const uint64_t *ll, const uint64_t *ml, const uint64_t *of, uint32_t dict_id, uint8_t *dst, uint64_t cap, int *rebuilds, uint32_t desc_limit)
{
    return zkt_write_header(lit, ll, ml, of, dict_id, dst, (size_t)cap, rebuilds, desc_limit);
}
extern "C" uint64_t zk_train_hdr_sim_xxh64(const uint8_t *p, uint64_t len) { return zkt_xxh64(p, (size_t)len); }
extern "C" uint32_t zk_train_hdr_sim_id(const uint8_t *p, uint64_t len) { return zkt_dict_id(p, (size_t)len); }
// d[0, len): a whole dictionary.  weights[256], maxbits; norm[3][64] in the order LL, OF, ML with nsym[3], al[3]; reps[3]; *content_off.
// Returns 0, or the decoder's error code.
extern "C" int zk_train_hdr_sim_parse(const uint8_t *d, uint64_t len, uint8_t *weights, uint32_t *maxbits, int16_t *norm, uint32_t *nsym, uint32_t *al,
                                      uint32_t *reps, uint32_t *id, uint64_t *content_off)
{
    ZkDictLayout L;
    const uint32_t r = zk_dict_parse(d, (size_t)len, L);
    if (r || !L.formatted) return r ? (int)r : -1;
    ZkHufHdr hd; ZkHufTmp tmp;
    uint32_t n = 0;
    if (!zk_huf_read_weights(d + L.huf_off, L.huf_len, &hd, &tmp, &n, maxbits)) return -2;
    memset(weights, 0, 256);
    memcpy(weights, hd.weights, n);
    const uint32_t offs[3] = {L.ll_off, L.of_off, L.ml_off}, lens[3] = {L.ll_len, L.of_len, L.ml_len};
    const int tabs[3] = {ZK_TAB_LL, ZK_TAB_OF, ZK_TAB_ML};
    for (int t = 0; t < 3; t++) {
        memset(norm + 64 * t, 0, 64 * sizeof(int16_t));
        if (!zk_fse_read_ncount(d + offs[t], lens[t], zk_tab_maxsym(tabs[t]), zk_tab_maxal(tabs[t]), norm + 64 * t, &nsym[t], &al[t])) return -3;
    }
    for (int i = 0; i < 3; i++) reps[i] = L.rep[i];
    *id = L.id; *content_off = L.content_off;
    return 0;
}

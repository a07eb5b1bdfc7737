// zk_train_host.h -- the header of a trained dictionary (RFC 8878 section 5), written on the host from four histograms: plain C++, no GPU,
// included by zk_train.hip and by tests/sim/zk_train_hdr_sim.cpp.
//   magic | Dictionary_ID | Huffman tree description | FSE descriptions OF, ML, LL | repeat offsets 1, 4, 8          (the content follows)
// Rules:
//   coverage  every literal value and every code LL 0..35, ML 0..52, OF 0..30 gets a count of at least 1 (counts are first scaled below
//             2^24), so that the engine's own rules always allow a Treeless first block and Repeat_Mode
//   FSE       the encoder's own normalisation and description writer (zke_fse_normalize / zke_fse_write_ncount) at logs 9 / 9 / 8 (LL / ML / OF)
//   Huffman   code lengths <= 11 over all 256 values; 255 weights exceed the direct form's 128, so they are written FSE-compressed (accuracy
//             log 6, two interleaved states, as HUF_compressWeights writes them).  A description above the form's 127 bytes: the counts are
//             flattened ((c + 1) / 2) and the tree built again (no histogram found reaches it -- 255 weights of <= 12 values hold <= 114
//             bytes -- so the limit is a parameter and the tests lower it).  One weight throughout (a uniform histogram) has no FSE form: the count of
//             value 0 is raised fourfold once (twofold still gives the full tree of depth 8).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <queue>
#include <vector>
#include "zk_enc_device.h"

constexpr uint32_t ZKT_DICT_MAGIC = 0xEC30A437u;

// XXH64, seed 0 (the public algorithm), for the Dictionary_ID of a content: 32768 + hash mod (2^31 - 65536), inside libzstd's private range
static inline uint64_t zkt_xxh64(const uint8_t *p, size_t len)
{
    const uint64_t P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P3 = 1609587929392839161ull, P4 = 9650029242287828579ull, P5 = 2870177450012600261ull;
    auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
    auto rd64 = [](const uint8_t *q) { uint64_t v; memcpy(&v, q, 8); return v; };
    auto rd32 = [](const uint8_t *q) { uint32_t v; memcpy(&v, q, 4); return (uint64_t)v; };
    auto round = [&](uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; };
    auto merge = [&](uint64_t h, uint64_t v) { return (h ^ round(0, v)) * P1 + P4; };
    const uint8_t *end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
        for (; p + 32 <= end; p += 32) { v1 = round(v1, rd64(p)); v2 = round(v2, rd64(p + 8)); v3 = round(v3, rd64(p + 16)); v4 = round(v4, rd64(p + 24)); }
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
        h = merge(h, v1); h = merge(h, v2); h = merge(h, v3); h = merge(h, v4);
    } else h = P5;
    h += (uint64_t)len;
    for (; p + 8 <= end; p += 8) h = rotl(h ^ round(0, rd64(p)), 27) * P1 + P4;
    if (p + 4 <= end) { h = rotl(h ^ (rd32(p) * P1), 23) * P2 + P3; p += 4; }
    for (; p < end; p++) h = rotl(h ^ (*p * P5), 11) * P1;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}
static inline uint32_t zkt_dict_id(const uint8_t *content, size_t len) { return 32768u + (uint32_t)(zkt_xxh64(content, len) % ((1ull << 31) - 65536ull)); }

// counts below 2^24 with the zeros made 1
static inline void zkt_cover(const uint64_t *in, int n, uint32_t *out)
{
    uint64_t mx = 0;
    for (int i = 0; i < n; i++) mx = in[i] > mx ? in[i] : mx;
    int sh = 0;
    while ((mx >> sh) >> 24) sh++;
    for (int i = 0; i < n; i++) { const uint64_t v = in[i] >> sh; out[i] = v ? (uint32_t)v : 1u; }
}
// Huffman code lengths of 256 present symbols, the deepest at most 11 (counts halved, rounding up, until the tree fits); returns the deepest
static inline int zkt_huf_lengths(const uint32_t *cnt_in, uint8_t *len)
{
    uint32_t cnt[256];
    memcpy(cnt, cnt_in, sizeof cnt);
    for (;;) {
        // (count, node) pairs: ties go to the lower node number, so the tree is a function of the counts
        typedef std::pair<uint64_t, int> P;
        std::priority_queue<P, std::vector<P>, std::greater<P>> q;
        int parent[511];
        for (int s = 0; s < 256; s++) q.push(P(cnt[s], s));
        int nn = 256;
        while (q.size() > 1) {
            const P a = q.top(); q.pop();
            const P b = q.top(); q.pop();
            parent[a.second] = parent[b.second] = nn;
            q.push(P(a.first + b.first, nn++));
        }
        int depth[511], mx = 0;
        depth[nn - 1] = 0;
        for (int i = nn - 2; i >= 0; i--) depth[i] = depth[parent[i]] + 1;
        for (int s = 0; s < 256; s++) mx = depth[s] > mx ? depth[s] : mx;
        if (mx <= 11) { for (int s = 0; s < 256; s++) len[s] = (uint8_t)depth[s]; return mx; }
        for (int s = 0; s < 256; s++) cnt[s] = (cnt[s] + 1) >> 1;
    }
}
// the FSE-compressed form of the weights w[0 .. n) (values 0 .. 12): NCount at log 6, then the two-state bitstream.  Returns its bytes; 0:
// one weight throughout, or no room
static inline uint32_t zkt_compress_weights(const uint8_t *w, uint32_t n, uint8_t *dst, uint32_t cap)
{
    constexpr int L = 6;
    uint32_t hist[13] = {0};
    int nsym = 0;
    for (uint32_t i = 0; i < n; i++) { hist[w[i]]++; nsym = w[i] + 1 > nsym ? w[i] + 1 : nsym; }
    int16_t norm[13];
    if (!zke_fse_normalize(hist, nsym, L, norm)) return 0;
    const uint32_t hb = zke_fse_write_ncount(dst, cap, norm, nsym, L);
    if (!hb) return 0;
    uint16_t state[1 << L]; uint32_t dfs[13], dnb[13]; uint8_t sym[1 << L]; int32_t cumul[15];
    zke_build_ctable(norm, nsym, L, state, dfs, dnb, sym, cumul);
    uint64_t acc = 0; uint32_t nb = 0, pos = hb; bool ovf = false;
    auto add = [&](uint32_t v, uint32_t bits) {
        acc |= (uint64_t)(v & ((1u << bits) - 1u)) << nb; nb += bits;
        while (nb >= 8) { if (pos < cap) dst[pos] = (uint8_t)acc; else ovf = true; pos++; acc >>= 8; nb -= 8; }
    };
    // symbol i belongs to state i & 1; the last symbols start the states, the first symbol is encoded last (decoded first)
    uint32_t st[2] = {0, 0}; bool started[2] = {false, false};
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t s = w[i], k = i & 1;
        if (!started[k]) { st[k] = zke_cinit(state, dnb[s], dfs[s]); started[k] = true; continue; }
        const uint32_t out = (st[k] + dnb[s]) >> 16;
        add(st[k], out);
        st[k] = state[(st[k] >> out) + dfs[s]];
    }
    add(st[1], L); add(st[0], L);
    add(1, 1);
    if (nb) add(0, 8 - nb);
    return ovf ? 0u : pos;
}
// The header's bytes into dst (cap >= 512 always suffices: 8 + 128 + 3 * 80 + 12); returns them, 0 on failure (never for cap >= 512).
// lit[256], ll[36], ml[53], of[32] (codes 31 of `of` is not used): what the matcher's literals and sequences count to; any values, zeros included.
static inline size_t zkt_write_header(const uint64_t *lit, const uint64_t *ll, const uint64_t *ml, const uint64_t *of, uint32_t dict_id, uint8_t *dst, size_t cap,
                                      int *rebuilds = nullptr,        // rebuilds: how often the tree was built again
                                      uint32_t desc_limit = 128)      // the tree description's FSE form must be SHORTER than this (the format: 128)
{
    if (cap < 8) return 0;
    size_t p = 0;
    auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; i++) dst[p++] = (uint8_t)(v >> (8 * i)); };
    put32(ZKT_DICT_MAGIC); put32(dict_id);
    // the tree description
    uint32_t cnt[256];
    zkt_cover(lit, 256, cnt);
    bool raised = false;
    for (int attempt = 0;; attempt++) {
        if (attempt > 64) return 0;
        if (rebuilds) *rebuilds = attempt;
        uint8_t len[256], w[256];
        const int mx = zkt_huf_lengths(cnt, len);
        for (int s = 0; s < 256; s++) w[s] = (uint8_t)(mx + 1 - len[s]);
        uint8_t body[160];
        const uint32_t n = zkt_compress_weights(w, 255, body, sizeof body);        // (the last value's weight is implied)
        if (n && n < desc_limit) {
            if (cap - p < 1 + n) return 0;
            dst[p++] = (uint8_t)n;
            memcpy(dst + p, body, n); p += n;
            break;
        }
        bool one = true;
        for (int s = 1; s < 255; s++) one = one && w[s] == w[0];
        if (one && !raised) { cnt[0] = 4 * cnt[0]; raised = true; }
        else for (int s = 0; s < 256; s++) cnt[s] = (cnt[s] + 1) >> 1;
    }
    // OF, ML, LL
    const struct { const uint64_t *h; int nsym, log; } tabs[3] = {{of, 31, 8}, {ml, 53, 9}, {ll, 36, 9}};
    for (const auto &t : tabs) {
        uint32_t c[64]; int16_t norm[64];
        zkt_cover(t.h, t.nsym, c);
        if (!zke_fse_normalize(c, t.nsym, t.log, norm)) return 0;
        const uint32_t n = zke_fse_write_ncount(dst + p, (uint32_t)(cap - p < 1024 ? cap - p : 1024), norm, t.nsym, t.log);
        if (!n) return 0;
        p += n;
    }
    if (cap - p < 12) return 0;
    put32(1); put32(4); put32(8);
    return p;
}

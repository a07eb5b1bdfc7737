// The host side of encoding against a dictionary (zk_enc_dict.h through tests/sim/zk_enc_dict_sim.cpp) built with AddressSanitizer + UBSan, a
// program of its own: every entry point of the simulation library once over a dictionary file -- the tables zk_cdict_create builds, the
// Huffman and FSE round trips through the decoder's lane code over seeded legal strings, and the per-table choice over seeded histograms.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/enc_dict_san.cpp -o /tmp/dictsan
//   /tmp/dictsan <dictionary file> <seed>
// Exit 0: every round trip returned its input (a raw-content dictionary has nothing to build: 0 as well).
#include "zk_enc_dict_sim.cpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + k);
    fclose(f);
    uint64_t s = strtoull(argv[2], nullptr, 10) * 2862933555777941757ull + 3037000493ull;
    auto rnd = [&](uint32_t n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((s >> 33) % n); };
    std::vector<uint8_t> len(256); std::vector<uint16_t> code(256); std::vector<uint32_t> cost(3 * 64);
    uint32_t al[3], mb = 0;
    const int rc = zk_enc_dict_sim_build(d.data(), d.size(), len.data(), code.data(), cost.data(), al, &mb);
    if (rc == -1) { printf("raw content\n"); return 0; }
    if (rc) return 1;
    std::vector<uint8_t> w(256); uint32_t ns = 0, mb2 = 0;
    if (zk_enc_dict_sim_huf_weights(d.data(), d.size(), w.data(), &ns, &mb2) || mb2 != mb) return 1;
    std::vector<uint8_t> alphabet;
    for (int b = 0; b < 256; b++) if (len[b]) alphabet.push_back((uint8_t)b);
    int bad = 0;
    for (uint32_t n : {1u, 2u, 255u, 256u, 4097u}) {
        std::vector<uint8_t> lits(n);
        for (auto &x : lits) x = alphabet[rnd((uint32_t)alphabet.size())];
        bad += zk_enc_dict_sim_huf_roundtrip(d.data(), d.size(), lits.data(), n) != 0;
    }
    for (int t = 0; t < 3; t++) {
        std::vector<uint8_t> legal;
        for (int c = 0; c < 64; c++) if (cost[64 * t + c] != ZKE_COST_NONE) legal.push_back((uint8_t)c);
        for (uint32_t n : {1u, 2u, 300u, 5000u}) {
            std::vector<uint8_t> syms(n);
            for (auto &x : syms) x = legal[rnd((uint32_t)legal.size())];
            bad += zk_enc_dict_sim_fse_roundtrip(d.data(), d.size(), t, syms.data(), n) != 0;
        }
        for (uint32_t nseq : {1u, 255u, 256u, 20000u}) {
            uint32_t hist[64] = {0};
            const int nsym = t == 0 ? 36 : t == 1 ? 32 : 53;
            for (uint32_t i = 0; i < nseq; i++) hist[rnd(1 + rnd((uint32_t)nsym))]++;
            uint64_t costs[3]; uint32_t dlen = 0;
            const int p = zk_enc_dict_sim_choose(hist, t, nseq, 1 + rnd(8), &cost[64 * t], al[t], costs, &dlen);
            bad += p < 0 || p > 2 || costs[p] == ~0ull;
        }
    }
    uint64_t bits[4] = {rnd(4000), rnd(4000), rnd(4000), rnd(4000)}; uint32_t z[4]; uint8_t head[5];
    (void)zk_enc_dict_sim_treeless_size(1000, bits, z, head);
    printf("%zu bytes, tree depth %u, %zu literals with a weight: %d failures\n", d.size(), mb, alphabet.size(), bad);
    return bad ? 1 : 0;
}

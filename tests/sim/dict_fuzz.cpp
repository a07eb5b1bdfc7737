// The decode lane code with a dictionary (zk_device.h and zk_dict.h, through tests/sim/zk_sim_dict.cpp) under AddressSanitizer + UBSan.
// Every buffer handed over is a heap allocation of exactly the size stated: compressed bytes (no padding: the harness makes its own copy
// with the padding the engine promises), the dictionary, the output.  A lane that follows a damaged header, table, offset or dictionary
// out of its buffers is a sanitizer report, where on the device it would be a silent read or a fault.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/dict_fuzz.cpp -o /tmp/dictfuzz
//   /tmp/dictfuzz <case file> <dictionary file> <iterations> <seed>
// case file (written by tests/test_generated_dict.py): u32 nframes, u64 comp_len, u64 out_len, (u64 c, u64 d) x nframes, comp.
// Round 0 decodes the case's bytes AS THEY ARE (the test hands over frames it damaged itself, the ones the kernels see later) and prints
// the statuses, one line; every further round damages a fresh copy some more -- every fourth one the dictionary too.
// Exit 0: no round left its buffers.
#include "zk_sim_dict.cpp"
#include <cstdio>
#include <cstdlib>

static uint64_t f_s;
static uint64_t f_rnd() { f_s ^= f_s << 13; f_s ^= f_s >> 7; f_s ^= f_s << 17; return f_s; }

static bool slurp(const char *path, std::vector<uint8_t> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) v.insert(v.end(), tmp, tmp + k);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> dict;
    if (!slurp(argv[2], dict)) return 2;
    const uint64_t iters = strtoull(argv[3], nullptr, 10);
    f_s = strtoull(argv[4], nullptr, 10) * 0x9E3779B97F4A7C15ull + 7;
    uint32_t nf; uint64_t clen, olen;
    if (fread(&nf, 4, 1, f) != 1 || fread(&clen, 8, 1, f) != 1 || fread(&olen, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> c_off(nf + 1, 0), d_off(nf + 1, 0);
    for (uint32_t i = 0; i < nf; i++) {
        uint64_t cd[2];
        if (fread(cd, 8, 2, f) != 2) return 2;
        c_off[i + 1] = c_off[i] + cd[0]; d_off[i + 1] = d_off[i] + cd[1];
    }
    std::vector<uint8_t> comp(clen);
    if (clen && fread(comp.data(), 1, clen, f) != clen) return 2;
    fclose(f);
    uint64_t flagged = 0;
    for (uint64_t it = 0; it <= iters; it++) {
        uint8_t *in = (uint8_t *)malloc(clen ? clen : 1), *out = (uint8_t *)malloc(olen + 1), *dc = (uint8_t *)malloc(dict.size() ? dict.size() : 1);
        int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (nf ? nf : 1));
        memcpy(in, comp.data(), clen); memcpy(dc, dict.data(), dict.size()); memset(out, 0xEE, olen + 1);
        uint64_t dlen = dict.size();
        if (it && clen) {
            const int k = 1 + (int)(f_rnd() % 6);
            for (int j = 0; j < k; j++) in[f_rnd() % clen] ^= (uint8_t)(1u << (f_rnd() % 8));
            if (f_rnd() % 5 == 0) { const uint64_t a = f_rnd() % clen, n = 1 + f_rnd() % 16; for (uint64_t q = a; q < clen && q < a + n; q++) in[q] = (uint8_t)f_rnd(); }
        }
        if (it && it % 4 == 0 && dlen) {                    // the entropy section sits in the first few hundred bytes
            const uint64_t span = dlen < 400 ? dlen : 400;
            dc[f_rnd() % span] ^= (uint8_t)(1u << (f_rnd() % 8));
            if (f_rnd() % 4 == 0) dlen = f_rnd() % (dlen + 1);
        }
        const int rc = zk_sim_dict_decode(in, clen, c_off.data(), d_off.data(), nf, dlen ? dc : nullptr, dlen, out, st);
        if (out[olen] != 0xEE) { fprintf(stderr, "a byte behind the output was written\n"); return 4; }
        if (!it) {
            if (rc != 0) { fprintf(stderr, "the dictionary does not load\n"); return 3; }
            printf("statuses");
            for (uint32_t i = 0; i < nf; i++) printf(" %d", st[i]);
            printf("\n");
        }
        bool any = rc != 0;
        for (uint32_t i = 0; i < nf && !any; i++) any = st[i] != 0;
        flagged += any;
        free(in); free(out); free(dc); free(st);
    }
    printf("%llu damaged inputs, %llu flagged\n", (unsigned long long)iters, (unsigned long long)flagged);
    return 0;
}

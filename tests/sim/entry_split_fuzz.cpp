// zk_split_entry (zeekstd_amd/csrc/zk_refine.h), the entry walk of zk_refine_entries, under AddressSanitizer + UBSan on mutated and
// truncated entries.  Every entry is a heap allocation of exactly its bytes + ZK_COMP_PADDING: a hop that follows a damaged size field out of
// the entry is a sanitizer report, where on the device it would be a silent read or a fault.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/entry_split_fuzz.cpp -o /tmp/splitfuzz
//   /tmp/splitfuzz <case file> <iterations> <seed>
// case file (written by tests/test_refine_entries.py): u32 entries, u64 comp_len, (u64 c_size) x entries, comp.
// Exit 0: the undamaged entries are whole frames, and on every input the count and the emit pass agree, every piece begins inside the
// entry, the pieces ascend by at least 3 bytes (so the walk ends) and nothing behind the `starts` array was written.
#include "../../zeekstd_amd/csrc/zk_refine.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t f_s;
static uint64_t f_rnd() { f_s ^= f_s << 13; f_s ^= f_s >> 7; f_s ^= f_s << 17; return f_s; }

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint64_t iters = strtoull(argv[2], nullptr, 10);
    f_s = strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 7;
    uint32_t ne; uint64_t clen;
    if (fread(&ne, 4, 1, f) != 1 || fread(&clen, 8, 1, f) != 1 || !ne) return 2;
    std::vector<uint64_t> c_off(ne + 1, 0);
    for (uint32_t i = 0; i < ne; i++) { uint64_t c; if (fread(&c, 8, 1, f) != 1) return 2; c_off[i + 1] = c_off[i] + c; }
    std::vector<uint8_t> comp(clen);
    if (c_off[ne] != clen || (clen && fread(comp.data(), 1, clen, f) != clen)) return 2;
    fclose(f);
    uint64_t stopped = 0;
    for (uint64_t it = 0; it < ne + iters; it++) {
        const uint32_t e = it < ne ? (uint32_t)it : (uint32_t)(f_rnd() % ne);
        uint64_t len = c_off[e + 1] - c_off[e];
        const bool mutate = it >= ne;
        if (mutate && len && f_rnd() % 3 == 0) len = f_rnd() % (len + 1);                  // truncated
        // the entry at a random place of its own buffer: [lead | entry | 8 bytes of padding], exact size
        const uint64_t lead = mutate ? f_rnd() % 5 : 0;
        uint8_t *in = (uint8_t *)malloc(lead + len + 8);
        memset(in, 0xAB, lead);
        memcpy(in + lead, comp.data() + c_off[e], len);
        memset(in + lead + len, 0, 8);
        if (mutate && len) {
            switch (f_rnd() % 5) {
            case 0: in[lead + f_rnd() % len] ^= (uint8_t)(1u << (f_rnd() % 8)); break;
            case 1: for (int k = 0; k < 3; k++) in[lead + f_rnd() % len] = (uint8_t)f_rnd(); break;
            case 2: { const uint64_t a = f_rnd() % len, n = 1 + f_rnd() % 16; for (uint64_t k = a; k < len && k < a + n; k++) in[lead + k] = (uint8_t)f_rnd(); break; }
            case 3: { const uint64_t a = f_rnd() % len; memset(in + lead + a, 0xFF, (size_t)((len - a) < 8 ? len - a : 8)); break; }   // (huge size fields)
            case 4: break;                                                                  // truncation alone
            }
        }
        const ZkSplit a = zk_split_entry(in, lead, lead + len, nullptr);
        if (a.n == 0) { fprintf(stderr, "no piece\n"); return 3; }
        uint64_t *starts = (uint64_t *)malloc(sizeof(uint64_t) * a.n);                      // exactly the count: one write more is a report
        const ZkSplit b = zk_split_entry(in, lead, lead + len, starts);
        if (a.n != b.n || a.stop != b.stop) { fprintf(stderr, "count and emit disagree\n"); return 3; }
        if (starts[0] != lead) { fprintf(stderr, "the first piece does not begin with the entry\n"); return 3; }
        for (uint32_t j = 1; j < a.n; j++)
            if (starts[j] < starts[j - 1] + 8 || starts[j] > lead + len) { fprintf(stderr, "pieces do not ascend inside the entry\n"); return 3; }
        if (!mutate && a.stop != ZK_OK) { fprintf(stderr, "entry %u of the undamaged archive is not a whole number of frames\n", e); return 4; }
        stopped += a.stop != ZK_OK;
        free(starts); free(in);
    }
    printf("%llu damaged entries, %llu stopped early\n", (unsigned long long)iters, (unsigned long long)stopped);
    return 0;
}

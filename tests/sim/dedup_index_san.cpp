// The kernels of the dedup index (zk_dedup_index.h, the source hipcc compiles) under the emulator, built with AddressSanitizer + UBSan: the
// harness of zk_dedup_index_sim.cpp as a program of its own.  An access outside the source (an exact copy that starts `misalign` bytes into
// its allocation and ends with it), outside a pass's decoded candidates (an allocation of exactly their bytes), outside the index's keys,
// lengths and table (exactly m entries, exactly its slots) or outside the lookup's scratch is a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/dedup_index_san.cpp -o /tmp/dxisan
//   /tmp/dxisan <key bits> <1: every key 0> <misalign> <pass bytes, 0 = default> {<source bytes> <offsets, uint64>}...
// The lists are generations: each is mapped against the archive so far and its fresh frames are appended.  Prints the archive's frames and
// an FNV-1a of every generation's ids | fresh; fails when the two lane orders disagree.
#include "zk_dedup_index_sim.cpp"
#include <cstdio>
#include <cstdlib>
static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> data;
    FILE *f = fopen(path, "rb");
    if (!f) return data;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    return data;
}
static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001B3ull;
    return h;
}
int main(int argc, char **argv)
{
    if (argc < 7 || (argc - 5) % 2) return 2;
    const uint32_t bits = (uint32_t)atoi(argv[1]), misalign = (uint32_t)atoi(argv[3]);
    const bool zero = atoi(argv[2]) != 0;
    const uint64_t pass = strtoull(argv[4], nullptr, 10);
    uint64_t h[2] = {0xCBF29CE484222325ull, 0xCBF29CE484222325ull};
    uint32_t frames[2] = {0, 0};
    for (int d = 0; d < 2; d++) {
        void *x = zkx_sim_create(bits);
        std::vector<uint8_t> arch;
        std::vector<uint64_t> arch_off{0};
        for (int g = 5; g < argc; g += 2) {
            const std::vector<uint8_t> data = slurp(argv[g]), offb = slurp(argv[g + 1]);
            if (offb.size() < 16 || offb.size() % 8) return 2;
            const uint32_t count = (uint32_t)(offb.size() / 8 - 1);
            std::vector<uint64_t> off(count + 1), hash(count, 0);
            memcpy(off.data(), offb.data(), offb.size());
            if (off[count] - off[0] != data.size()) return 2;
            std::vector<uint32_t> ids(count), fresh(count);
            uint32_t nf = 0, rounds = 0, passes = 0;
            uint64_t largest = 0;
            arch.push_back(0);                                                          // (a pointer to hand over when the archive is empty)
            const int rc = zkx_sim_against(x, arch.data(), arch_off.data(), (uint32_t)arch_off.size() - 1, data.data(), data.size(), misalign, off.data(), count,
                                           zero ? hash.data() : nullptr, bits, d, pass, 1, ids.data(), fresh.data(), &nf, &rounds, &passes, &largest);
            arch.pop_back();
            if (rc) { fprintf(stderr, "zkx_sim_against: %d\n", rc); return 1; }
            h[d] = fnv(fnv(h[d], ids.data(), (size_t)count * 4), fresh.data(), (size_t)nf * 4);
            for (uint32_t k = 0; k < nf; k++) {
                const uint64_t a = off[fresh[k]] - off[0], b = off[fresh[k] + 1] - off[0];
                arch.insert(arch.end(), data.begin() + a, data.begin() + b);
                arch_off.push_back(arch.size());
            }
            if (zkx_sim_count(x) != arch_off.size() - 1 || !zkx_sim_table_ok(x)) return 1;
        }
        frames[d] = zkx_sim_count(x);
        zkx_sim_free(x);
    }
    printf("%u %016llx\n", frames[0], (unsigned long long)h[0]);
    return frames[0] == frames[1] && h[0] == h[1] ? 0 : 1;
}

// An encode over a frame list under the workgroup emulator (zk_enc_plan_list_sim.cpp: the plan kernels of zk_enc_plan_dev.h, the list forms
// of the far-history kernels of zk_enc_far.h -- the sources hipcc compiles), built with AddressSanitizer + UBSan: `__shared__` arrays are
// real arrays here and every buffer is an exact-size heap allocation, so an index that leaves the scan's partial sums, a record written
// outside the lists the totals sized, a table entry outside a frame's own table or a byte read behind the source is a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/enc_plan_list_san.cpp -o /tmp/listsan
//   /tmp/listsan <data file> <offsets file: uint64 prefix sums> <level> <slice bytes>
#include "zk_enc_plan_list_sim.cpp"
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
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const std::vector<uint8_t> data = slurp(argv[1]), raw = slurp(argv[2]);
    if (raw.size() < 16 || raw.size() % 8) return 2;
    std::vector<uint64_t> off(raw.size() / 8);
    memcpy(off.data(), raw.data(), raw.size());
    const uint32_t count = (uint32_t)off.size() - 1;
    if (off[count] > data.size()) return 2;
    const int level = atoi(argv[3]);
    const uint64_t slice = strtoull(argv[4], nullptr, 10);
    int bad = 0;
    for (int descending = 0; descending < 2; descending++)
        for (uint64_t plen : {0ull, 1000ull, 200000ull}) {
            const int rc = zk_plan_list_sim_dev(off.data(), count, level, plen, descending);
            if (rc) { printf("plan kernels: %d (prefix %llu, order %d)\n", rc, (unsigned long long)plen, descending); bad = 1; }
        }
    const uint64_t n = off[count] - off[0];
    std::vector<uint64_t> lf(3 * (size_t)count + 3);
    std::vector<uint32_t> table((size_t)1 << 20), cand(n + 1), cand2(n + 1);
    uint32_t nlf = 0;
    const int a = zk_plan_list_sim_encode(data.data(), off.data(), count, level, slice, 0, 0, lf.data(), count, &nlf, table.data(), table.size(), cand.data(),
                                          0xFFFFFFFFu, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ~0ull, nullptr, ~0ull);
    const int d = zk_plan_list_sim_encode(data.data(), off.data(), count, level, slice, 1, 0, lf.data(), count, &nlf, table.data(), table.size(), cand2.data(),
                                          0xFFFFFFFFu, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ~0ull, nullptr, ~0ull);
    uint64_t entries = 0;
    for (uint64_t i = 0; i < n; i++) entries += cand[i] != 0;
    printf("%u frames, %llu bytes, level %d, slices of %llu: %d blocks, %u tables, %llu candidates\n", count, (unsigned long long)n, level, (unsigned long long)slice, a, nlf,
           (unsigned long long)entries);
    return !bad && a >= 0 && d == a && cand == cand2 ? 0 : 1;
}

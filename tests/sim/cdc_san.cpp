// The kernels that find content-defined frame boundaries (zk_cdc.h, the source hipcc compiles) under the workgroup emulator, built with
// AddressSanitizer + UBSan: `__shared__` arrays are real arrays here, so an index that leaves the staged tile, the gear table or the
// selection's chunk -- silent corruption of a neighbouring array in LDS on the device -- is a report; so is an access outside the source
// (an exact copy that starts `misalign` bytes into its allocation and ends with it: the aligned 16-byte loads must stay inside), the
// bitmap, the tile counts, the candidate list or the offsets, which the harness allocates at exactly the sizes zk_cdc_pass gives them.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/cdc_san.cpp -o /tmp/cdcsan
//   /tmp/cdcsan <file> <min> <bits> <max> <slice bytes, 0 = default> <misalign> <off_cap>
// Prints the number of frames; fails when the two lane orders disagree.
#include "zk_cdc_sim.cpp"
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
    if (argc != 8) return 2;
    const std::vector<uint8_t> data = slurp(argv[1]);
    if (data.empty()) return 2;
    const uint32_t min = (uint32_t)atoi(argv[2]), bits = (uint32_t)atoi(argv[3]), max = (uint32_t)atoi(argv[4]), misalign = (uint32_t)atoi(argv[6]);
    const uint64_t slice = strtoull(argv[5], nullptr, 10), off_cap = strtoull(argv[7], nullptr, 10);
    std::vector<uint8_t> bm((data.size() + 7) / 8), bm2(bm.size());
    std::vector<uint64_t> off(off_cap + 1), off2(off_cap + 1);
    uint64_t count = 0, count2 = 0;
    const int a = zk_cdc_sim(data.data(), data.size(), min, bits, max, slice, misalign, 0, bm.data(), off.data(), off_cap, &count);
    const int b = zk_cdc_sim(data.data(), data.size(), min, bits, max, slice, misalign, 1, bm2.data(), off2.data(), off_cap, &count2);
    printf("%llu frames\n", (unsigned long long)count);
    return a == 0 && b == 0 && count == count2 && bm == bm2 && off == off2 ? 0 : 1;
}

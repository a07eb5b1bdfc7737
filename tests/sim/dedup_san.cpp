// The kernels that find duplicate frames (zk_dedup.h, the source hipcc compiles) under the emulator, built with AddressSanitizer + UBSan:
// an access outside the source is a report -- an exact copy that starts `misalign` bytes into its allocation and ends with it, so the
// aligned 16-byte loads of the long compare, the 8-byte loads of a lane's compare and the gather's copies must stay inside the frames --,
// and so is one outside the table, the lists, the outputs or a gathered slice, which the harness allocates at exactly the sizes
// zk_dedup_core and zk_dedup_encode give them.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/dedup_san.cpp -o /tmp/dedupsan
//   /tmp/dedupsan <source bytes> <offsets, uint64> <hashes, uint64, or - for zk_k_dedup_hash's> <key bits> <misalign> <slice bytes, 0 = default>
// Prints n_unique, the rounds, the slices and an FNV-1a of ref | ids; fails when the two lane orders disagree (the gathered bytes too).
#include "zk_dedup_sim.cpp"
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
    if (argc != 7) return 2;
    const bool own = !strcmp(argv[3], "-");
    const std::vector<uint8_t> data = slurp(argv[1]), offb = slurp(argv[2]), hashb = own ? std::vector<uint8_t>() : slurp(argv[3]);
    if (offb.size() < 16 || offb.size() % 8 || (!own && hashb.size() != offb.size() - 8)) return 2;
    const uint32_t count = (uint32_t)(offb.size() / 8 - 1), bits = (uint32_t)atoi(argv[4]), misalign = (uint32_t)atoi(argv[5]);
    const uint64_t slice = strtoull(argv[6], nullptr, 10);
    std::vector<uint64_t> off(count + 1), hash(count);
    memcpy(off.data(), offb.data(), offb.size());
    if (!own) memcpy(hash.data(), hashb.data(), hashb.size());
    if (off[count] - off[0] != data.size()) return 2;
    std::vector<uint32_t> ref[2], uniq[2], ids[2];
    std::vector<uint8_t> got[2];
    uint32_t nu[2] = {0, 0}, rounds[2] = {0, 0}, slices[2] = {0, 0};
    for (int d = 0; d < 2; d++) {
        ref[d].resize(count); uniq[d].resize(count); ids[d].resize(count); got[d].assign(data.size() + 1, 0);
        if (zk_dedup_sim(data.data(), data.size(), misalign, off.data(), count, own ? nullptr : hash.data(), bits, d, ref[d].data(), uniq[d].data(), ids[d].data(), &nu[d], &rounds[d],
                         got[d].data(), slice, &slices[d], nullptr)) return 1;
    }
    uint64_t h = fnv(fnv(0xCBF29CE484222325ull, ref[0].data(), (size_t)count * 4), ids[0].data(), (size_t)count * 4);
    printf("%u %u %u %016llx\n", nu[0], rounds[0], slices[0], (unsigned long long)h);
    return nu[0] == nu[1] && ref[0] == ref[1] && ids[0] == ids[1] && uniq[0] == uniq[1] && got[0] == got[1] ? 0 : 1;
}

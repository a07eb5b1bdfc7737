// The digest kernels (zk_digest.h, the source hipcc compiles) under the emulator, built with AddressSanitizer + UBSan: the harness of
// zk_digest_sim.cpp as a program of its own.  The source is an allocation that starts `misalign` bytes in and ends with its last byte, the
// offsets, the digests and the scratch allocations of exactly the layout's sizes: a load that leaves the list -- a 16-byte piece over a
// frame's end, a slab past the last leaf -- or a store outside the digests is a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/digest_san.cpp -o /tmp/digestsan
//   /tmp/digestsan <algo: 1 SHA-256, 2 BLAKE2s tree> <misalign> <source bytes> <offsets, uint64>
// Runs the list in both lane orders; prints the digests in hex, one line; fails when the orders disagree or a byte behind the digests changed.
#include "zk_digest_sim.cpp"
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
    if (argc != 5) return 2;
    const int algo = atoi(argv[1]);
    const uint32_t misalign = (uint32_t)atoi(argv[2]);
    const std::vector<uint8_t> data = slurp(argv[3]), offb = slurp(argv[4]);
    if (offb.size() < 16 || offb.size() % 8) return 2;
    const uint32_t count = (uint32_t)(offb.size() / 8 - 1);
    std::vector<uint64_t> off((size_t)count + 1);
    memcpy(off.data(), offb.data(), offb.size());
    if (off[count] - off[0] != data.size()) return 2;
    constexpr size_t GUARD = 64;
    std::vector<uint8_t> out[2];
    for (int d = 0; d < 2; d++) {
        out[d].assign((size_t)count * ZKG_BYTES + GUARD, 0xA5);
        if (zk_digest_sim(algo, data.empty() ? nullptr : data.data(), off.data(), count, misalign, d, out[d].data(), out[d].size())) return 1;
        for (size_t g = 0; g < GUARD; g++) if (out[d][(size_t)count * ZKG_BYTES + g] != 0xA5) { fprintf(stderr, "a write behind the digests\n"); return 1; }
    }
    for (size_t i = 0; i < (size_t)count * ZKG_BYTES; i++) printf("%02x", out[0][i]);
    printf("\n");
    return out[0] == out[1] ? 0 : 1;
}

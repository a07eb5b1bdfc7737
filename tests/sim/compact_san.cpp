// The kernels that remove frames from an archive (zk_compact.h, the source hipcc compiles) under the emulator, built with AddressSanitizer +
// UBSan: the harness of zk_compact_sim.cpp as a program of its own.  The source is an exact copy that starts `misalign` bytes into its
// allocation and ends with the archive's last byte; a destination of its own is an allocation of exactly `written` bytes, a staged step's
// scratch of exactly the step, every array of the scratch of exactly its entries: an access outside any of them is a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/compact_san.cpp -o /tmp/cmpsan
//   /tmp/cmpsan <misalign> <slice bytes, 0 = default> <archive bytes> <c_off, uint64> <d_off, uint64> <live, uint8>
// Runs the archive out of place and in place, in both lane orders; marks the kept frames through zk_k_cmp_mark and renumbers them through
// zk_k_cmp_remap_ids.  Prints n_kept, written and an FNV-1a of remap | c_off_out | d_off_out | the destination's bytes for the out-of-place and
// the in-place run; fails when the two lane orders disagree.
#include "zk_compact_sim.cpp"
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
    const uint32_t misalign = (uint32_t)atoi(argv[1]);
    const uint64_t slice = strtoull(argv[2], nullptr, 10);
    const std::vector<uint8_t> comp = slurp(argv[3]), cb = slurp(argv[4]), db = slurp(argv[5]), live_in = slurp(argv[6]);
    if (cb.size() < 16 || cb.size() % 8 || db.size() != cb.size() || live_in.size() != cb.size() / 8 - 1) return 2;
    const uint32_t n = (uint32_t)live_in.size();
    std::vector<uint64_t> c_off(n + 1), d_off(n + 1);
    memcpy(c_off.data(), cb.data(), cb.size());
    memcpy(d_off.data(), db.data(), db.size());
    if (c_off[n] != comp.size()) return 2;
    // the kept frames as a list of ids (some twice), marked into an array of zeroes
    std::vector<uint32_t> ids;
    for (uint32_t s = 0; s < n; s++) if (live_in[s]) { ids.push_back(s); if (s % 3 == 0) ids.push_back(s); }
    uint64_t h[2][2];
    uint32_t kept[2] = {0, 0};
    uint64_t written[2] = {0, 0};
    for (int d = 0; d < 2; d++) {
        std::vector<uint8_t> live(n, 0);
        if (zk_compact_sim_mark(ids.data(), (uint32_t)ids.size(), n, live.data(), d)) return 1;
        for (uint32_t s = 0; s < n; s++) if ((live[s] != 0) != (live_in[s] != 0)) return 1;
        for (int in_place = 0; in_place < 2; in_place++) {
            std::vector<uint32_t> remap(n);
            std::vector<uint64_t> c_out(n + 1), d_out(n + 1);
            std::vector<uint8_t> buf(comp.size() + 1);
            uint32_t nk = 0, steps = 0, staged = 0;
            uint64_t wr = 0;
            const int rc = zk_compact_sim(comp.data(), misalign, c_off.data(), d_off.data(), n, live.data(), in_place, slice, d, remap.data(), c_out.data(), d_out.data(), &nk,
                                          &wr, buf.data(), &steps, &staged);
            if (rc) { fprintf(stderr, "zk_compact_sim: %d\n", rc); return 1; }
            std::vector<uint32_t> out(ids.size() + 1);
            if (zk_compact_sim_remap_ids(remap.data(), n, ids.data(), (uint32_t)ids.size(), out.data(), d)) return 1;
            for (size_t i = 0; i < ids.size(); i++) if (out[i] != remap[ids[i]]) return 1;
            uint64_t x = fnv(fnv(fnv(0xCBF29CE484222325ull, remap.data(), (size_t)n * 4), c_out.data(), ((size_t)nk + 1) * 8), d_out.data(), ((size_t)nk + 1) * 8);
            h[d][in_place] = fnv(x, buf.data() + c_off[0], (size_t)(wr - c_off[0]));
            kept[d] = nk; written[d] = wr;
        }
    }
    printf("%u %llu %016llx %016llx\n", kept[0], (unsigned long long)written[0], (unsigned long long)h[0][0], (unsigned long long)h[0][1]);
    return kept[0] == kept[1] && written[0] == written[1] && h[0][0] == h[1][0] && h[0][1] == h[1][1] ? 0 : 1;
}

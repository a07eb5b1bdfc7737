// The encoder's far-history kernels (zk_enc_far.h, the source hipcc compiles) under the workgroup emulator, built with AddressSanitizer +
// UBSan: `__shared__` arrays are real arrays here, so an index that leaves the pass tables, the per-wave cursors or the chunk counters of
// zk_k_enc_dense_part / zk_k_enc_dense_cand -- silent corruption of a neighbouring array in LDS on the device -- is a report; so is an access
// outside the source, the prefix copy (+ ZKE_LDM_SLACK), the candidate and position arrays (+ ZKE_DENSE_SLACK), the pass offsets, the
// sampled tables or the matcher's records, which the harness allocates at exactly the engine's sizes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/enc_far_san.cpp -o /tmp/farsan
//   /tmp/farsan frames <file> <frame size> <level> <slice bytes>      dense kernels (both lane orders) + in-frame sampled tables
//   /tmp/farsan prefix <file> <frame size> <level> <prefix bytes>     the file's first <prefix bytes> as the prefix of the rest: table + records
#include "zk_enc_far_sim.cpp"
#include <cstdio>
#include <cstdlib>
#include <string>
int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const std::string mode = argv[1];
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    const uint32_t fs = (uint32_t)strtoul(argv[3], nullptr, 10);
    const int level = atoi(argv[4]);
    const uint64_t arg = strtoull(argv[5], nullptr, 10);
    if (mode == "frames") {
        const uint64_t n = data.size();
        ZkEncPlan pl;
        if (!zke_plan_count(n, fs, 0, &pl)) return 2;
        std::vector<uint32_t> cand(n), part(n), poff((size_t)pl.nseg * (ZKD_NBMAX + 1)), cand2(n), table((size_t)pl.nf << 20);
        const int a = zk_enc_far_sim_dense(data.data(), n, fs, level, arg, 0, cand.data(), part.data(), poff.data());
        const int d = zk_enc_far_sim_dense(data.data(), n, fs, level, arg, 1, cand2.data(), part.data(), poff.data());
        const int log = zk_enc_far_sim_ldm_frames(data.data(), n, fs, level, 0, table.data(), table.size());
        uint64_t entries = 0;
        for (uint64_t i = 0; i < n; i++) entries += cand[i] != 0;
        printf("%llu bytes, frames of %u, level %d, slices of %llu: %d segments, %llu entries, table log %d\n", (unsigned long long)n, fs, level,
               (unsigned long long)arg, a, (unsigned long long)entries, log);
        return a == (int)pl.nseg && d == a && cand == cand2 && log >= 10 ? 0 : 1;
    }
    if (mode == "prefix") {
        if (arg > data.size()) return 2;
        const uint8_t *prefix = data.data(), *src = data.data() + arg;
        const uint64_t n = data.size() - arg;
        std::vector<uint32_t> table((size_t)1 << 23);
        const int log = zk_enc_far_sim_ldm_prefix(prefix, arg, 0, table.data(), table.size());
        std::vector<uint8_t> stage((n / fs + 1) * ((size_t)ZKE_WINDOW + fs));
        const int hist = zk_enc_far_sim_stage_hist(src, n, fs, level, prefix, arg, stage.data(), stage.size());
        printf("prefix %llu, %llu bytes in frames of %u: table log %d, history %d\n", (unsigned long long)arg, (unsigned long long)n, fs, log, hist);
        return hist >= 0 && (log >= 10) == (arg > ZKE_WINDOW) ? 0 : 1;
    }
    return 2;
}

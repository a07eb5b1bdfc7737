// The kernels that select a trained dictionary's content (zk_train.h, the source hipcc compiles) under the workgroup emulator, built with
// AddressSanitizer + UBSan: `__shared__` arrays are real arrays here, so an index that leaves the prefix sums or the reduction arrays of
// zk_k_train_select -- silent corruption of a neighbouring array in LDS on the device -- is a report; so is an access outside the samples
// (an exact copy, nothing readable behind the last one), the offsets, the per-position hashes, the counters, a candidate's content or its
// segment list, which the harness allocates at exactly the sizes zk_train_run gives them.
// The host writer of the header (zk_train_host.h) runs here too, on the samples' byte histogram and on sequence histograms of zeros, of one
// count of 2^63 and of a ramp, into a heap buffer of exactly 512 bytes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/train_san.cpp -o /tmp/trainsan
//   /tmp/trainsan <file of samples> <file of count + 1 uint64 offsets> <d> <f> <content capacity> <k> [<k> ...]
#include "zk_train_sim.cpp"
#include "../../zeekstd_amd/csrc/zk_train_host.h"
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
    if (argc < 7 || argc > 6 + (int)ZKT_CANDS_MAX) return 2;
    const std::vector<uint8_t> data = slurp(argv[1]), offb = slurp(argv[2]);
    if (offb.size() < 16 || offb.size() % 8) return 2;
    std::vector<uint64_t> off(offb.size() / 8);
    memcpy(off.data(), offb.data(), offb.size());
    const uint32_t count = (uint32_t)off.size() - 1, d = (uint32_t)atoi(argv[3]), f = (uint32_t)atoi(argv[4]), ccap = (uint32_t)atoi(argv[5]), nk = (uint32_t)argc - 6;
    if (off[count] > data.size() || off[count] <= off[0]) return 2;
    uint32_t ks[ZKT_CANDS_MAX];
    for (uint32_t c = 0; c < nk; c++) ks[c] = (uint32_t)atoi(argv[6 + c]);
    const uint32_t n = (uint32_t)(off[count] - off[0]), segs_cap = ccap / ks[0] + 1;
    std::vector<uint32_t> hpos(n), freq((size_t)1 << f), segs((size_t)nk * segs_cap), segs2(segs.size()), out(2 * nk), out2(2 * nk);
    std::vector<uint8_t> content((size_t)nk * ccap), content2(content.size());
    const int a = zk_train_sim(data.data(), off.data(), count, d, f, ks, nk, ccap, 0, hpos.data(), freq.data(), segs.data(), segs_cap, content.data(), out.data());
    const int b = zk_train_sim(data.data(), off.data(), count, d, f, ks, nk, ccap, 1, hpos.data(), freq.data(), segs2.data(), segs_cap, content2.data(), out2.data());
    for (uint32_t c = 0; c < nk; c++) printf("k = %u: %u segments, %u bytes\n", ks[c], out[2 * c], out[2 * c + 1]);
    bool same = out == out2;
    for (uint32_t c = 0; c < nk && same; c++) {
        same = memcmp(segs.data() + (size_t)c * segs_cap, segs2.data() + (size_t)c * segs_cap, (size_t)out[2 * c] * 4) == 0 &&
               memcmp(content.data() + (size_t)(c + 1) * ccap - out[2 * c + 1], content2.data() + (size_t)(c + 1) * ccap - out[2 * c + 1], out[2 * c + 1]) == 0;
    }
    // the header writer
    uint64_t lit[256] = {0}, zero[256] = {0}, one[256] = {0}, ramp[64];
    for (uint32_t i = 0; i < n; i++) lit[data[off[0] + i]]++;
    one[5] = 1ull << 63;
    for (int i = 0; i < 64; i++) ramp[i] = (uint64_t)i * i * i;
    bool wrote = true;
    for (const uint64_t *h : {zero, one, ramp}) {
        const auto head = zkt_exact<uint8_t>(ZKT_HEADER_RESERVE);
        const size_t hb = zkt_write_header(h == ramp ? lit : h == one ? one : zero, h, h, h, zkt_dict_id(content.data(), content.size()), head.get(), ZKT_HEADER_RESERVE);
        printf("header: %zu bytes\n", hb);
        wrote = wrote && hb > 20 && hb <= ZKT_HEADER_RESERVE;
    }
    return a == 0 && b == 0 && same && wrote ? 0 : 1;
}

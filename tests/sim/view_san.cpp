// The kernels of zk_read_view_ranges_dev (zk_view.h, the source hipcc compiles) under the emulator, built with AddressSanitizer + UBSan: the
// harness of zk_view_sim.cpp as a program of its own.  The destination is an allocation that starts `misalign` bytes in and ends with its last
// byte, a pass's scratch an allocation of exactly the pass's bytes, every array of the plan of exactly its entries: an access outside any of
// them is a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/view_san.cpp -o /tmp/viewsan
//   /tmp/viewsan <misalign> <pass bytes, 0 = default> <dst_cap> <size> <frames' bytes> <d_off> <ids> <voff> <offs> <lens> <dst_off or -> <frame_err or ->
// (uint64 arrays but ids: uint32 and frame_err: int32.)  Runs the case in both lane orders; prints the return value, the frames decoded, the
// passes and a positional checksum of the destination and of the statuses; fails when the two orders disagree.
#include "zk_view_sim.cpp"
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
template <class T> static std::vector<T> as(const std::vector<uint8_t> &b)
{
    std::vector<T> v(b.size() / sizeof(T) + 1);
    if (!b.empty()) memcpy(v.data(), b.data(), b.size() / sizeof(T) * sizeof(T));
    return v;
}
// a checksum that numpy restates without a loop: the sum of (byte + 1) * (position * K + 1) modulo 2^64
static uint64_t possum(const void *p, size_t n)
{
    uint64_t h = 0;
    for (size_t i = 0; i < n; i++) h += (uint64_t)(((const uint8_t *)p)[i] + 1) * ((uint64_t)i * 0x9E3779B97F4A7C15ull + 1);
    return h;
}
int main(int argc, char **argv)
{
    if (argc != 13) return 2;
    const uint32_t misalign = (uint32_t)atoi(argv[1]);
    const uint64_t pass = strtoull(argv[2], nullptr, 10), dst_cap = strtoull(argv[3], nullptr, 10), size = strtoull(argv[4], nullptr, 10);
    std::vector<uint8_t> data = slurp(argv[5]);
    const std::vector<uint8_t> db = slurp(argv[6]), ib = slurp(argv[7]), vb = slurp(argv[8]), ob = slurp(argv[9]), lb = slurp(argv[10]);
    const bool packed = strcmp(argv[11], "-") == 0, fine = strcmp(argv[12], "-") == 0;
    const std::vector<uint8_t> tb = packed ? std::vector<uint8_t>() : slurp(argv[11]), eb = fine ? std::vector<uint8_t>() : slurp(argv[12]);
    if (db.size() < 8 || vb.size() < 8 || vb.size() / 8 != ib.size() / 4 + 1 || ob.size() != lb.size() || (!packed && tb.size() != ob.size())) return 2;
    const uint32_t n = (uint32_t)(db.size() / 8 - 1), vcount = (uint32_t)(ib.size() / 4), count = (uint32_t)(ob.size() / 8);
    if (!fine && eb.size() != (size_t)n * 4) return 2;
    const auto d_off = as<uint64_t>(db), voff = as<uint64_t>(vb), offs = as<uint64_t>(ob), lens = as<uint64_t>(lb), given = as<uint64_t>(tb);
    const auto ids = as<uint32_t>(ib);
    const auto ferr = as<int32_t>(eb);
    if (d_off[n] != data.size()) return 2;
    data.push_back(0);
    uint64_t h[2], out2[2][2];
    int rc[2];
    for (int d = 0; d < 2; d++) {
        std::vector<uint8_t> dst((size_t)size + 1, 0xA5);
        std::vector<int32_t> st((size_t)count + 1, -12345);
        rc[d] = zk_view_sim(data.data(), d_off.data(), n, ids.data(), voff.data(), vcount, offs.data(), lens.data(), packed ? nullptr : given.data(), count, dst.data(), dst_cap,
                            size, misalign, pass, fine ? nullptr : ferr.data(), d, st.data(), out2[d]);
        if (rc[d] == -5) { fprintf(stderr, "zk_view_sim: a write outside the destination\n"); return 1; }
        h[d] = possum(dst.data(), (size_t)size) ^ (possum(st.data(), (size_t)count * 4) << 1);
    }
    printf("%d %llu %llu %016llx\n", rc[0], (unsigned long long)out2[0][0], (unsigned long long)out2[0][1], (unsigned long long)h[0]);
    return rc[0] == rc[1] && h[0] == h[1] && out2[0][0] == out2[1][0] && out2[0][1] == out2[1][1] ? 0 : 1;
}

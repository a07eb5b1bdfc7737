// The decoder's XXH64 kernels (zk_xxh64.h, the source hipcc compiles) under the workgroup emulator, built with AddressSanitizer + UBSan:
// zk_xxh_sim.cpp gives every buffer a kernel sees -- the frames' bytes at their alignment, the offsets, infos, hashes, skip and progress
// words -- a heap allocation of exactly its size, so that a read in front of the first frame or behind the last one (a lane without a
// frame that reads frame 0, the last round of a double-batch loop that reads the first batch again, a 16-byte load at a frame's end, a
// follower that reads ahead of a word) is a report.  `__shared__` arrays are real arrays here: so is an index that leaves the ring.
// Every job runs in both lane orders and its results are held against what the job expects.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/sim/xxh_san.cpp -o /tmp/xxhsan
//   /tmp/xxhsan <file of jobs: tests/helpers/xxh_inputs.py, pack_job>
#include "zk_xxh_sim.cpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::vector<uint64_t> w;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        uint64_t buf[8192];
        for (size_t k; (k = fread(buf, 8, 8192, f)) > 0;) w.insert(w.end(), buf, buf + k);
        fclose(f);
    }
    size_t at = 0, jobs = 0;
    const auto take = [&](size_t n) { const uint64_t *p = w.data() + at; at += n; if (at > w.size()) { fprintf(stderr, "job %zu: truncated\n", jobs); exit(2); } return p; };
    const auto narrow = [](const uint64_t *p, size_t n) { std::vector<uint32_t> v(n); for (size_t i = 0; i < n; i++) v[i] = (uint32_t)p[i]; return v; };
    while (at < w.size()) {
        const uint64_t *h = take(13);
        const uint32_t follow = (uint32_t)h[0], kernel = (uint32_t)h[1], first = (uint32_t)h[2], count = (uint32_t)h[3], align = (uint32_t)h[4];
        const bool with_infos = h[5] != 0, with_skip = h[6] != 0, with_hashes = h[12] != 0;
        const uint32_t nev = (uint32_t)h[7], nwg = (uint32_t)h[8];
        const uint64_t tick = h[9], max_polls = h[10], nbytes = h[11];
        const uint64_t *d_off = take((size_t)first + count + 1);
        const std::vector<uint32_t> st = narrow(take(count), count), fl = narrow(take(count), count), ck = narrow(take(count), count);
        const uint64_t *skip = take(count);
        const uint64_t *evw = take((size_t)nev * 5);
        const std::vector<uint32_t> wg = narrow(take(nwg), nwg);
        const uint64_t *want_hash = take(count), *want_status = take(count), *want_progress = take(count);
        const uint8_t *bytes = (const uint8_t *)take((nbytes + 7) / 8);
        for (int desc = 0; desc < 2; desc++) {
            if (follow) {
                std::vector<ZkxEvent> ev(nev);
                for (uint32_t e = 0; e < nev; e++) ev[e] = ZkxEvent{(uint32_t)evw[5 * e], (uint32_t)evw[5 * e + 1], (uint32_t)evw[5 * e + 2], (uint32_t)evw[5 * e + 3], (uint32_t)evw[5 * e + 4]};
                std::vector<uint64_t> prog(count), polls(nwg);
                const int rc = zk_xxh_sim_follow(bytes, nbytes, align, d_off, first, count, st.data(), fl.data(), ck.data(), ev.data(), nev, wg.data(), tick, max_polls, desc,
                                                 prog.data(), polls.data());
                if (rc != 0) { fprintf(stderr, "job %zu (follower, %u frames): rc %d\n", jobs, count, rc); return 1; }
                for (uint32_t f = 0; f < count; f++) if (prog[f] != want_progress[f]) {
                    fprintf(stderr, "job %zu (follower, %u frames, order %d): frame %u's word is %016llx, expected %016llx\n", jobs, count, desc, f,
                            (unsigned long long)prog[f], (unsigned long long)want_progress[f]);
                    return 1;
                }
                continue;
            }
            std::vector<uint32_t> status = st;
            std::vector<uint64_t> hashes(count, 0x5A5A5A5A5A5A5A5Aull);
            const int rc = zk_xxh_sim_pass((int)kernel, bytes, nbytes, align, d_off, first, count, with_infos ? status.data() : nullptr, fl.data(), ck.data(),
                                           with_hashes || !with_infos ? hashes.data() : nullptr, with_skip ? skip : nullptr, desc);
            if (rc != 0) { fprintf(stderr, "job %zu (kernel %u, %u frames): rc %d\n", jobs, kernel, count, rc); return 1; }
            for (uint32_t f = 0; f < count; f++) {
                if (with_hashes && hashes[f] != want_hash[f]) { fprintf(stderr, "job %zu (kernel %u, order %d): frame %u's hash\n", jobs, kernel, desc, f); return 1; }
                if (with_infos && status[f] != want_status[f]) { fprintf(stderr, "job %zu (kernel %u, order %d): frame %u's status %u\n", jobs, kernel, desc, f, status[f]); return 1; }
            }
        }
        jobs++;
    }
    printf("%zu jobs\n", jobs);
    return 0;
}

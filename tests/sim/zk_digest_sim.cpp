// zk_digest_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels of zk_frame_digests_dev (zeekstd_amd/csrc/zk_digest.h, the very source hipcc compiles for gfx950) on the CPU under the
// emulator of hip_wg_emu.h, with the launchers' grids (zk_digest.hip: zkg_enqueue), in ascending or descending order of lanes AND
// workgroups.  tests/test_sim_digest.py compares every digest with hashlib (tests/helpers/digest_model.py); tests/sim/digest_san.cpp runs the
// same under AddressSanitizer + UBSan.  Every array a kernel sees is a heap allocation of exactly its size: the source starts `misalign`
// bytes into its allocation and ends with its last byte, the offsets hold count + 1 words, the scratch is ZkgLayout's, the digests are
// 32 * count bytes -- the caller's poisoned buffer is copied in and out, so what lies behind them there must come back unchanged.
//   The kernels' lanes meet at wave fences (the slab), so every workgroup runs as fibres (emu_run_workgroup).  zk_k_scan64 (zk_encode.hip) is
// restated in plain C++.  zk_digest_sim_long_sha256 calls the LANE code directly, outside the emulator, on one frame longer than 2^32 bits.
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_digest.h"
#include <memory>

template <class T> static std::unique_ptr<T[]> zkg_exact(size_t n, int fill = 0xA5)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    memset(p.get(), fill, (n ? n : 1) * sizeof(T));
    return p;
}
static void zkg_grid(uint32_t grid, bool descending, const std::function<void()> &body)
{
    for (uint32_t bi = 0; bi < grid; bi++) emu_run_workgroup(ZKG_THREADS, descending ? grid - 1 - bi : bi, body, grid);
}

// the plan functions, for literal expectations
extern "C" uint64_t zkg_sim_leaves(uint64_t len) { return zkg_leaves(len); }
extern "C" uint32_t zkg_sim_blocks(uint64_t lanes) { return zkg_blocks(lanes); }
extern "C" uint32_t zkg_sim_pass_end(const uint64_t *off, uint32_t a, uint32_t n, uint64_t pass_max) { return zkg_pass_end(off, a, n, pass_max); }
extern "C" uint64_t zkg_sim_scratch(uint32_t count, uint64_t total_leaves) { return zkg_layout(count, total_leaves).end; }

// "zk_frame_digests_dev".  src_in: the bytes [off[0], off[count]) (NULL when there are none); out_io[out_size]: the caller's buffer, its
// first 32 * count bytes receive the digests.  Returns 0, or -5 when anything behind the digests changed
extern "C" int zk_digest_sim(int algo, const uint8_t *src_in, const uint64_t *off_in, uint32_t count, uint32_t misalign, int descending, uint8_t *out_io, uint64_t out_size)
{
    if (count == 0) return 0;
    const bool desc = descending != 0;
    const uint64_t n = off_in[count] - off_in[0], base = off_in[0];
    const auto block = zkg_exact<uint8_t>((size_t)n + misalign, 0xEE);
    uint8_t *src = block.get() + misalign;
    if (n) memcpy(src, src_in, (size_t)n);
    const auto off = zkg_exact<uint64_t>((size_t)count + 1);
    memcpy(off.get(), off_in, ((size_t)count + 1) * 8);
    const auto digests = zkg_exact<uint32_t>((size_t)count * 8);
    memcpy(digests.get(), out_io, (size_t)count * ZKG_BYTES);

    emu_set_lane_order(desc);
    if (algo == ZKG_SHA256) {
        zkg_grid(zkg_blocks(count), desc, [&] { zk_k_digest_sha256(n ? src : nullptr, off.get(), base, count, digests.get()); });
    } else {
        uint64_t total = 0;
        for (uint32_t i = 0; i < count; i++) total += zkg_leaves(off[i + 1] - off[i]);
        const ZkgLayout L = zkg_layout(count, total);
        const auto cnt = zkg_exact<uint64_t>((L.lp - L.cnt) / 8), lp = zkg_exact<uint64_t>((L.leaves - L.lp) / 8);
        const auto leaves = zkg_exact<uint32_t>((L.end - L.leaves) / 4);
        zkg_grid(zkg_blocks(count), desc, [&] { zk_k_digest_counts(off.get(), count, cnt.get()); });
        uint64_t s = 0;                                     // zk_k_scan64: the exclusive scan of count values, the total behind it
        for (uint32_t i = 0; i < count; i++) { lp[i] = s; s += cnt[i]; }
        lp[count] = s;
        if (s != total) return -6;
        zkg_grid(zkg_blocks(total), desc, [&] { zk_k_digest_leaves(n ? src : nullptr, off.get(), base, count, lp.get(), total, leaves.get()); });
        zkg_grid(zkg_blocks(count), desc, [&] { zk_k_digest_roots(leaves.get(), lp.get(), count, digests.get()); });
    }
    emu_set_lane_order(false);
    int rc = 0;
    for (uint32_t m = 0; m < misalign; m++) if (block[m] != 0xEE) rc = -5;
    memcpy(out_io, digests.get(), (size_t)count * ZKG_BYTES);
    (void)out_size;
    return rc;
}

// SHA-256 of len bytes, byte i = (i ^ (i >> 8)) & 255, by the lane code alone (zkg_sha256_init / _step, as zkg_sha256_wave drives them): the
// blocks are made here as the stager leaves them in a lane's row -- the message, 0x80 behind it, zeros.  out: the 32 bytes of the digest
extern "C" void zk_digest_sim_long_sha256(uint64_t len, uint8_t *out)
{
    ZkgSha q;
    zkg_sha256_init(q, len);
    while (!q.done) {
        uint8_t b[64];
        const uint64_t p = q.pos;
        for (uint32_t k = 0; k < 64; k++) { const uint64_t i = p + k; b[k] = i < len ? (uint8_t)(i ^ (i >> 8)) : i == len ? 0x80 : 0; }
        uint32_t w[16];
        for (int i = 0; i < 16; i++) { uint32_t x; memcpy(&x, b + 4 * i, 4); w[i] = __builtin_bswap32(x); }
        zkg_sha256_step(q, w);
    }
    for (int i = 0; i < 8; i++) { const uint32_t x = __builtin_bswap32(q.s[i]); memcpy(out + 4 * i, &x, 4); }
}

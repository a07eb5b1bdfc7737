// zk_digest.h -- content digests of the frames of a list (zk_frame_digests[_dev], zk_archive_digests_dev, include/zeekstd_amd.h "THE DIGEST";
// DESIGN.md 5o): the lane code and the kernels (included by zk_digest.hip, which keeps their launchers; tests/sim/zk_digest_sim.cpp runs the
// same source on the CPU under the workgroup emulator, against hashlib).
//   lane code   zkg_sha256_block / zkg_blake2s_block: one compression, every round unrolled -- the message schedule and BLAKE2s's
//               permutation are compile-time indices, so the sixteen message words stay in registers --, rotates as v_alignbit.
//               zkg_sha256_step / zkg_blake2s_step: a message as a chain of 64-byte blocks, ONE call site of the compression each (padding,
//               the 64-bit bit length and the final flags are values, not branches around a second copy)
//   dealing     lanes are dealt over the whole LIST, never a workgroup per frame (a list of 4 KiB frames would run one lane in 256):
//               SHA-256 a lane per frame; BLAKE2s a lane per LEAF of 4096 bytes -- zk_k_digest_counts gives the leaves of every frame,
//               zk_k_scan64 (zk_encode.hip) their prefix sums, a lane finds its frame by binary search in them as zk_k_view_gather finds
//               its range -- and then a lane per frame for the root over the frame's leaf digests, which lie in engine scratch (1/128
//               of the input)
//   loading     a lane that walked its own message with 16-byte loads would give wave instructions whose 64 lanes read 64 different
//               rows (4 KiB apart for leaves), a shape that loads at a small fraction of the streaming rate.  So a WAVE
//               stages the next ZKG_SLAB = 256 bytes of each of its 64 messages through LDS (zkg_stage): 16 lanes x 16 bytes per message,
//               four messages per load instruction, at any alignment (like zk_k_dedup_hash); the last bytes of a message are fetched one by one,
//               so that no load leaves it.  A message's row is ZKG_SLAB + 16 bytes apart from the next: the 16-byte reads of the lanes
//               of a ds_read_b128 group fall into 16 different 16-byte slots, and so do the writes of a message's 16 lanes.  Where a
//               lane's message goes on, and how many bytes of it are left, the fetching lanes read from a slot per lane behind the rows.
//               Lanes whose message is finished publish ZKG_DONE and are skipped; SHA-256's 0x80 is put behind the last byte by the stager
// Every store is a vector store.  No lane waits for another except at the wave fence on either side of the slab.  Plain C++ only.
#pragma once
#include <stdint.h>
#include <string.h>
#include "zk_device.h"

// Slab and workgroup, measured on 1 GiB of text cut at avg_size 4 KiB / 64 KiB / 2 MiB (tools/digest_probe.py --digests-only under the libraries
// of tools/build_digest_variant.sh; profiles/digest_probe.txt; DESIGN.md 5o has the table) -- ms of the leaf pass | of SHA-256's frame pass:
//   256 bytes, 2 waves (chosen)   0.98 / 0.70 / 0.70 | 3.7 / 20.7 / 703-807      128 bytes   0.87 / 0.69 / 0.68 | 3.5 / 20.7 / 759
//   512 bytes                     1.25 / 0.82 / 0.79 | 4.5 / 21.0 / 740          4 waves     0.96 / 0.71 / 0.69 | 3.7 / 25.5 / 692
//   no slab, every lane four 16-byte loads at its own address (ZKG_DIRECT)         1.43 / 0.73 / 0.64 | 4.5 / 24.5 / 798
// The kernels are bound by their integer work: the staging buys 5-45 % at 4 KiB and 64 KiB, not the factor of the uncoalesced load alone.
// The three switches exist for that measurement only
#ifndef ZKG_SLAB_BYTES
#define ZKG_SLAB_BYTES 256
#endif
#ifndef ZKG_WAVES_PER_WG
#define ZKG_WAVES_PER_WG 2
#endif
constexpr uint32_t ZKG_WAVES = ZKG_WAVES_PER_WG;            // waves per workgroup: each has its own slab rows, no workgroup barrier
constexpr uint32_t ZKG_THREADS = 64 * ZKG_WAVES;
constexpr uint32_t ZKG_SLAB = ZKG_SLAB_BYTES;               // bytes of a message staged at a time
constexpr uint32_t ZKG_LPM = ZKG_SLAB / 16;                 // lanes that fetch one message's slab, 16 bytes each: 64 / ZKG_LPM messages per load instruction
static_assert(ZKG_SLAB == 128 || ZKG_SLAB == 256 || ZKG_SLAB == 512, "a slab is whole 64-byte blocks dealt to 8, 16 or 32 lanes");
constexpr uint32_t ZKG_ROW = ZKG_SLAB / 16 + 1;             // a message's row in LDS, in 16-byte slots: the slab and one slot of padding
constexpr uint32_t ZKG_WAVE_ROWS = 64 * ZKG_ROW;            // a wave's rows, in slots
constexpr uint32_t ZKG_WAVE_LDS = ZKG_WAVE_ROWS + 64;       // ... and behind them a slot per lane: where its message goes on, and how far
constexpr uint32_t ZKG_LEAF = 4096;                         // ZK_DIGEST_LEAF
constexpr uint32_t ZKG_BYTES = 32;                          // ZK_DIGEST_BYTES
constexpr uint32_t ZKG_GRID_MAX = 1u << 20;                 // workgroups: more lanes are strided over
constexpr uint32_t ZKG_DONE = 0xFFFFFFFFu;                  // zkg_stage: this lane's message wants nothing
enum { ZKG_SHA256 = 1, ZKG_BLAKE2S_TREE = 2 };              // ZK_DIGEST_*

ZK_HD uint64_t zkg_leaves(uint64_t len) { return len ? (len + ZKG_LEAF - 1) / ZKG_LEAF : 1; }
ZK_HD uint32_t zkg_blocks(uint64_t lanes)
{
    const uint64_t b = (lanes + ZKG_THREADS - 1) / ZKG_THREADS;
    return b > ZKG_GRID_MAX ? ZKG_GRID_MAX : (uint32_t)b;
}
// zk_archive_digests_dev: the pass of archive frames that begins with frame a ends before the returned one -- whole frames of at most pass_max
// decoded bytes in all, one at least (the passes of zk_dedup_index_add_archive_dev: zkd_slice_end).  off: the frames' decoded offsets
constexpr uint64_t ZKG_PASS_BYTES = 1ull << 30;             // ZK_CHOICE_DEDUP_PASS_KIB's default
ZK_HD uint32_t zkg_pass_end(const uint64_t *off, uint32_t a, uint32_t n, uint64_t pass_max)
{
    uint32_t b = a + 1;
    while (b < n && off[b + 1] - off[a] <= pass_max) b++;
    return b;
}
// The call's scratch, in bytes from its start: cnt[count] (uint64: the frames' leaves), lp[count + 1] (their prefix sums, the total behind
// them), leaves[32 * total].  SHA-256 needs none of it
struct ZkgLayout { size_t cnt, lp, leaves, end; };
ZK_HD ZkgLayout zkg_layout(uint32_t count, uint64_t total_leaves)
{
    ZkgLayout L;
    L.cnt = 0;
    L.lp = L.cnt + (size_t)count * 8;
    L.leaves = L.lp + ((size_t)count + 1) * 8;
    L.end = L.leaves + (size_t)total_leaves * ZKG_BYTES;
    return L;
}

// a rotate to the right: v_alignbit_b32 (the emulator header supplies the builtin; a host pass gets the funnel form)
#if defined(__HIP_DEVICE_COMPILE__) || defined(__builtin_amdgcn_alignbit)
#define ZKG_ROTR(x, n) __builtin_amdgcn_alignbit((x), (x), (n))
#else
#define ZKG_ROTR(x, n) (((x) >> (n)) | ((x) << (32 - (n))))
#endif

// ---------------------------------------------------------------- SHA-256 (FIPS 180-4)
static constexpr uint32_t ZKG_SHA_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
    0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
    0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
static constexpr uint32_t ZKG_IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};   // SHA-256's H(0) and BLAKE2s's IV

// one compression: w = the block's sixteen big-endian words
ZK_HD void zkg_sha256_block(uint32_t s[8], const uint32_t win[16])
{
    uint32_t w[16], v[8];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = win[i];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = s[i];
    // the eight working variables do not move: round i names them through (j - i) & 7, a compile-time index once the loop is unrolled
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t x = w[(i - 15) & 15], y = w[(i - 2) & 15];
            w[i & 15] += (ZKG_ROTR(x, 7) ^ ZKG_ROTR(x, 18) ^ (x >> 3)) + w[(i - 7) & 15] + (ZKG_ROTR(y, 17) ^ ZKG_ROTR(y, 19) ^ (y >> 10));
        }
        const uint32_t a = v[(0 - i) & 7], b = v[(1 - i) & 7], c = v[(2 - i) & 7], e = v[(4 - i) & 7], f = v[(5 - i) & 7], g = v[(6 - i) & 7];
        const uint32_t t1 = v[(7 - i) & 7] + (ZKG_ROTR(e, 6) ^ ZKG_ROTR(e, 11) ^ ZKG_ROTR(e, 25)) + ((e & f) ^ (~e & g)) + ZKG_SHA_K[i] + w[i & 15];
        v[(3 - i) & 7] += t1;
        v[(7 - i) & 7] = t1 + (ZKG_ROTR(a, 2) ^ ZKG_ROTR(a, 13) ^ ZKG_ROTR(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    }
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] += v[i];
}

// A message of len bytes as a chain: the caller hands zkg_sha256_step the next 64 bytes of  message | 0x80 | zeros  as big-endian words, block
// after block, until done.  The 64-bit bit length goes into the block that has room for it: the one that holds the 0x80 when fewer than 56
// bytes of it are the message's, else one more block of zeros (`extra`: the words handed over are not looked at then)
struct ZkgSha { uint32_t s[8]; uint64_t len, pos; bool extra, done; };
ZK_HD void zkg_sha256_init(ZkgSha &q, uint64_t len)
{
#pragma unroll
    for (int i = 0; i < 8; i++) q.s[i] = ZKG_IV[i];
    q.len = len; q.pos = 0; q.extra = false; q.done = false;
}
ZK_HD void zkg_sha256_step(ZkgSha &q, uint32_t w[16])
{
    const uint64_t rest = q.len - q.pos;
    if (q.extra) {
#pragma unroll
        for (int i = 0; i < 14; i++) w[i] = 0;
    }
    const bool fin = q.extra || rest < 56;
    if (fin) { w[14] = (uint32_t)(q.len >> 29); w[15] = (uint32_t)(q.len << 3); }
    zkg_sha256_block(q.s, w);
    if (fin) q.done = true;
    else if (rest < 64) { q.extra = true; q.pos = q.len; }
    else q.pos += 64;
}

// ---------------------------------------------------------------- BLAKE2s (RFC 7693) with the tree parameters of the BLAKE2 specification
#define ZKG_B2_G(a, b, c, d, x, y) do { \
        v[a] += v[b] + (x); v[d] = ZKG_ROTR(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = ZKG_ROTR(v[b] ^ v[c], 12); \
        v[a] += v[b] + (y); v[d] = ZKG_ROTR(v[d] ^ v[a], 8); v[c] += v[d]; v[b] = ZKG_ROTR(v[b] ^ v[c], 7); } while (0)
#define ZKG_B2_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) do { \
        ZKG_B2_G(0, 4, 8, 12, m[s0], m[s1]); ZKG_B2_G(1, 5, 9, 13, m[s2], m[s3]); ZKG_B2_G(2, 6, 10, 14, m[s4], m[s5]); ZKG_B2_G(3, 7, 11, 15, m[s6], m[s7]); \
        ZKG_B2_G(0, 5, 10, 15, m[s8], m[s9]); ZKG_B2_G(1, 6, 11, 12, m[s10], m[s11]); ZKG_B2_G(2, 7, 8, 13, m[s12], m[s13]); ZKG_B2_G(3, 4, 9, 14, m[s14], m[s15]); } while (0)

// one compression: m = the block's sixteen little-endian words, t = the bytes of the message up to and including this block
ZK_HD void zkg_blake2s_block(uint32_t h[8], const uint32_t m[16], uint64_t t, bool last, bool last_node)
{
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = ZKG_IV[i]; }
    v[12] ^= (uint32_t)t; v[13] ^= (uint32_t)(t >> 32);
    if (last) v[14] = ~v[14];
    if (last_node) v[15] = ~v[15];
    ZKG_B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    ZKG_B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    ZKG_B2_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    ZKG_B2_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    ZKG_B2_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    ZKG_B2_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    ZKG_B2_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    ZKG_B2_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    ZKG_B2_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    ZKG_B2_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

// A node of the tree as a chain: the caller hands zkg_blake2s_step the next 64 bytes of  message | zeros  as little-endian words until done.  A
// message that is a multiple of 64 bytes keeps its last block for the final flag; the empty message is one block of zeros
struct ZkgB2 { uint32_t h[8]; uint32_t len, pos; bool last_node, done; };
// digest length 32, no key, fanout 0, maximal depth 2, leaf length 4096, inner length 32; no salt, no personalisation
ZK_HD void zkg_blake2s_init(ZkgB2 &q, uint32_t len, uint64_t node_offset, uint32_t node_depth, bool last_node)
{
#pragma unroll
    for (int i = 0; i < 8; i++) q.h[i] = ZKG_IV[i];
    q.h[0] ^= 0x02000020u;
    q.h[1] ^= ZKG_LEAF;
    q.h[2] ^= (uint32_t)node_offset;
    q.h[3] ^= ((uint32_t)(node_offset >> 32) & 0xFFFFu) | (node_depth << 16) | (ZKG_BYTES << 24);
    q.len = len; q.pos = 0; q.last_node = last_node; q.done = false;
}
ZK_HD void zkg_blake2s_step(ZkgB2 &q, const uint32_t m[16])
{
    const bool fin = q.len - q.pos <= 64;
    q.pos = fin ? q.len : q.pos + 64;
    zkg_blake2s_block(q.h, m, q.pos, fin, fin && q.last_node);
    q.done = fin;
}

// ---------------------------------------------------------------- the slab
// sixteen bytes of a message at any alignment: one global_load_dwordx4, as the 16-byte loads of zk_k_dedup_hash
struct __attribute__((packed, aligned(1), may_alias)) ZkgPiece { uint32_t x, y, z, w; };
// Wave-wide (all 64 lanes call it): lane l's message goes on at src + at and has `avail` bytes there (at most ZKG_SLAB; ZKG_DONE: it wants
// nothing).  Row l of `rows` receives those bytes, the byte PAD behind them when they end inside the slab, and zeros up to the end of the
// 64-byte block that holds that byte.  Nothing outside src[at, at + avail) is loaded, but for `safe`: 16 bytes anywhere that may always be read
// (the kernels pass their offsets, which hold two words at least)
template <uint32_t PAD> __device__ __forceinline__ void zkg_stage(uint4 *rows, const uint8_t *src, const uint8_t *safe, uint64_t at, uint32_t avail, uint32_t lane)
{
    const uint32_t c = lane % ZKG_LPM, o = 16u * c, first = lane / ZKG_LPM;
    // every lane says where its message goes on, behind the rows; the sixteen lanes that fetch a message read it from there
    rows[ZKG_WAVE_ROWS + lane] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), avail, 0u);
    __builtin_amdgcn_wave_barrier();
    // the whole 16-byte pieces first, all of their loads in flight at once; then the piece that holds a message's end, byte by byte; then LDS
    ZkgPiece v[ZKG_LPM];
    uint64_t am[ZKG_LPM];
    uint32_t nm[ZKG_LPM];
#pragma unroll
    for (uint32_t it = 0; it < ZKG_LPM; it++) {
        const uint4 q = rows[ZKG_WAVE_ROWS + (64u / ZKG_LPM) * it + first];
        am[it] = (uint64_t)q.x | ((uint64_t)q.y << 32);
        nm[it] = q.z;
        // (no branch round the load: the lanes without a whole piece read `safe`, so that the wave's sixteen loads are issued back to back)
        const bool whole = nm[it] != ZKG_DONE && o + 16u <= nm[it];
        const ZkgPiece t = *(const ZkgPiece *)(whole ? src + am[it] + o : safe);
        v[it] = ZkgPiece{whole ? t.x : 0u, whole ? t.y : 0u, whole ? t.z : 0u, whole ? t.w : 0u};
    }
#pragma unroll
    for (uint32_t it = 0; it < ZKG_LPM; it++) {
        if (nm[it] == ZKG_DONE || nm[it] < o || nm[it] >= o + 16u) continue;
        const uint32_t nb = nm[it] - o;                     // 0 .. 15 bytes of the message, PAD behind them
        uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
        for (uint32_t k = 0; k <= nb; k++) {
            const uint32_t byte = (k < nb ? (uint32_t)src[am[it] + o + k] : PAD) << (8u * (k & 3u));
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) x[j] |= (k >> 2) == j ? byte : 0u;
        }
        v[it] = ZkgPiece{x[0], x[1], x[2], x[3]};
    }
#pragma unroll
    for (uint32_t it = 0; it < ZKG_LPM; it++)
        if (nm[it] != ZKG_DONE && o < ((nm[it] >> 6) + 1u) << 6) rows[((64u / ZKG_LPM) * it + first) * ZKG_ROW + c] = make_uint4(v[it].x, v[it].y, v[it].z, v[it].w);
}
#ifdef ZKG_DIRECT
// (measurement only) the straightforward loader: the lane's own block, four 16-byte loads at its own address -- 64 rows per wave instruction
template <uint32_t PAD> __device__ __forceinline__ void zkg_direct_block(const uint8_t *src, uint64_t at, uint64_t rest, uint32_t w[16])
{
    if (rest >= 64) {
#pragma unroll
        for (int i = 0; i < 4; i++) { const ZkgPiece t = *(const ZkgPiece *)(src + at + 16 * i); w[4 * i] = t.x; w[4 * i + 1] = t.y; w[4 * i + 2] = t.z; w[4 * i + 3] = t.w; }
        return;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = 0;
#pragma unroll 1
    for (uint32_t k = 0; k <= (uint32_t)rest; k++) {
        const uint32_t byte = (k < rest ? (uint32_t)src[at + k] : PAD) << (8u * (k & 3u));
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) w[j] |= (k >> 2) == j ? byte : 0u;
    }
}
#endif
// block b of this lane's row
__device__ __forceinline__ void zkg_row_block(const uint4 *rows, uint32_t lane, uint32_t b, uint32_t w[16])
{
    const uint4 *r = rows + lane * ZKG_ROW + 4u * b;
#pragma unroll
    for (int i = 0; i < 4; i++) { const uint4 q = r[i]; w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w; }
}

// Wave-wide.  `live` lanes: BLAKE2s of src[at, at + len) as the node (node_offset, node_depth, last_node) -> out[0 .. 8)
__device__ __forceinline__ void zkg_blake2s_wave(uint4 *rows, const uint8_t *src, const void *safe16, uint64_t at, uint32_t len, bool live, uint64_t node_offset, uint32_t node_depth,
                                                 bool last_node, uint32_t lane, uint32_t *out)
{
    const uint8_t *safe = (const uint8_t *)safe16;
    ZkgB2 q;
    zkg_blake2s_init(q, len, node_offset, node_depth, last_node);
    q.done = !live;
    while (__any(!q.done)) {
        const uint32_t left = q.len - q.pos;
#ifndef ZKG_DIRECT
        zkg_stage<0u>(rows, src, safe, at + q.pos, q.done ? ZKG_DONE : (left < ZKG_SLAB ? left : ZKG_SLAB), lane);
#else
        (void)left; (void)safe;
#endif
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (uint32_t b = 0; b < ZKG_SLAB / 64; b++) {
            if (q.done) break;
            uint32_t m[16];
#ifdef ZKG_DIRECT
            zkg_direct_block<0u>(src, at + q.pos, q.len - q.pos, m);
#else
            zkg_row_block(rows, lane, b, m);
#endif
            zkg_blake2s_step(q, m);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = q.h[i];
    }
}
// Wave-wide.  `live` lanes: SHA-256 of src[at, at + len) -> out[0 .. 8), the bytes in the order of the digest
__device__ __forceinline__ void zkg_sha256_wave(uint4 *rows, const uint8_t *src, const void *safe16, uint64_t at, uint64_t len, bool live, uint32_t lane, uint32_t *out)
{
    const uint8_t *safe = (const uint8_t *)safe16;
    ZkgSha q;
    zkg_sha256_init(q, len);
    q.done = !live;
    while (__any(!q.done)) {
        const uint64_t left = q.len - q.pos;
#ifndef ZKG_DIRECT
        zkg_stage<0x80u>(rows, src, safe, at + q.pos, q.done ? ZKG_DONE : (left < ZKG_SLAB ? (uint32_t)left : ZKG_SLAB), lane);
#else
        (void)left; (void)safe;
#endif
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (uint32_t b = 0; b < ZKG_SLAB / 64; b++) {
            if (q.done) break;
            uint32_t w[16];
#ifdef ZKG_DIRECT
            zkg_direct_block<0x80u>(src, at + q.pos, q.len - q.pos, w);
#else
            zkg_row_block(rows, lane, b, w);
#endif
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = __builtin_bswap32(w[i]);        // (a byte permute)
            zkg_sha256_step(q, w);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(q.s[i]);
    }
}

// ---------------------------------------------------------------- the kernels
// Frame i is src[off[i] - base, off[i + 1] - base): src points at the byte off[0] names, as for zk_k_dedup_hash.
__global__ __launch_bounds__(ZKG_THREADS) void zk_k_digest_counts(const uint64_t *off, uint32_t count, uint64_t *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * ZKG_THREADS + threadIdx.x;
    if (i < count) cnt[i] = zkg_leaves(off[i + 1] - off[i]);
}

// a lane per frame
__global__ __launch_bounds__(ZKG_THREADS) void zk_k_digest_sha256(const uint8_t *src, const uint64_t *off, uint64_t base, uint32_t count, uint32_t *digests)
{
    __shared__ uint4 lds[ZKG_WAVES * ZKG_WAVE_LDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint4 *rows = lds + (tid >> 6) * ZKG_WAVE_LDS;
    for (uint64_t g0 = (uint64_t)blockIdx.x * ZKG_THREADS; g0 < count; g0 += (uint64_t)gridDim.x * ZKG_THREADS) {
        const uint64_t i = g0 + tid;
        const bool live = i < count;
        const uint64_t at = live ? off[i] - base : 0, len = live ? off[i + 1] - off[i] : 0;
        zkg_sha256_wave(rows, src, off, at, len, live, lane, digests + 8 * (live ? i : 0));
    }
}

// a lane per leaf: lp[count + 1] are the prefix sums of the frames' leaf counts, total = lp[count]; leaf g's digest goes to leaves[8 g ...]
__global__ __launch_bounds__(ZKG_THREADS) void zk_k_digest_leaves(const uint8_t *src, const uint64_t *off, uint64_t base, uint32_t count, const uint64_t *lp,
                                                                  uint64_t total, uint32_t *leaves)
{
    __shared__ uint4 lds[ZKG_WAVES * ZKG_WAVE_LDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint4 *rows = lds + (tid >> 6) * ZKG_WAVE_LDS;
    for (uint64_t g0 = (uint64_t)blockIdx.x * ZKG_THREADS; g0 < total; g0 += (uint64_t)gridDim.x * ZKG_THREADS) {
        const uint64_t g = g0 + tid;
        const bool live = g < total;
        uint64_t at = 0, k = 0;
        uint32_t len = 0;
        bool last = false;
        if (live) {
            uint32_t f = 0, above = count;              // the frame with lp[f] <= g < lp[f + 1] (every frame has a leaf: lp ascends strictly)
            while (above - f > 1) { const uint32_t mid = f + ((above - f) >> 1); if (lp[mid] <= g) f = mid; else above = mid; }
            const uint64_t o0 = off[f], flen = off[f + 1] - o0;
            k = g - lp[f];
            last = g + 1 == lp[f + 1];
            at = o0 - base + k * ZKG_LEAF;
            len = (uint32_t)(flen - k * ZKG_LEAF < ZKG_LEAF ? flen - k * ZKG_LEAF : ZKG_LEAF);
        }
        zkg_blake2s_wave(rows, src, off, at, len, live, k, 0u, last, lane, leaves + 8 * (live ? g : 0));
    }
}

// a lane per frame: the root over the frame's leaf digests
__global__ __launch_bounds__(ZKG_THREADS) void zk_k_digest_roots(const uint32_t *leaves, const uint64_t *lp, uint32_t count, uint32_t *digests)
{
    __shared__ uint4 lds[ZKG_WAVES * ZKG_WAVE_LDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint4 *rows = lds + (tid >> 6) * ZKG_WAVE_LDS;
    for (uint64_t g0 = (uint64_t)blockIdx.x * ZKG_THREADS; g0 < count; g0 += (uint64_t)gridDim.x * ZKG_THREADS) {
        const uint64_t i = g0 + tid;
        const bool live = i < count;
        const uint64_t first = live ? lp[i] : 0, n = live ? lp[i + 1] - first : 0;
        zkg_blake2s_wave(rows, (const uint8_t *)leaves, lp, first * ZKG_BYTES, (uint32_t)(n * ZKG_BYTES), live, 0, 1u, true, lane, digests + 8 * (live ? i : 0));
    }
}

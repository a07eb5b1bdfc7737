// zk_dedup.h -- which frames of a list are byte-identical, decided on the device: the kernels of zk_dedup_frames[_dev] and the gather of
// zk_encode_dedup[_dev] (included by zk_dedup.hip, which keeps their launchers; tests/sim/zk_dedup_sim.cpp runs the same source on the CPU
// under the workgroup emulator, against the model of tests/helpers/dedup_model.py).  The rule (include/zeekstd_amd.h):
//   ref[i]    the smallest j <= i whose frame has the length and the bytes of frame i
//   uniq      the i with ref[i] == i, ascending;  ids[i] = the position of ref[i] in uniq
// The scheme, in ROUNDS over the frames that are still OPEN (all of them at first; a list of their indices from the second round on):
//   zk_k_dedup_hash         a 64-bit hash of every frame, made to be summed in any order: the frame is read as 8-byte words counted from its
//                           own first byte (zero-padded to 16), word w gives a term mixed from its value and w, and the hash is the sum of
//                           the terms' low halves beside the sum of their high halves, each mod 2^32 -- a workgroup per frame and piece of
//                           ZKD_PIECE bytes adds its lanes' share with 32-bit atomics.  (XXH64 is a serial chain per frame: 6.5 ms for
//                           411 frames of 2 MiB, where this pass runs at the speed of the memory.)  Once per call
//   key       that hash ^ the frame's length * an odd constant, cut to ZK_CHOICE_DEDUP_KEY_BITS bits (zkd_key)
//   zk_k_dedup_insert       a lane per open frame puts its index into an open-addressing table of 32-bit words (EMPTY, or the smallest open
//                           index of one key so far): compare-and-swap takes an empty slot, a slot that holds a frame of the same key is
//                           lowered with an atomic minimum, any other slot is passed by.  A slot's key is the key of whichever index it
//                           holds -- it never changes once the slot is taken -- so the table needs no key words.  slot[i] = where i went
//   zk_k_dedup_verify       (a launch of its own: the table is read with plain loads now) a lane per open frame: the leader is
//                           table[slot[i]].  The leader itself settles as ref = i.  Another length than the leader's: different.  At most
//                           ZKD_LANE_MAX bytes: compared by the lane.  Longer: put on the list of long compares
//   zk_k_dedup_verify_long  a workgroup per long compare and piece of ZKD_PIECE bytes (blockIdx.y strides the pieces): aligned 16-byte loads
//                           from the frame, unaligned ones from the leader, the bytes before the first 16-byte boundary and behind the last
//                           whole piece one by one; no load leaves the two frames.  A difference is an atomic OR into differ[item]
//   zk_k_dedup_settle_long  a lane per long compare: equal -> ref = leader, different -> open in the next round
//   A frame that differs from its leader stays open.  Every round settles the leader of every key (and all its copies), so the open
//   frames grow fewer until none is left; the leader of a round is the first frame of its content because frames of one content share a
//   key, hence a slot, and are all open or all settled (DESIGN.md 5k has the argument in full).
//   zk_k_dedup_flags / (zk_k_scan64) / zk_k_dedup_emit      uniq and ids
//   zk_k_dedup_gather       the bytes of uniq frames [k0, k0 + m) back to back (zk_encode_dedup*: a slice of whole frames for the list encoder)
// Every write to the table, the lists and the outputs is a vector store or a vector atomic.  Plain C++ only: no lane waits for another.
#pragma once
#include <stdint.h>
#include <string.h>
#include "zk_device.h"

// a look at a table word that other workgroups change in this launch: any value the word has held since the launch began will do
#ifndef ZKD_PEEK
#define ZKD_PEEK(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

constexpr uint32_t ZKD_THREADS = 256;
constexpr uint32_t ZKD_EMPTY = 0xFFFFFFFFu;                 // a free table slot; ref[] of a frame that is still open
constexpr uint32_t ZKD_LANE_MAX = 64;                       // frames up to this many bytes are compared by one lane
constexpr uint32_t ZKD_PIECE = 64u << 10;                   // bytes of a long compare (and of the gather) a workgroup takes at a time
constexpr uint32_t ZKD_PIECES_MAX = 256;                    // workgroups side by side on one frame
constexpr uint32_t ZKD_GRID_MAX = 1u << 22;                 // workgroups in x: a longer list is strided over
enum { ZKD_CNT_NEXT = 0, ZKD_CNT_LONG = 1, ZKD_CNT_WORDS = 4 };

ZK_HD uint64_t zkd_key(uint64_t hash, uint64_t len, uint32_t bits)
{
    const uint64_t k = hash ^ (len * 0x9E3779B97F4A7C15ull);
    return bits == 0 || bits >= 64 ? k : k & ((1ull << bits) - 1);
}
ZK_HD uint32_t zkd_home(uint64_t key, uint32_t mask) { return (uint32_t)((key * 0xD6E8FEB86659FD93ull) >> 32) & mask; }
// slots for `open` frames: a power of two, at least twice as many and at least 64
ZK_HD uint32_t zkd_slots(uint32_t open)
{
    uint32_t s = 64;
    while (s < 2ull * open) s <<= 1;
    return s;
}
ZK_HD uint32_t zkd_blocks(uint64_t items) { return (uint32_t)((items + ZKD_THREADS - 1) / ZKD_THREADS); }
// workgroups side by side on the pieces of one frame, from the list's longest
ZK_HD uint32_t zkd_pieces(uint64_t max_frame)
{
    const uint64_t p = (max_frame + ZKD_PIECE - 1) / ZKD_PIECE;
    return p < 1 ? 1 : p > ZKD_PIECES_MAX ? ZKD_PIECES_MAX : (uint32_t)p;
}
// zk_encode_dedup*: the slice of unique frames that begins with the k0-th ends before the returned one: whole frames of at most slice_max
// bytes in all, one at least.  len_of(k): the length of the k-th unique frame
template <class LenOf> ZK_HD uint32_t zkd_slice_end(uint32_t k0, uint32_t nu, uint64_t slice_max, LenOf len_of)
{
    uint64_t bytes = 0;
    uint32_t k = k0;
    for (; k < nu; k++) {
        const uint64_t len = len_of(k);
        if (k > k0 && bytes + len > slice_max) break;
        bytes += len;
    }
    return k;
}
// The scratch of one call for `count` frames, in bytes from its start (zk_dedup_core reserves it, the emulator harness allocates the same):
// hash[count] | flags[count + 1] | pos[count + 2] | ref | slot | list[2] | longl | differ | uniq | ids (count each) | cnt[4] | table[zkd_slots(count)]
struct ZkDedupLayout { size_t hash, flags, pos, ref, slot, list[2], longl, differ, uniq, ids, cnt, table, end; };
ZK_HD ZkDedupLayout zkd_layout(uint32_t count)
{
    ZkDedupLayout L;
    const size_t c = count, q = (4 * c + 15) & ~(size_t)15;
    L.hash = 0;
    L.flags = L.hash + 8 * c;
    L.pos = L.flags + 8 * (c + 1);
    L.ref = (L.pos + 8 * (c + 2) + 15) & ~(size_t)15;
    L.slot = L.ref + q; L.list[0] = L.slot + q; L.list[1] = L.list[0] + q; L.longl = L.list[1] + q; L.differ = L.longl + q;
    L.uniq = L.differ + q; L.ids = L.uniq + q; L.cnt = L.ids + q;
    L.table = L.cnt + 16;
    L.end = L.table + 4 * (size_t)zkd_slots(count);
    return L;
}

// the frames: frame i is src[off[i] - off[0], off[i + 1] - off[0]) -- src points at the byte off[0] names
struct ZkDedupIn { const uint8_t *src; const uint64_t *off; uint64_t base; const uint64_t *hash; uint32_t bits; };
// one round: its open frames (list == nullptr: frames 0 .. nopen - 1), the table of mask + 1 slots
struct ZkDedupRound { const uint32_t *list; uint32_t nopen, mask; };

// the term of the 8 bytes v that are word w of their frame
ZK_HD uint64_t zkd_term(uint64_t v, uint64_t w)
{
    uint64_t x = v + (w + 1) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}
// hash32: the frames' hashes as pairs of 32-bit sums (low word first), zero before the launch.  Workgroup (i, y) takes the pieces y, y +
// gridDim.y, ... of frame i; 16 bytes per lane and step at any alignment, the last 1..15 bytes of a frame one by one: no load leaves a frame
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_hash(const uint8_t *src, const uint64_t *off, uint64_t base, uint32_t count, uint32_t *hash32)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint64_t len = off[i + 1] - off[i];
        const uint8_t *x = src + (off[i] - base);
        uint32_t lo = 0, hi = 0;
        for (uint64_t p0 = (uint64_t)blockIdx.y * ZKD_PIECE; p0 < len; p0 += (uint64_t)gridDim.y * ZKD_PIECE) {
            const uint32_t n = (uint32_t)(len - p0 < ZKD_PIECE ? len - p0 : ZKD_PIECE), nq = n >> 4;
            for (uint32_t q = tid; q < nq; q += ZKD_THREADS) {
                uint64_t v[2];
                memcpy(v, x + p0 + 16 * (size_t)q, 16);
                const uint64_t w = (p0 >> 3) + 2 * (uint64_t)q, s = zkd_term(v[0], w), t = zkd_term(v[1], w + 1);
                lo += (uint32_t)s + (uint32_t)t; hi += (uint32_t)(s >> 32) + (uint32_t)(t >> 32);
            }
            if (tid == 0 && (n & 15u)) {
                // the frame's last 1..15 bytes, zero-padded to one more piece of 16
                uint64_t v[2] = {0, 0};
                for (uint32_t k = 0; k < (n & 15u); k++) v[k >> 3] |= (uint64_t)x[p0 + 16 * (size_t)nq + k] << (8 * (k & 7u));
                const uint64_t w = (p0 >> 3) + 2 * (uint64_t)nq, s = zkd_term(v[0], w), t = zkd_term(v[1], w + 1);
                lo += (uint32_t)s + (uint32_t)t; hi += (uint32_t)(s >> 32) + (uint32_t)(t >> 32);
            }
        }
        if (lo | hi) { atomicAdd(hash32 + 2 * (size_t)i, lo); atomicAdd(hash32 + 2 * (size_t)i + 1, hi); }
    }
}

__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_insert(ZkDedupIn a, ZkDedupRound r, uint32_t *table, uint32_t *slot)
{
    const uint32_t t = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (t >= r.nopen) return;
    const uint32_t i = r.list ? r.list[t] : t;
    const uint64_t key = zkd_key(a.hash[i], a.off[i + 1] - a.off[i], a.bits);
    uint32_t s = zkd_home(key, r.mask);
    for (;;) {
        uint32_t old = ZKD_PEEK(table + s);
        if (old == ZKD_EMPTY) old = atomicCAS(table + s, ZKD_EMPTY, i);
        if (old == ZKD_EMPTY) break;                                             // taken: i leads the slot for now
        if (old == i || zkd_key(a.hash[old], a.off[old + 1] - a.off[old], a.bits) == key) {
            // the slot of this key: the word only falls, so a smaller index seen there (however old the look) means i cannot lead
            if (i < old) atomicMin(table + s, i);
            break;
        }
        s = (s + 1) & r.mask;
    }
    slot[i] = s;
}

__device__ __forceinline__ bool zkd_lane_equal(const uint8_t *x, const uint8_t *y, uint32_t n)
{
    uint32_t k = 0;
    for (; k + 8 <= n; k += 8) {
        uint64_t u, v;
        memcpy(&u, x + k, 8); memcpy(&v, y + k, 8);
        if (u != v) return false;
    }
    for (; k < n; k++) if (x[k] != y[k]) return false;
    return true;
}

// next / longl / differ are written at places drawn from cnt[ZKD_CNT_NEXT] / cnt[ZKD_CNT_LONG] (zero before the launch)
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_verify(ZkDedupIn a, ZkDedupRound r, const uint32_t *table, const uint32_t *slot, uint32_t *ref,
                                                                 uint32_t *next, uint32_t *longl, uint32_t *differ, uint32_t *cnt)
{
    const uint32_t t = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (t >= r.nopen) return;
    const uint32_t i = r.list ? r.list[t] : t;
    const uint32_t lead = table[slot[i]];
    if (lead == i) { ref[i] = i; return; }
    const uint64_t at = a.off[i] - a.base, len = a.off[i + 1] - a.off[i], lat = a.off[lead] - a.base, llen = a.off[lead + 1] - a.off[lead];
    bool equal = len == llen;
    if (equal && len > ZKD_LANE_MAX) {
        const uint32_t p = atomicAdd(cnt + ZKD_CNT_LONG, 1u);
        longl[p] = i; differ[p] = 0;
        return;
    }
    if (equal) equal = zkd_lane_equal(a.src + at, a.src + lat, (uint32_t)len);
    if (equal) ref[i] = lead;
    else next[atomicAdd(cnt + ZKD_CNT_NEXT, 1u)] = i;
}

// does [x, x + n) differ from [y, y + n)?  The lanes of a workgroup side by side; every load lies inside the two ranges
__device__ __forceinline__ bool zkd_wg_differ(const uint8_t *x, const uint8_t *y, uint32_t n, uint32_t tid)
{
    const uint32_t to16 = (16u - (uint32_t)((uintptr_t)x & 15u)) & 15u, head = to16 < n ? to16 : n;
    const uint32_t nq = (n - head) >> 4, tail = head + 16 * nq;
    bool d = false;
    if (tid < head) d = x[tid] != y[tid];
    for (uint32_t q = tid; q < nq; q += ZKD_THREADS) {
        const uint4 u = *(const uint4 *)(x + head + 16 * (size_t)q);             // aligned
        uint4 v;
        memcpy(&v, y + head + 16 * (size_t)q, 16);                               // any alignment
        d |= ((u.x ^ v.x) | (u.y ^ v.y) | (u.z ^ v.z) | (u.w ^ v.w)) != 0;
    }
    if (tail + tid < n) d |= x[tail + tid] != y[tail + tid];
    return d;
}

__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_verify_long(ZkDedupIn a, const uint32_t *table, const uint32_t *slot, const uint32_t *longl,
                                                                      uint32_t nlong, uint32_t *differ)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t item = blockIdx.x; item < nlong; item += gridDim.x) {
        const uint32_t i = longl[item], lead = table[slot[i]];
        const uint64_t len = a.off[i + 1] - a.off[i];
        const uint8_t *x = a.src + (a.off[i] - a.base), *y = a.src + (a.off[lead] - a.base);
        bool d = false;
        for (uint64_t p0 = (uint64_t)blockIdx.y * ZKD_PIECE; p0 < len; p0 += (uint64_t)gridDim.y * ZKD_PIECE)
            d |= zkd_wg_differ(x + p0, y + p0, (uint32_t)(len - p0 < ZKD_PIECE ? len - p0 : ZKD_PIECE), tid);
        if (d) atomicOr(differ + item, 1u);
    }
}

__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_settle_long(const uint32_t *table, const uint32_t *slot, const uint32_t *longl, uint32_t nlong,
                                                                      const uint32_t *differ, uint32_t *ref, uint32_t *next, uint32_t *cnt)
{
    const uint32_t t = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (t >= nlong) return;
    const uint32_t i = longl[t];
    if (differ[t]) next[atomicAdd(cnt + ZKD_CNT_NEXT, 1u)] = i;
    else ref[i] = table[slot[i]];
}

// flags[i] = frame i is the first of its content; flags[count] = 0, so that the scan of count + 1 values leaves pos[count] = n_unique
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_flags(const uint32_t *ref, uint32_t count, uint64_t *flags)
{
    const uint32_t i = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (i <= count) flags[i] = i < count && ref[i] == i;
}
// pos: the exclusive scan of the flags.  uniq / ids may be null
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_emit(const uint32_t *ref, uint32_t count, const uint64_t *pos, uint32_t *uniq, uint32_t *ids)
{
    const uint32_t i = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t j = ref[i];
    if (uniq && j == i) uniq[pos[i]] = i;
    if (ids) ids[i] = (uint32_t)pos[j];
}

// dst[goff[k] - goff[0] ...] = frame uniq[k], k < m: workgroup (k, y) takes the pieces y, y + gridDim.y, ... of frame k.  16 bytes per lane and
// step at any alignment on both sides, the last bytes one by one; nothing is read outside a frame or written outside its place
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dedup_gather(const uint8_t *src, const uint64_t *off, uint64_t base, const uint32_t *uniq, uint32_t m,
                                                                 const uint64_t *goff, uint8_t *dst)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < m; k += gridDim.x) {
        const uint32_t i = uniq[k];
        const uint64_t len = off[i + 1] - off[i];
        const uint8_t *from = src + (off[i] - base);
        uint8_t *to = dst + (goff[k] - goff[0]);
        for (uint64_t p0 = (uint64_t)blockIdx.y * ZKD_PIECE; p0 < len; p0 += (uint64_t)gridDim.y * ZKD_PIECE) {
            const uint32_t n = (uint32_t)(len - p0 < ZKD_PIECE ? len - p0 : ZKD_PIECE), nq = n >> 4;
            for (uint32_t q = tid; q < nq; q += ZKD_THREADS) {
                uint4 v;
                memcpy(&v, from + p0 + 16 * (size_t)q, 16);
                memcpy(to + p0 + 16 * (size_t)q, &v, 16);
            }
            if (16 * nq + tid < n) to[p0 + 16 * nq + tid] = from[p0 + 16 * nq + tid];
        }
    }
}

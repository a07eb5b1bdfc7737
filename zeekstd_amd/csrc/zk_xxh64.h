// zk_xxh64.h -- the XXH64 kernels of the decoder: the passes behind the executor (zk_k_xxh64, _wide, _lean, _fed) and the followers
// beside it (zk_k_xxh64_follow, _follow1).  hipcc compiles them as part of zk_decode.hip, which includes this file where they stood;
// g++ compiles the same text under tests/sim/hip_wg_emu.h (tests/sim/zk_xxh_sim.cpp), workgroup after workgroup on the CPU.  What has
// no meaning there stands behind hooks the includer may define first (as ZKE_WALK / ZKE_FFBL in zk_enc_match.h):
//   ZKX_XCC_ID()      the XCD this wave runs on (zk_progress.h)
//   ZKX_CLOCK()       wall_clock64
//   ZKX_SLEEP(n)      s_sleep: the one place in a polling loop where the whole wave meets and time passes
//   ZKX_ACQUIRE()     the agent-scope acquire fence between a progress word and the loads of the bytes it announces
//   ZKX_PROG_LOAD(p)  the relaxed agent-scope load of a progress word
#pragma once
#include "zk_device.h"
#include "zk_progress.h"
#ifndef ZKX_CLOCK
#define ZKX_CLOCK() wall_clock64()
#endif
#ifndef ZKX_SLEEP
#define ZKX_SLEEP(n) __builtin_amdgcn_s_sleep(n)
#endif
#ifndef ZKX_ACQUIRE
#define ZKX_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#endif
#ifndef ZKX_PROG_LOAD
#define ZKX_PROG_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

// ------------------------------------------------------------------------------------------------ XXH64
// hashes != nullptr -> store the 64-bit hash; infos != nullptr -> verify Content_Checksum.
// rotl by 1 ... 31 as two v_alignbit_b32 (the compiler's form: a 64-bit shift, a 32-bit one and an or -- three instructions of a chain on
// which every instruction is ~8 clocks of a lone wave, the 64-bit shift more)
__device__ __forceinline__ uint64_t zk_rotl64(uint64_t x, int r)
{
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    return ((uint64_t)__builtin_amdgcn_alignbit(hi, lo, 32u - (uint32_t)r) << 32) | __builtin_amdgcn_alignbit(lo, hi, 32u - (uint32_t)r);
}
constexpr uint64_t XP1 = 0x9E3779B185EBCA87ull, XP2 = 0xC2B2AE3D27D4EB4Full, XP3 = 0x165667B19E3779F9ull,
                   XP4 = 0x85EBCA77C2B2AE63ull, XP5 = 0x27D4EB2F165667C5ull;
__device__ __forceinline__ uint64_t zk_xround(uint64_t acc, uint64_t x) { return zk_rotl64(acc + x * XP2, 31) * XP1; }
// accumulator kl (0..3) before the first stripe.  (A macro: as an inlined function the same expression changes the register allocation of
// the double-batch loops -- zk_k_xxh64_lean 68 -> 72 bytes of scratch, zk_k_xxh64_follow 64 -> 61 registers, zk_k_xxh64_wide and _fed rescheduled)
#define ZK_XXH64_SEED(kl) ((kl) == 0 ? XP1 + XP2 : (kl) == 1 ? XP2 : (kl) == 2 ? 0 : 0 - XP1)
// the hash of a frame from its four accumulators behind the last whole stripe: their merge, the tail of len % 32 bytes (8, 4, 1 at a
// time) and the avalanche.  Once per frame, in one lane; every XXH64 kernel below ends here.
__device__ __forceinline__ uint64_t zk_xxh64_finish(uint64_t v1, uint64_t v2, uint64_t v3, uint64_t v4, const uint8_t *p, uint64_t len, uint64_t nstripes)
{
    uint64_t h;
    if (len >= 32) {
        h = zk_rotl64(v1, 1) + zk_rotl64(v2, 7) + zk_rotl64(v3, 12) + zk_rotl64(v4, 18);
        h = (h ^ zk_xround(0, v1)) * XP1 + XP4;
        h = (h ^ zk_xround(0, v2)) * XP1 + XP4;
        h = (h ^ zk_xround(0, v3)) * XP1 + XP4;
        h = (h ^ zk_xround(0, v4)) * XP1 + XP4;
    } else h = XP5;
    h += len;
    const uint8_t *t = p + (nstripes << 5), *end = p + len;
    while (t + 8 <= end) { h ^= zk_xround(0, zk_ld64(t)); h = zk_rotl64(h, 27) * XP1 + XP4; t += 8; }
    if (t + 4 <= end) { h ^= (uint64_t)zk_rd32(t) * XP1; h = zk_rotl64(h, 23) * XP2 + XP3; t += 4; }
    while (t < end) { h ^= (uint64_t)(*t) * XP5; h = zk_rotl64(h, 11) * XP1; t++; }
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return h;
}
// Sixteen frames per wave, lane = (frame f, accumulator): which frame is this lane's, and where the wave's frames stop having stripes
// in common.  live: f is in range, checksummed and OK (infos may be null: hash everything), and not already verified by zk_k_xxh64_follow
// (skip may be null).  least: the fewest stripes of a live frame among the wave's lanes, ~0 when the wave has no frame to hash.
struct ZkXxhLane { bool live; const uint8_t *p; uint64_t len, nstripes, least; };
__device__ __forceinline__ ZkXxhLane zk_xxh64_lane(bool in_range, uint32_t f, const uint8_t *data, const uint64_t *d_off, uint32_t first,
                                                   const ZkFrameInfo *infos, const uint64_t *skip)
{
    ZkXxhLane x;
    x.live = in_range;
    if (x.live && infos && !(infos[f].status == ZK_OK && infos[f].checksum_flag)) x.live = false;
    if (x.live && skip && (skip[f] & ZK_PROG_VERIFIED)) x.live = false;
    const uint32_t fa = x.live ? f : 0;                     // (a lane without a frame reads frame 0 and keeps nothing)
    x.p = data + (d_off[first + fa] - d_off[first]);
    x.len = d_off[first + fa + 1] - d_off[first + fa];
    x.nstripes = x.live ? x.len >> 5 : 0;
    x.least = x.live ? x.nstripes : ~0ull;
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) { const uint64_t o = __shfl_xor(x.least, m, 64); x.least = o < x.least ? o : x.least; }
    return x;
}

// One wave per frame.  All 64 lanes stream the frame in 1 KiB chunks (coalesced 16 B loads, one chunk
// in flight ahead) and pre-multiply every word by P2; the products go through LDS to lanes 0-3, which
// run the four serial accumulator chains acc = rotl(acc + x*P2, 31) * P1.
__global__ __launch_bounds__(64) void zk_k_xxh64(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                 ZkFrameInfo *infos, uint64_t *hashes)
{
    __shared__ uint64_t prod[128];
    const uint32_t lane = threadIdx.x, f = blockIdx.x;
    if (infos && !(infos[f].status == ZK_OK && infos[f].checksum_flag)) return;
    const uint8_t *p = data + (d_off[first + f] - d_off[first]);
    const uint64_t len = d_off[first + f + 1] - d_off[first + f];
    const uint64_t nchunks = len >> 10;
    // lanes 4..15 shadow lanes 0..3: a wave with < 16 active lanes runs ~3x slower on gfx950 (tools/ubench/lat3.hip)
    const uint32_t kl = lane & 3;
    uint64_t acc = ZK_XXH64_SEED(kl);
    const bool aligned = (((uintptr_t)p) & 15) == 0;
    uint64_t a = 0, b = 0;
    auto ldpair = [&](uint64_t c) {
        const uint8_t *q = p + (c << 10) + lane * 16;
        if (aligned) { uint4 v = *reinterpret_cast<const uint4 *>(q); a = v.x | ((uint64_t)v.y << 32); b = v.z | ((uint64_t)v.w << 32); }
        else { a = zk_ld64(q); b = zk_ld64(q + 8); }
    };
    if (nchunks) ldpair(0);
    for (uint64_t c = 0; c < nchunks; c++) {
        prod[2 * lane] = a * XP2; prod[2 * lane + 1] = b * XP2;
        if (c + 1 < nchunks) ldpair(c + 1);
        __syncthreads();
        if (lane < 16) {
#pragma unroll 8
            for (int r = 0; r < 32; r++) acc = zk_rotl64(acc + prod[4 * r + kl], 31) * XP1;
        }
        __syncthreads();
    }
    // remaining whole stripes (< 32 of them), straight from memory
    const uint64_t nstripes = len >> 5;
    if (lane < 16) for (uint64_t i = nchunks << 5; i < nstripes; i++) acc = zk_xround(acc, zk_ld64(p + (i << 5) + 8 * kl));
    uint64_t v1 = __shfl(acc, 0, 64), v2 = __shfl(acc, 1, 64), v3 = __shfl(acc, 2, 64), v4 = __shfl(acc, 3, 64);
    if (lane != 0) return;
    const uint64_t h = zk_xxh64_finish(v1, v2, v3, v4, p, len, nstripes);
    if (hashes) hashes[f] = h;
    if (infos && (uint32_t)h != infos[f].checksum) infos[f].status = ZK_E_CHECKSUM_WRONG;
}

// The same for a large batch: SIXTEEN frames per wave, lane = (frame, accumulator).  A frame's four chains are a latency floor
// (65 536 dependent rounds per 2 MiB, ~110 clocks each) whatever runs them; one wave per frame spends a whole wave's instruction
// slots on 4 (16) lanes -- 1.7 G wave instructions per 4 GiB, a twelfth of what the encoder's matcher issues, and whichever kernel
// runs beside the checksums pays for them (the entropy stage: 6.3 -> 7.6 ms).  Here the same chains cost a sixteenth of that:
// 128 waves for 2048 frames, a lane loading its own 8 bytes of every stripe, 24 stripes per batch, two batches under way.
// (Its own frame selection and tail, not zk_xxh64_lane / zk_xxh64_finish, and zk_fse_share_pick its own keys: with the helpers this kernel's
// epilogue and zk_k_fse_predef_fed's prologue and feeder set-up were compiled differently, and a generated-frames decode through those two
// kernels ended once in a HIP queue error on the device whose cause was not found.  Both keep the code object they had, byte for byte,
// until it is: profiles/r10_fold_kdiff.txt.)
constexpr int ZK_XXW = 24;
__global__ __launch_bounds__(64) void zk_k_xxh64_wide(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                      ZkFrameInfo *infos, uint64_t *hashes, const uint64_t *skip)
{
    const uint32_t lane = threadIdx.x, f = blockIdx.x * 16 + (lane >> 2), kl = lane & 3;
    bool live = f < count;
    if (live && infos && !(infos[f].status == ZK_OK && infos[f].checksum_flag)) live = false;
    if (live && skip && (skip[f] & ZK_PROG_VERIFIED)) live = false;       // zk_k_xxh64_follow has verified this frame
    const uint32_t fa = live ? f : 0;                       // (a lane without a frame reads frame 0 and keeps nothing)
    const uint8_t *p = data + (d_off[first + fa] - d_off[first]);
    const uint64_t len = d_off[first + fa + 1] - d_off[first + fa];
    const uint64_t nstripes = live ? len >> 5 : 0;
    uint64_t acc = kl == 0 ? XP1 + XP2 : kl == 1 ? XP2 : kl == 2 ? 0 : 0 - XP1;
    // the stripes every live frame of the wave has, in whole double batches: no predicates
    uint64_t least = live ? nstripes : ~0ull;
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) { const uint64_t o = __shfl_xor(least, m, 64); least = o < least ? o : least; }
    if (least == ~0ull) return;                             // no frame to hash in this wave
    const uint64_t common = least - least % (2 * ZK_XXW);
    const uint8_t *q = p + 8 * kl;
    uint64_t wa[ZK_XXW], wb[ZK_XXW];
    if (common) {
#pragma unroll
        for (int u = 0; u < ZK_XXW; u++) wa[u] = zk_ld64(q + 32 * (uint64_t)u);
        for (uint64_t s = 0; s < common; s += 2 * ZK_XXW) {
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) wb[u] = zk_ld64(q + 32 * (s + ZK_XXW + u));
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) acc = zk_xround(acc, wa[u]);
            const uint64_t nx = s + 2 * ZK_XXW < common ? s + 2 * ZK_XXW : 0;     // (the last round reads the frame's first batch again)
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) wa[u] = zk_ld64(q + 32 * (nx + u));
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) acc = zk_xround(acc, wb[u]);
        }
    }
    // what is left of the longer frames, stripe by stripe
    for (uint64_t i = common; i < nstripes; i++) acc = zk_xround(acc, zk_ld64(q + (i << 5)));
    const uint32_t base = lane & ~3u;
    const uint64_t v1 = __shfl(acc, base, 64), v2 = __shfl(acc, base + 1, 64), v3 = __shfl(acc, base + 2, 64), v4 = __shfl(acc, base + 3, 64);
    if (kl != 0 || !live) return;
    uint64_t h;
    if (len >= 32) {
        h = zk_rotl64(v1, 1) + zk_rotl64(v2, 7) + zk_rotl64(v3, 12) + zk_rotl64(v4, 18);
        h = (h ^ zk_xround(0, v1)) * XP1 + XP4;
        h = (h ^ zk_xround(0, v2)) * XP1 + XP4;
        h = (h ^ zk_xround(0, v3)) * XP1 + XP4;
        h = (h ^ zk_xround(0, v4)) * XP1 + XP4;
    } else h = XP5;
    h += len;
    const uint8_t *t = p + (nstripes << 5), *end = p + len;
    while (t + 8 <= end) { h ^= zk_xround(0, zk_ld64(t)); h = zk_rotl64(h, 27) * XP1 + XP4; t += 8; }
    if (t + 4 <= end) { h ^= (uint64_t)zk_rd32(t) * XP1; h = zk_rotl64(h, 23) * XP2 + XP3; t += 4; }
    while (t < end) { h ^= (uint64_t)(*t) * XP5; h = zk_rotl64(h, 11) * XP1; t++; }
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    if (hashes) hashes[f] = h;
    if (infos && (uint32_t)h != infos[f].checksum) infos[f].status = ZK_E_CHECKSUM_WRONG;
}

// A WAVE THAT ONLY RUNS THE CHAINS, FED BY ANOTHER (r6).  zk_k_xxh64_wide's wave does everything for its 64 chains: per round the load,
// the product x * P2 (four instructions) and the chain's own six -- of one wave, all 64 lanes at work: an instruction is four passes of the
// SIMD, a 32-bit multiply sixteen clocks: ~100 clocks per round, 2.7 ms per 2 MiB frame, during which the device is all but idle (128
// waves) and the decode waits (the step's stages run one after the other).  Here wave 0 runs the chains and nothing else -- a product out
// of LDS, mad + two mul_lo + add3, two alignbit -- in SIXTEEN lanes (NF = 4 frames per workgroup): one pass of the SIMD per instruction
// instead of four.  Wave 1 brings the products a chunk of 32 stripes ahead: 16-byte loads (lane l: words 2l and 2l + 1 of the frame's
// next KiB), D chunks of every frame under way, two products per lane, one 16-byte LDS write -- rows of NF x 32 bytes + 32 bytes of
// padding, so that eight lanes' writes (four rows) fall into eight groups of banks.  One barrier per chunk: behind barrier k the chains
// take buffer k & 1 while the producer fills the other one.
//   Measured (2048 x 2 MiB, tools/gpu_calls/r6am.sh ... r6an.sh): wide 2.72 ms (2.52 with the rotations as two alignbit), 64 chains fed by
// two waves 2.96 (the chains' instructions still take four passes), 16 chains fed by one wave with two chunks under way 2.36 (the chains
// wait for memory at the barrier), with six: 1.65 ms.
constexpr int ZK_XF_CHUNK = 32;
constexpr int zk_xf_depth(int nf) { return nf == 4 ? 6 : 2; }       // chunks of every frame a producer wave has under way (D below)
template <int NF>                                            // frames per workgroup: 4 (16 chains: one of the SIMD's four passes per instruction)
__global__ __launch_bounds__(64 * (1 + (NF >= 8 ? NF / 8 : 1))) void zk_k_xxh64_fed(const uint8_t *__restrict__ data, const uint64_t *__restrict__ d_off, uint32_t first, uint32_t count,
                                                      ZkFrameInfo *infos, uint64_t *hashes, const uint64_t *skip)
{
    constexpr int PF = NF >= 8 ? 8 : NF;                     // frames per producer wave
    constexpr int ZK_XF_ROW = NF * 32 + 32;
    __shared__ __attribute__((aligned(16))) uint8_t ring[2][ZK_XF_CHUNK * ZK_XF_ROW];
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t f = blockIdx.x * NF + (lane >> 2), kl = lane & 3;
    const ZkXxhLane x = zk_xxh64_lane(lane < 4 * NF && f < count, f, data, d_off, first, infos, skip);
    bool ragged = (((uintptr_t)x.p) & 15) != 0;
    if (x.least == ~0ull) return;                           // no frame to hash in this workgroup (every wave finds the same)
    const bool any_ragged = __any(ragged);
    const uint64_t nchunks = x.least / ZK_XF_CHUNK;          // the chunks every live frame of the group has
    if (wave != 0) {
        // producers: frames PF (wave - 1) ... of the group; the frame's pointer sits in lane 4 j of the consumer's layout
        const uint32_t j0 = PF * (wave - 1);
        const uint8_t *pj[PF];
#pragma unroll
        for (int j = 0; j < PF; j++) {
            const uint64_t a = (uint64_t)(uintptr_t)x.p;
            pj[j] = (const uint8_t *)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(a >> 32), 4 * (int)(j0 + j)) << 32) |
                                                 (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)a, 4 * (int)(j0 + j)));
        }
        // D chunks of every frame under way (a chunk of the chains is ~0.8 us, a load from memory two or three times that; D = 2 left the
        // chains waiting at the barrier: 2.36 ms per 2 MiB frame with four frames per workgroup)
        constexpr int D = zk_xf_depth(NF);
        uint64_t wa[D][PF], wb[D][PF];
        auto load = [&](uint64_t c, uint64_t *xa, uint64_t *xb) {
#pragma unroll
            for (int j = 0; j < PF; j++) {
                const uint8_t *q = pj[j] + (c << 10) + lane * 16;
                if (!any_ragged) { const uint4 v = *reinterpret_cast<const uint4 *>(q); xa[j] = v.x | ((uint64_t)v.y << 32); xb[j] = v.z | ((uint64_t)v.w << 32); }
                else { xa[j] = zk_ld64(q); xb[j] = zk_ld64(q + 8); }
            }
        };
        auto fill = [&](uint32_t buf, const uint64_t *xa, const uint64_t *xb) {
            uint8_t *row = ring[buf] + (lane >> 1) * ZK_XF_ROW + j0 * 32 + (lane & 1) * 16;
#pragma unroll
            for (int j = 0; j < PF; j++) {
                const uint64_t pa = xa[j] * XP2, pb = xb[j] * XP2;
                *reinterpret_cast<uint4 *>(row + j * 32) = make_uint4((uint32_t)pa, (uint32_t)(pa >> 32), (uint32_t)pb, (uint32_t)(pb >> 32));
            }
        };
        // chunk c lives in registers [c % D]; before barrier k the buffer k & 1 holds chunk k, behind it chunk k + 1 is written
#pragma unroll
        for (int d = 0; d < D; d++) if ((uint64_t)d < nchunks) load(d, wa[d], wb[d]);
        if (nchunks) fill(0, wa[0], wb[0]);
        for (uint64_t k0 = 0; k0 < nchunks; k0 += D) {
#pragma unroll
            for (int d = 0; d < D; d++) {
                const uint64_t k = k0 + d;
                if (k < nchunks) {
                    __syncthreads();
                    if (k + D < nchunks) load(k + D, wa[d], wb[d]);              // (chunk k's registers are free: it went into the ring before this barrier)
                    if (k + 1 < nchunks) fill((uint32_t)(k + 1) & 1u, wa[(d + 1) % D], wb[(d + 1) % D]);
                }
            }
        }
        return;
    }
    // the chains
    uint64_t acc = ZK_XXH64_SEED(kl);
    for (uint64_t k = 0; k < nchunks; k++) {
        __syncthreads();
        if (lane < 4 * NF) {                                 // (NF = 4: sixteen lanes at work -- an instruction of the chain takes one pass of the SIMD, not four)
            const uint8_t *row = ring[k & 1] + lane * 8;
#pragma unroll 8
            for (int r = 0; r < ZK_XF_CHUNK; r++) acc = zk_rotl64(acc + *reinterpret_cast<const uint64_t *>(row + r * ZK_XF_ROW), 31) * XP1;
        }
    }
    // what is left of the longer frames, stripe by stripe
    const uint8_t *q = x.p + 8 * kl;
    for (uint64_t i = nchunks * ZK_XF_CHUNK; i < x.nstripes; i++) acc = zk_xround(acc, zk_ld64(q + (i << 5)));
    const uint32_t base = lane & ~3u;
    const uint64_t v1 = __shfl(acc, base, 64), v2 = __shfl(acc, base + 1, 64), v3 = __shfl(acc, base + 2, 64), v4 = __shfl(acc, base + 3, 64);
    if (kl != 0 || !x.live) return;
    const uint64_t h = zk_xxh64_finish(v1, v2, v3, v4, x.p, x.len, x.nstripes);
    if (hashes) hashes[f] = h;
    if (infos && (uint32_t)h != infos[f].checksum) infos[f].status = ZK_E_CHECKSUM_WRONG;
}

// The same in 64 registers (12 stripes per batch under waves_per_eu(8); zk_k_xxh64_wide takes 78): what is left on a SIMD beside four
// executor waves of 112, so that the checksums of one batch can run while the executor of the next batch in flight holds the CUs --
// with 78 the checksum waves of batch A wait until executor workgroups of batch B retire.  (A template only for this kernel.  The two
// double-batch loops stay two: zk_k_xxh64_wide as zk_xxh64_lean_body<24> with `skip` takes 121 registers instead of its 78 -- measured
// again with the frame selection and the tail shared, which is all the two have in common.)
template <int ZK_XXW>
__device__ __forceinline__ void zk_xxh64_lean_body(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                    ZkFrameInfo *infos, uint64_t *hashes)
{
    const uint32_t lane = threadIdx.x, f = blockIdx.x * 16 + (lane >> 2), kl = lane & 3;
    const ZkXxhLane x = zk_xxh64_lane(f < count, f, data, d_off, first, infos, nullptr);
    uint64_t acc = ZK_XXH64_SEED(kl);
    // the stripes every live frame of the wave has, in whole double batches: no predicates
    if (x.least == ~0ull) return;                           // no frame to hash in this wave
    const uint64_t common = x.least - x.least % (2 * ZK_XXW);
    const uint8_t *q = x.p + 8 * kl;
    uint64_t wa[ZK_XXW], wb[ZK_XXW];
    if (common) {
#pragma unroll
        for (int u = 0; u < ZK_XXW; u++) wa[u] = zk_ld64(q + 32 * (uint64_t)u);
        for (uint64_t s = 0; s < common; s += 2 * ZK_XXW) {
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) wb[u] = zk_ld64(q + 32 * (s + ZK_XXW + u));
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) acc = zk_xround(acc, wa[u]);
            const uint64_t nx = s + 2 * ZK_XXW < common ? s + 2 * ZK_XXW : 0;     // (the last round reads the frame's first batch again)
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) wa[u] = zk_ld64(q + 32 * (nx + u));
#pragma unroll
            for (int u = 0; u < ZK_XXW; u++) acc = zk_xround(acc, wb[u]);
        }
    }
    // what is left of the longer frames, stripe by stripe
    for (uint64_t i = common; i < x.nstripes; i++) acc = zk_xround(acc, zk_ld64(q + (i << 5)));
    const uint32_t base = lane & ~3u;
    const uint64_t v1 = __shfl(acc, base, 64), v2 = __shfl(acc, base + 1, 64), v3 = __shfl(acc, base + 2, 64), v4 = __shfl(acc, base + 3, 64);
    if (kl != 0 || !x.live) return;
    const uint64_t h = zk_xxh64_finish(v1, v2, v3, v4, x.p, x.len, x.nstripes);
    if (hashes) hashes[f] = h;
    if (infos && (uint32_t)h != infos[f].checksum) infos[f].status = ZK_E_CHECKSUM_WRONG;
}

constexpr int ZK_XXL = 12;                                   // zk_k_xxh64_lean's stripes per batch
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void zk_k_xxh64_lean(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                                                                  ZkFrameInfo *infos, uint64_t *hashes)
{
    zk_xxh64_lean_body<ZK_XXL>(data, d_off, first, count, infos, hashes);
}

// The checksums of a large batch WHILE the executor writes it (zk_engine.hip launches this kernel on the context's second queue
// beside zk_k_exec).  A frame's four chains are 65 536 dependent rounds per 2 MiB whoever runs them (2.75 ms behind an 8 ms
// executor: a fifth of the step); but the first byte of a frame is final milliseconds before its last one.  The layout of
// zk_k_xxh64_lean -- sixteen frames per wave, 64 registers: a wave that fits beside four executor waves of 96 on a SIMD -- with the
// sixteen frames advancing together behind the slowest of their executors' progress words (zk_publish above: relaxed agent-scope
// polls, one invalidation of this CU's L1 per step forward, plain loads behind it).  Wave g takes the frames g % 8 + 8 k of its
// group of 128: the frames whose executors the dispatcher puts on XCD g % 8, where it puts this wave too -- if it does (see above).
//   Nothing depends on this kernel: a frame it verifies is marked ZK_PROG_VERIFIED in its progress word; every other frame --
// its executor ran on another XCD, never came (the two kernels were serialised: a profiler, one hardware queue), the wave gave up
// after ZK_FOLLOW_PATIENCE without any news, the hash differs from the frame's Content_Checksum for whatever reason -- is left to
// the pass behind the executor (zk_k_xxh64_wide with `skip`), which alone reports ZK_E_CHECKSUM_WRONG.  All loops are left by the
// whole wave on a wave-uniform verdict (the trap of the per-lane exit from a polling loop).
#ifndef ZK_FOLLOW_W
#define ZK_FOLLOW_W 7
#endif
constexpr uint64_t ZK_FOLLOW_PATIENCE = 5000000;             // wall_clock64 ticks (100 MHz): 50 ms without any progress
template <int W>
__device__ __forceinline__ void zk_xxh64_follow_body(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                      const ZkFrameInfo *infos, uint64_t *progress)
{
    const uint32_t lane = threadIdx.x, g = blockIdx.x, kl = lane & 3;
    const uint32_t here = ZKX_XCC_ID() + 1;
    uint64_t t_news = ZKX_CLOCK();
    // Which frames run on this XCD?  The dispatcher deals a kernel's workgroups round the XCDs, b -> (b + r) % 8, with a start r that
    // differs from launch to launch (tools/ubench/xcc_map.hip): the first executor whose word appears tells r, and of the 128 frames
    // of this wave's group the class c = (this XCD - r) % 8 is the one to follow.  (A habit, not a promise: every frame's own word is
    // checked again below.)
    uint32_t rot;
    for (;;) {
        uint32_t cand = 0xFFFFFFFFu;
        if (lane < count) {
            const uint64_t w = ZKX_PROG_LOAD(progress + lane);
            if (w != 0) cand = (((uint32_t)(w >> 32) & 15u) - 1u - lane) & 7u;
        }
        const unsigned long long m = __ballot(cand != 0xFFFFFFFFu);
        if (m) { rot = (uint32_t)__builtin_amdgcn_readlane(cand, __builtin_ctzll(m)); break; }
        const uint32_t waited = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ZKX_CLOCK() - t_news > ZK_FOLLOW_PATIENCE));
        if (waited) return;
        ZKX_SLEEP(20);
    }
    const uint32_t f = (g >> 3) * 128 + ((here - 1u - rot) & 7u) + 8 * (lane >> 2);
    bool live = f < count;
    if (live && !(infos[f].status == ZK_OK && infos[f].checksum_flag)) live = false;
    const uint32_t fa = live ? f : 0;                       // (a lane without a frame reads frame 0 and keeps nothing)
    const uint8_t *p = data + (d_off[first + fa] - d_off[first]);
    const uint64_t len = d_off[first + fa + 1] - d_off[first + fa];
    const uint32_t nstripes = live ? (uint32_t)(len >> 5) : 0;
    uint64_t acc = ZK_XXH64_SEED(kl);
    auto wave_min = [](uint32_t v) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) { const uint32_t o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
        return (uint32_t)__builtin_amdgcn_readfirstlane(v);
    };
    // the frame's word: bytes complete (0 before its executor has started), or 0xFFFFFFFF for "not mine (any more)": failed, or
    // written through another XCD's L2
    auto news = [&]() {
        uint32_t have = 0xFFFFFFFFu;
        if (live) {
            const uint64_t w = ZKX_PROG_LOAD(progress + f);
            if ((w & ZK_PROG_ABORT) || (w != 0 && ((uint32_t)(w >> 32) & 15u) != here)) live = false;
            else have = (uint32_t)w;
        }
        return have;
    };
    uint32_t s = 0, common = 0;
    {
        const uint32_t least = wave_min(live ? nstripes : 0xFFFFFFFFu);
        if (least == 0xFFFFFFFFu) return;                   // no frame to hash in this wave
        common = least - least % (2 * W);                   // the stripes every frame has, in whole double batches (a frame that drops out later changes nothing)
    }
    const uint8_t *q = p + 8 * kl;
    uint64_t wa[W], wb[W];
    // A: the sixteen frames together, as far as the slowest executor has come
    while (s < common) {
        const uint32_t have = news();
        if (__ballot(live) == 0) return;
        uint32_t upto = wave_min(have == 0xFFFFFFFFu ? have : have >> 5);
        upto = upto < common ? upto - upto % (2 * W) : common;
        if (upto <= s) {
            const uint32_t waited = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ZKX_CLOCK() - t_news > ZK_FOLLOW_PATIENCE));
            if (waited) return;                             // (the whole wave: `waited` is scalar)
            ZKX_SLEEP(100);
            continue;
        }
        ZKX_ACQUIRE();  // (s_waitcnt vmcnt(0); buffer_inv sc1: this CU's L1 may hold the buffer's bytes of an earlier decode)
        t_news = ZKX_CLOCK();
#pragma unroll
        for (int u = 0; u < W; u++) wa[u] = zk_ld64(q + 32 * (uint64_t)(s + u));
        for (uint32_t x = s; x < upto; x += 2 * W) {
#pragma unroll
            for (int u = 0; u < W; u++) wb[u] = zk_ld64(q + 32 * (uint64_t)(x + W + u));
#pragma unroll
            for (int u = 0; u < W; u++) acc = zk_xround(acc, wa[u]);
            const uint32_t nx = x + 2 * W < upto ? x + 2 * W : s;       // (the last round reads the step's first batch again)
#pragma unroll
            for (int u = 0; u < W; u++) wa[u] = zk_ld64(q + 32 * (uint64_t)(nx + u));
#pragma unroll
            for (int u = 0; u < W; u++) acc = zk_xround(acc, wb[u]);
        }
        s = upto;
    }
    // B: what is left of every frame once ALL of it is there
    for (;;) {
        const uint32_t have = news();
        const bool pending = live && have < (uint32_t)len;
        if (__ballot(pending) == 0) break;
        const uint32_t waited = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ZKX_CLOCK() - t_news > ZK_FOLLOW_PATIENCE));
        if (waited) return;
        ZKX_SLEEP(100);
    }
    ZKX_ACQUIRE();
    for (uint32_t i = common; i < nstripes; i++) acc = zk_xround(acc, zk_ld64(q + ((uint64_t)i << 5)));
    const uint32_t base = lane & ~3u;
    const uint64_t v1 = __shfl(acc, base, 64), v2 = __shfl(acc, base + 1, 64), v3 = __shfl(acc, base + 2, 64), v4 = __shfl(acc, base + 3, 64);
    if (kl != 0 || !live) return;
    const uint64_t h = zk_xxh64_finish(v1, v2, v3, v4, p, len, nstripes);
    progress[f] |= (uint32_t)h == infos[f].checksum ? ZK_PROG_VERIFIED : ZK_PROG_MISMATCH;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void zk_k_xxh64_follow(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                                                                    const ZkFrameInfo *infos, uint64_t *progress)
{
    zk_xxh64_follow_body<ZK_FOLLOW_W>(data, d_off, first, count, infos, progress);
}

// The same for a HANDFUL of frames (r6): a wave per frame -- zk_k_xxh64's layout, the fastest a frame's four chains run on this device
// (1.7 ms per 2 MiB; sixteen frames to a wave: 2.25 ms) -- behind the frame's progress word.  Eight waves per group of eight frames;
// wave g takes, of its group, the frame whose executor shares ITS XCD (the word says where it runs; two waves of a group on one XCD hash
// the same frame twice and leave another to the pass behind the executor, which takes every frame that is not marked verified).
__global__ __launch_bounds__(64) void zk_k_xxh64_follow1(const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                                                         const ZkFrameInfo *infos, uint64_t *progress)
{
    __shared__ uint64_t prod[128];
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    const uint32_t here = ZKX_XCC_ID() + 1;
    uint64_t t_news = ZKX_CLOCK();
    const uint32_t g0 = g & ~7u;
    uint32_t f = 0xFFFFFFFFu;
    for (;;) {                                               // whose executor runs here?  Once every word of the group has spoken:
        bool mine = false, pending = false;
        if (lane < 8 && g0 + lane < count) {
            const uint64_t w = ZKX_PROG_LOAD(progress + g0 + lane);
            if (w == 0) pending = true;
            else mine = !(w & ZK_PROG_ABORT) && ((uint32_t)(w >> 32) & 15u) == here;
        }
        const unsigned long long mm = __ballot(mine), pm = __ballot(pending);
        if (!pm) {
            if (!mm) return;                                 // none of the group's frames runs on this XCD
            // the frames that run here, in order; this wave takes number (its place in the group) mod (how many): one each when the
            // dispatcher deals waves and workgroups round the XCDs alike
            unsigned long long m2 = mm;
            for (uint32_t k = (g & 7u) % (uint32_t)__popcll(mm); k; k--) m2 &= m2 - 1;
            f = g0 + (uint32_t)__builtin_ctzll(m2);
            break;
        }
        const uint32_t waited = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ZKX_CLOCK() - t_news > ZK_FOLLOW_PATIENCE));
        if (waited) return;
        ZKX_SLEEP(20);
    }
    if (!(infos[f].status == ZK_OK && infos[f].checksum_flag)) return;
    const uint8_t *p = data + (d_off[first + f] - d_off[first]);
    const uint64_t len = d_off[first + f + 1] - d_off[first + f];
    const uint64_t nchunks = len >> 10;
    const uint32_t kl = lane & 3;
    uint64_t acc = ZK_XXH64_SEED(kl);
    const bool aligned = (((uintptr_t)p) & 15) == 0;
    uint64_t a = 0, b = 0;
    auto ldpair = [&](uint64_t c) {
        const uint8_t *q = p + (c << 10) + lane * 16;
        if (aligned) { uint4 v = *reinterpret_cast<const uint4 *>(q); a = v.x | ((uint64_t)v.y << 32); b = v.z | ((uint64_t)v.w << 32); }
        else { a = zk_ld64(q); b = zk_ld64(q + 8); }
    };
    uint64_t have = 0;                                       // bytes of the frame known to be final
    // wait until `need` bytes are final; false: the frame is not (any more) this wave's -- it failed, ran elsewhere, or nothing was heard for too long
    auto wait_for = [&](uint64_t need) -> bool {
        while (have < need) {
            const uint64_t w = zk_uni((uint64_t)ZKX_PROG_LOAD(progress + f));     // one verdict per pass for the whole wave
            if ((w & ZK_PROG_ABORT) || ((uint32_t)(w >> 32) & 15u) != here) return false;
            const uint64_t got = (uint32_t)w;
            if (got > have) { have = got; t_news = ZKX_CLOCK(); ZKX_ACQUIRE(); continue; }     // (this CU's L1 may hold the buffer's bytes of an earlier decode)
            if (ZKX_CLOCK() - t_news > ZK_FOLLOW_PATIENCE) return false;
            ZKX_SLEEP(50);
        }
        return true;
    };
    // (the word is wave-uniform, so is every verdict: the loops below are left by the whole wave)
    if (nchunks) { if (!wait_for(1024)) return; ldpair(0); }
    for (uint64_t c = 0; c < nchunks; c++) {
        prod[2 * lane] = a * XP2; prod[2 * lane + 1] = b * XP2;
        if (c + 1 < nchunks) { if (!wait_for((c + 2) << 10)) return; ldpair(c + 1); }
        __syncthreads();
        if (lane < 16) {
#pragma unroll 8
            for (int r = 0; r < 32; r++) acc = zk_rotl64(acc + prod[4 * r + kl], 31) * XP1;
        }
        __syncthreads();
    }
    if (!wait_for(len)) return;
    const uint64_t nstripes = len >> 5;
    if (lane < 16) for (uint64_t i = nchunks << 5; i < nstripes; i++) acc = zk_xround(acc, zk_ld64(p + (i << 5) + 8 * kl));
    uint64_t v1 = __shfl(acc, 0, 64), v2 = __shfl(acc, 1, 64), v3 = __shfl(acc, 2, 64), v4 = __shfl(acc, 3, 64);
    if (lane != 0) return;
    const uint64_t h = zk_xxh64_finish(v1, v2, v3, v4, p, len, nstripes);
    atomicOr((unsigned long long *)(progress + f), (uint32_t)h == infos[f].checksum ? ZK_PROG_VERIFIED : ZK_PROG_MISMATCH);
}

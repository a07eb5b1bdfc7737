// zk_progress.h -- what the executor kernels (zk_decode.hip: zk_publish) and the checksum followers (zk_xxh64.h) share: the layout of
// a frame's progress word, the XCD a wave runs on and zk_uni.  hipcc compiles it as part of zk_decode.hip; g++ includes it with
// tests/sim/hip_wg_emu.h in front (tests/sim/zk_xxh_sim.cpp), which supplies the hook that has no meaning on the CPU.
#pragma once
#include <stdint.h>

// a value the whole wave holds alike, said so to the compiler (a scalar register; a branch on it is a scalar branch)
__device__ __forceinline__ uint32_t zk_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t zk_uni(uint64_t v) { return (uint64_t)zk_uni((uint32_t)v) | ((uint64_t)zk_uni((uint32_t)(v >> 32)) << 32); }

// the word: [31:0] bytes complete, [35:32] XCD + 1 (a word that is 0 says nothing yet), [60] the frame has failed,
// [61] / [62] set by the checksum wave at its end: verified / hashed and found different
constexpr uint64_t ZK_PROG_ABORT = 1ull << 60, ZK_PROG_VERIFIED = 1ull << 61, ZK_PROG_MISMATCH = 1ull << 62;
// the XCD this wave runs on (HW_REG_XCC_ID)
#ifndef ZKX_XCC_ID
__device__ __forceinline__ uint32_t zk_xcc_id()
{
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
    return x;
}
#define ZKX_XCC_ID() zk_xcc_id()
#endif

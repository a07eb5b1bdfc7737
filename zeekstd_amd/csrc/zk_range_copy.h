// zk_range_copy.h -- the copy routine of the byte-range reads: what zk_k_range_gather (zk_ranges.hip) and zk_k_view_gather (zk_view.h)
// move bytes with.  Plain C++ over uint4, so that the workgroup emulator of tests/sim runs it as well.
#pragma once
#include <stdint.h>

// 16 bytes as the destination sees them, from any source address (global_load_dwordx4 takes unaligned addresses)
struct __attribute__((packed, aligned(1))) ZkU16 { uint32_t w[4]; };

// n bytes src -> dst by T lanes: 16-byte stores on the destination's grid, the bytes in front of and behind it one by one.  Nothing
// outside [dst, dst + n) is written and nothing outside [src, src + n) read.
template <uint32_t T> __device__ __forceinline__ void zk_range_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n, uint32_t t)
{
    uint64_t head = (0 - (uintptr_t)dst) & 15;
    if (head > n) head = n;
    if (t < head) dst[t] = src[t];
    const uint64_t n16 = (n - head) >> 4;
    uint4 *__restrict__ o = reinterpret_cast<uint4 *>(dst + head);
    const ZkU16 *__restrict__ s = reinterpret_cast<const ZkU16 *>(src + head);
    uint64_t i = t;
    for (; i + 3 * T < n16; i += 4 * T) {               // four loads in flight per lane
        const ZkU16 v0 = s[i], v1 = s[i + T], v2 = s[i + 2 * T], v3 = s[i + 3 * T];
        o[i] = make_uint4(v0.w[0], v0.w[1], v0.w[2], v0.w[3]);
        o[i + T] = make_uint4(v1.w[0], v1.w[1], v1.w[2], v1.w[3]);
        o[i + 2 * T] = make_uint4(v2.w[0], v2.w[1], v2.w[2], v2.w[3]);
        o[i + 3 * T] = make_uint4(v3.w[0], v3.w[1], v3.w[2], v3.w[3]);
    }
    for (; i < n16; i += T) { const ZkU16 v = s[i]; o[i] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]); }
    const uint64_t done = head + (n16 << 4);
    if (done + t < n) dst[done + t] = src[done + t];    // (fewer than 16 bytes)
}

// zk_enc_far.h -- the kernels that feed the matcher its far history (included by zk_encode.hip, which keeps their launchers;
// tests/sim/zk_enc_far_sim.cpp runs the same source on the CPU under a workgroup emulator, against the tables of the CPU twin
// oracle/zstd_oracle_enc.c: ldm_build / ldm_build_frame / dense_build_frame / dense_lookup).
//   zk_k_enc_stage_hist        prefix mode: the [prefix tail | frame] records the matcher reads
//   zk_k_enc_ldm_build         the sampled long-distance table over a prefix the ring cannot hold
//   zk_k_enc_ldm_build_frames  the same per frame over its own bytes (in-frame far history)
//   zk_k_enc_dense_part / zk_k_enc_dense_cand   the dense levels: a far candidate per input byte
// HBM-bound integer/byte work; no MFMA.  ZKE_CLK* (experiments) and zke_first16 / ZKE_FFBH come from zk_enc_match.h.
#pragma once
#include <stdint.h>
#include "zk_enc_device.h"
#include "zk_enc_match.h"

// [prefix tail | frame] records for the matcher (prefix mode only; not on the hot path)
__global__ __launch_bounds__(256) void zk_k_enc_stage_hist(const uint8_t *src, const uint8_t *prefix_tail, const ZkEncFrame *frames, uint8_t *stage)
{
    const ZkEncFrame fr = frames[blockIdx.x];
    uint8_t *rec = stage + fr.m_off;
    for (uint32_t i = threadIdx.x; i < fr.hist; i += 256) rec[i] = prefix_tail[i];
    const uint8_t *from = src + fr.src_off;
    for (uint32_t i = threadIdx.x; i < fr.d_size; i += 256) rec[fr.hist + i] = from[i];
}
// The long-distance table over prefix[u0, plen): every sampled position (zke_ldm_selected) enters, the smallest position keeps
// a slot.  Four positions per lane and pass out of 20 bytes; the table was filled with ZKE_LDM_NONE.
__global__ __launch_bounds__(256) void zk_k_enc_ldm_build(ZkEncLdm ldm, uint32_t *table)
{
    const uint64_t n = ldm.plen - ldm.u0;
    const uint8_t *s = ldm.pfx + ldm.u0;
    for (uint64_t i = 4ull * ((uint64_t)blockIdx.x * 256 + threadIdx.x); i + ZKE_LDM_MIN <= n; i += 4ull * gridDim.x * 256) {
        uint32_t w[5];
        memcpy(w, s + i, 16);
        if (i + 20 <= n) memcpy(&w[4], s + i + 16, 4);
        else { w[4] = 0; for (uint64_t j = i + 16; j < n; j++) w[4] |= (uint32_t)s[j] << (8 * (j - i - 16)); }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i + k + ZKE_LDM_MIN > n) break;
            const uint32_t h = zke_ldm_hash(__builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)k), __builtin_amdgcn_alignbyte(w[2], w[1], (uint32_t)k),
                                            __builtin_amdgcn_alignbyte(w[3], w[2], (uint32_t)k), __builtin_amdgcn_alignbyte(w[4], w[3], (uint32_t)k));
            if (zke_ldm_selected(h)) atomicMin(&table[zke_ldm_slot(h, ldm.log)], (uint32_t)(i + k));
        }
    }
}
// The same for the frames' own tables (in-frame far history): blockIdx.y = frame; frame f's table = table + (f << ldm.log), of which
// its own 2^zke_ldm_log(size) entries are used.  Under a frame list (ZkEncLdm::lf) blockIdx.y counts the frames that have a table.
__global__ __launch_bounds__(256) void zk_k_enc_ldm_build_frames(const uint8_t *src, ZkEncLdm ldm, uint32_t *table, uint32_t f0)
{
    // (under a frame list: the f-th frame that qualifies, its table where the list says)
    const uint64_t f = (uint64_t)f0 + blockIdx.y, at = ldm.lf ? ldm.lf[f].start : f * ldm.frame_size;
    const uint64_t n = ldm.lf ? ldm.lf[f].size : ldm.n_total - at < ldm.frame_size ? ldm.n_total - at : ldm.frame_size;
    const uint32_t log = zke_ldm_log(n);
    const uint8_t *s = src + at;
    uint32_t *t = table + (ldm.lf ? ldm.lf[f].tbase : f << ldm.log);
    for (uint64_t i = 4ull * ((uint64_t)blockIdx.x * 256 + threadIdx.x); i + ZKE_LDM_MIN <= n; i += 4ull * gridDim.x * 256) {
        uint32_t w[5];
        for (int k = 0; k < 5; k++) { w[k] = 0; const uint64_t q = i + 4 * k; if (q + 4 <= n) memcpy(&w[k], s + q, 4); else for (uint64_t b = q; b < n; b++) w[k] |= (uint32_t)s[b] << (8 * (b - q)); }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i + k + ZKE_LDM_MIN > n) break;
            const uint32_t h = zke_ldm_hash(__builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)k), __builtin_amdgcn_alignbyte(w[2], w[1], (uint32_t)k),
                                            __builtin_amdgcn_alignbyte(w[3], w[2], (uint32_t)k), __builtin_amdgcn_alignbyte(w[4], w[3], (uint32_t)k));
            if (zke_ldm_selected(h)) atomicMin(&t[zke_ldm_slot(h, log)], (uint32_t)(i + k));
        }
    }
}
// DENSE far history (round 6; ZkEncLdm in zk_enc_device.h, the rule: oracle/zstd_oracle_enc.c dense_build_frame / dense_lookup): two
// kernels, a workgroup per matcher segment each, leave every position's far candidate (length | catch-up << 5 | distance << 8) in
// `cand`, where the match kernel reads it in whole lines.  The two tables a position is looked up in -- smallest position per slot of
// its own segment, largest position + 1 per slot of the segment before, over the 5-byte hash of EVERY position -- exist in LDS only,
// 2^13 slots of both per pass (64 KiB: two workgroups per CU).
//   zk_k_enc_dense_part  hashes every position ONCE and sorts it by the pass its slot belongs to: per segment and pass a list of
//                        `position in the segment << 13 | slot in the pass` in `part` (count, prefix, place: every wave owns a piece of
//                        every list, so the only atomics are a wave's own LDS cursors)
//   zk_k_enc_dense_cand  per pass: the list of the segment before and the own list into the tables (every lane has an entry), the own
//                        list again for the lookups; what a pass finds is appended to the list of the position's 8192-position chunk,
//                        which lives where the chunk's entries of `cand` will be; a last sweep per chunk measures the candidates
//                        (16 bytes + the 4 bytes in front, through L2, all lanes at work) and writes the entries in whole lines.
// How it got here (profiles/r06c_dense_probe.txt, ms per 4 GiB): tables in HBM read by the match kernel 212 (two random 4-byte reads
// per input byte = a line from HBM each); one kernel that hashed both segments in every pass and filtered by slot range 107-134 (~650
// vector instructions per position, one lane in eight at work behind the filter); the partition 75; two workgroups per CU 63.  HBM-bound byte
// work: 4 bytes of `part` and 4 of `cand` per input byte.
constexpr uint32_t ZKD_PLOG = 13, ZKD_PSLOTS = 1u << ZKD_PLOG, ZKD_NBMAX = ZKE_DENSE_PASSES_MAX, ZKD_U = 8;
template <bool PLACE>
__device__ __forceinline__ void zkd_sweep(const uint8_t *frame, uint32_t s0, uint32_t e1, uint32_t fsz, uint32_t dlog, uint32_t tid, uint32_t *wcnt, uint32_t *lst)
{
    // (eight steps' input requested before the first is hashed: four waves per SIMD do not cover a trip to L2 per step)
    for (uint32_t qb = s0 + 4 * tid; qb < e1; qb += 4096 * ZKD_U) {
        uint32_t w0[ZKD_U], w1[ZKD_U];
#pragma unroll
        for (uint32_t u = 0; u < ZKD_U; u++) {
            const uint32_t q0 = qb + 4096 * u, at = q0 < e1 && q0 + 8 <= fsz ? q0 : 0;      // (none of a step's four positions has its eight bytes: the frame's first bytes, unused)
            memcpy(&w0[u], frame + at, 4); memcpy(&w1[u], frame + at + 4, 4);
        }
#pragma unroll
        for (uint32_t u = 0; u < ZKD_U; u++) {
            const uint32_t q0 = qb + 4096 * u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t q = q0 + k;
                const uint32_t lo = __builtin_amdgcn_alignbyte(w1[u], w0[u], (uint32_t)k);
                const uint32_t h = zke_hash(lo, (w1[u] >> (8 * k)) & 0xFFu, dlog);
                // a position whose four bytes are one byte stays out: a byte run, offset 1 codes it better (the twin has the numbers)
                if (q < e1 && q + 8 <= fsz && lo != (lo & 0xFFu) * 0x01010101u) {
                    const uint32_t i = atomicAdd(&wcnt[h >> ZKD_PLOG], 1u);
                    if (PLACE) lst[i] = ((q - s0) << ZKD_PLOG) | (h & (ZKD_PSLOTS - 1));
                }
            }
        }
    }
}
__global__ __launch_bounds__(1024) void zk_k_enc_dense_part(const uint8_t *src, const ZkEncFrame *segs, ZkEncLdm ldm, uint32_t *part, uint32_t *poff)
{
    // per wave and pass: its count, then its cursor.  (A counter per LANE and pass -- no two lanes on one LDS word -- measured slower, 74.9 ->
    // 98.7 ms: a wave's 64 stores then go to 64 different places of the lists instead of a handful of dense streams)
    __shared__ uint32_t cnt[16][ZKD_NBMAX];
    __shared__ uint32_t total[ZKD_NBMAX], start[ZKD_NBMAX + 1];
    const ZkEncFrame sg = segs[blockIdx.x];
    const uint8_t *frame = src + sg.src_off;
    const uint32_t fsz = zke_ldm_frame_bytes(ldm, sg);
    const uint32_t s0 = sg.seg_at, e1 = s0 + sg.d_size, tid = threadIdx.x, dlog = ldm.dlog, wave = tid >> 6, nb = 1u << (dlog - ZKD_PLOG);
    uint32_t *lst = part + sg.src_off + s0;                         // the segment's lists, pass after pass
    static_assert(16 * ZKD_NBMAX <= 1024, "one counter per lane");
    // a last frame of fewer than 8 bytes has no position to list, and not the 8 bytes zkd_sweep reads at the frame's start for a step without
    // positions: behind it the caller's source ends (found by tests/sim/enc_far_san.cpp)
    if (fsz < 8) { if (tid <= nb) poff[(size_t)blockIdx.x * (ZKD_NBMAX + 1) + tid] = 0; return; }
    if (tid < 16 * ZKD_NBMAX) (&cnt[0][0])[tid] = 0;
    __syncthreads();
    zkd_sweep<false>(frame, s0, e1, fsz, dlog, tid, cnt[wave], lst);
    __syncthreads();
    if (tid < nb) { uint32_t t = 0; for (uint32_t w = 0; w < 16; w++) t += cnt[w][tid]; total[tid] = t; }
    __syncthreads();
    if (tid == 0) { uint32_t run = 0; for (uint32_t b = 0; b < nb; b++) { start[b] = run; run += total[b]; } start[nb] = run; }
    __syncthreads();
    if (tid < nb) { uint32_t run = start[tid]; for (uint32_t w = 0; w < 16; w++) { const uint32_t c = cnt[w][tid]; cnt[w][tid] = run; run += c; } }
    if (tid <= nb) poff[(size_t)blockIdx.x * (ZKD_NBMAX + 1) + tid] = start[tid];
    __syncthreads();
    zkd_sweep<true>(frame, s0, e1, fsz, dlog, tid, cnt[wave], lst);
}
__global__ __launch_bounds__(1024) void zk_k_enc_dense_cand(const uint8_t *src, const ZkEncFrame *segs, ZkEncLdm ldm, const uint32_t *part, const uint32_t *poff, uint32_t *cand)
{
    constexpr uint32_t PLOG = ZKD_PLOG, PSLOTS = ZKD_PSLOTS;
#ifndef ZKD_E
#define ZKD_E 16
#endif
    constexpr uint32_t E = ZKD_E;                                   // list entries requested per lane before the first is used (4 | 8 | 16: 50.1 | 47.9 | 47.1 ms per 4 GiB)
    constexpr uint32_t CLOG = 13, CHUNK = 1u << CLOG, NCHUNK = ZKE_SEGMENT / CHUNK;     // found candidates are listed per chunk of 8192 positions
    static_assert(ZKE_SEGMENT + ZKE_SEGMENT - ZKE_WINDOW <= (1u << (32 - CLOG)), "a list entry: position inside the chunk | (distance - ZKE_WINDOW - 1) << 13");
    static_assert(ZKE_SEGMENT <= (1u << (32 - PLOG)), "an entry of `part`: position inside the segment << 13 | slot");
    __shared__ uint32_t first[PSLOTS], last[PSLOTS];
    __shared__ uint32_t count[NCHUNK];
    // Which segment: workgroups go to the eight XCDs in turn, each with an L2 of its own; workgroup b takes segment (b % 8) * (n / 8) + b / 8, so
    // that an XCD works through CONSECUTIVE segments -- the candidates of a segment lie in its own and the segment before's bytes, which the
    // same L2 has just seen -- instead of every eighth one of all frames (62.4 -> see profiles/r06c_dense_probe.txt)
    const uint32_t nwg = gridDim.x, seg = (nwg & 7u) ? blockIdx.x : (blockIdx.x & 7u) * (nwg >> 3) + (blockIdx.x >> 3);
    const ZkEncFrame sg = segs[seg];
    const uint8_t *frame = src + sg.src_off;
    const uint32_t fsz = zke_ldm_frame_bytes(ldm, sg);
    const uint32_t s0 = sg.seg_at, e1 = s0 + sg.d_size, tid = threadIdx.x, dlog = ldm.dlog;
    uint32_t *out = cand + sg.src_off;                              // indexed by the position inside the frame
    const uint32_t *olist = part + sg.src_off + s0, *plist = olist - ZKE_SEGMENT;           // the segment before mine is a whole one, and the one before me in the list
    const uint32_t *oo = poff + (size_t)seg * (ZKD_NBMAX + 1), *po = oo - (ZKD_NBMAX + 1);
    // a last frame of fewer than 20 bytes has no candidates, and not the 20 bytes the last sweep reads at the frame's start for a position
    // without one: behind it the caller's source ends (found by tests/sim/enc_far_san.cpp)
    if (fsz < 20) { for (uint32_t q = s0 + tid; q < e1; q += 1024) out[q] = 0; return; }
    if (tid < NCHUNK) count[tid] = 0;
    ZKE_CLK_BEGIN();
    for (uint32_t pass = 0; pass < (1u << (dlog - PLOG)); pass++) {
        for (uint32_t i = tid; i < PSLOTS; i += 1024) { first[i] = ZKE_DENSE_NONE; last[i] = 0; }
        __syncthreads();
        // (E entries requested per lane before the first is used: a pass's lists are ~16 entries per lane, so usually all of them)
        if (s0) {
            const uint32_t *l = plist + po[pass], n = po[pass + 1] - po[pass];
            for (uint32_t i0 = tid; i0 < n; i0 += 1024 * E) {
                uint32_t e[E];
#pragma unroll
                for (uint32_t u = 0; u < E; u++) e[u] = l[i0 + 1024 * u < n ? i0 + 1024 * u : i0];
#pragma unroll
                for (uint32_t u = 0; u < E; u++) if (i0 + 1024 * u < n) atomicMax(&last[e[u] & (PSLOTS - 1)], (e[u] >> PLOG) + 1);
            }
        }
        const uint32_t *l = olist + oo[pass], n = oo[pass + 1] - oo[pass];
        for (uint32_t i0 = tid; i0 < n; i0 += 1024 * E) {
            uint32_t e[E];
#pragma unroll
            for (uint32_t u = 0; u < E; u++) e[u] = l[i0 + 1024 * u < n ? i0 + 1024 * u : i0];
#pragma unroll
            for (uint32_t u = 0; u < E; u++) if (i0 + 1024 * u < n) atomicMin(&first[e[u] & (PSLOTS - 1)], e[u] >> PLOG);
        }
        __syncthreads();
        ZKE_CLK(13);
        // What a pass finds is NOT stored by position -- a line of `cand` would be written an eighth at a time, pass after pass -- but appended
        // to the list of the position's chunk, which lives where the chunk's entries of `cand` will be (a chunk has at most as many candidates
        // as positions): whole lines, filled front to back.
        for (uint32_t i0 = tid; i0 < n; i0 += 1024 * E) {
            uint32_t e[E];
#pragma unroll
            for (uint32_t u = 0; u < E; u++) e[u] = l[i0 + 1024 * u < n ? i0 + 1024 * u : i0];
#pragma unroll
            for (uint32_t u = 0; u < E; u++) {
                if (i0 + 1024 * u >= n) continue;
                const uint32_t r = e[u] >> PLOG, m1 = first[e[u] & (PSLOTS - 1)], m2 = last[e[u] & (PSLOTS - 1)];
                uint32_t d = 0;
                if (m1 < r && r - m1 > ZKE_WINDOW) d = r - m1;                             // (the slot holds a position: mine at the latest)
                else if (m2 && r + ZKE_SEGMENT - (m2 - 1) > ZKE_WINDOW) d = r + ZKE_SEGMENT - (m2 - 1);
                const uint32_t chunk = r >> CLOG;
                if (d) out[s0 + (chunk << CLOG) + atomicAdd(&count[chunk], 1u)] = (r & (CHUNK - 1)) | ((d - ZKE_WINDOW - 1) << CLOG);
            }
        }
        __syncthreads();
        ZKE_CLK(14);
    }
    // Chunk by chunk: the list into LDS by position, then every position's candidate measured -- 16 bytes at the position against 16
    // bytes `distance` before it, every lane at work -- and the chunk's entries of `cand` written in whole lines over its list.
    uint32_t *dist = first;
    for (uint32_t c = 0; (c << CLOG) < sg.d_size; c++) {
        const uint32_t cb = s0 + (c << CLOG);
        for (uint32_t i = tid; i < CHUNK; i += 1024) dist[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < count[c]; i += 1024) { const uint32_t e = out[cb + i]; dist[e & (CHUNK - 1)] = (e >> CLOG) + ZKE_WINDOW + 1; }
        __syncthreads();
        for (uint32_t q0 = cb + 4 * tid; q0 < cb + CHUNK && q0 < e1; q0 += 4096) {
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = dist[q0 - cb + k];
            uint32_t own[5] = {0, 0, 0, 0, 0};
            if (q0 + 20 <= fsz) memcpy(own, frame + q0, 20);
            else for (uint32_t b = q0; b < fsz; b++) own[(b - q0) >> 2] |= (uint32_t)frame[b] << (8 * ((b - q0) & 3));     // the frame's last bytes: zeros behind them
            // ... and the four bytes in front of both (the catch-up count of the entry: how many of them agree, not past the frame's first byte)
            uint32_t before = 0;                                              // bytes q0 - 4 .. q0 - 1 (zeros in front of the frame)
            if (q0 >= 4) memcpy(&before, frame + q0 - 4, 4);
            uint32_t cc[4][5];                                                // the candidate's bytes e - 4 .. e + 15
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t e = d[k] ? q0 + k - d[k] : 4u;                     // (no candidate: the frame's first bytes, unused)
                if (e >= 4) memcpy(cc[k], frame + e - 4, 20);
                else { cc[k][0] = 0; for (uint32_t b = 0; b < e; b++) cc[k][0] |= (uint32_t)frame[b] << (8 * (4 - e + b)); memcpy(&cc[k][1], frame + e, 16); }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t l = zke_first16(cc[k][1] ^ __builtin_amdgcn_alignbyte(own[1], own[0], (uint32_t)k), cc[k][2] ^ __builtin_amdgcn_alignbyte(own[2], own[1], (uint32_t)k),
                                               cc[k][3] ^ __builtin_amdgcn_alignbyte(own[3], own[2], (uint32_t)k), cc[k][4] ^ __builtin_amdgcn_alignbyte(own[4], own[3], (uint32_t)k));
                const uint32_t mine4 = k ? __builtin_amdgcn_alignbyte(own[0], before, (uint32_t)k) : before;      // the four bytes that end at q0 + k
                uint32_t bk = ZKE_FFBH(mine4 ^ cc[k][0]);
                bk = (bk < 32u ? bk : 32u) >> 3;
                const uint32_t e = q0 + k - d[k];
                bk = bk < e ? bk : e;
                d[k] = d[k] && l >= ZKE_DENSE_MIN ? l | (bk << 5) | (d[k] << 8) : 0u;
            }
            if (q0 + 4 <= e1) memcpy(out + q0, d, 16);
            else for (uint32_t k = 0; q0 + k < e1; k++) out[q0 + k] = d[k];
        }
        __syncthreads();
    }
    ZKE_CLK(15);
    ZKE_CLK_END();
}

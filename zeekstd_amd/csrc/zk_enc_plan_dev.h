// zk_enc_plan_dev.h -- the plan of an encode over a caller-given frame list, made ON THE DEVICE from the list's offsets (included by
// zk_encode.hip, which keeps the launcher; tests/sim/zk_enc_plan_list_sim.cpp runs the same source on the CPU under the workgroup emulator
// against zke_plan_fill_list, record by record).
//   zk_k_enc_plan_scan   per frame what it takes -- blocks, matcher segments, sequence entries, scratch bytes -- and the running sums in
//                        front of every frame; the last entry holds the totals, which size the encode's buffers (they go to the host)
//   zk_k_enc_plan_fill   a lane per frame: its ZkEncFrame, its blocks, its segments and its offset, by the one function the host plan
//                        runs per frame (zke_plan_frame, zk_enc_plan.h), started from the frame's running sums
// ZkEncPlanSum and what a frame adds to it are zk_enc_plan.h's: the engine's host code reads the totals.
// Why: the host plan writes and uploads 48 + 64 + 48 bytes per frame of small records; the offsets are 8.
// Integer work on a few bytes per frame; no LDS traffic to speak of, no MFMA.
#pragma once
#include <stdint.h>
#include "zk_enc_device.h"
#include "zk_enc_plan.h"

constexpr uint32_t ZKP_SCAN_THREADS = 1024;
// One workgroup: lane t sums the frames [t * per, (t + 1) * per), the lanes' sums are scanned in LDS, and the lane writes the running sum in
// front of each of its frames.  sums[count + 1]; sums[count] = the totals.  (A lane reads its own run of offsets: 8 bytes per frame out of L2,
// twice.  Half a million frames are 488 per lane.)
__global__ __launch_bounds__(ZKP_SCAN_THREADS) void zk_k_enc_plan_scan(const uint64_t *off, uint32_t count, uint32_t prefix, ZkEncPlanSum *sums)
{
    __shared__ ZkEncPlanSum part[ZKP_SCAN_THREADS];
    const uint32_t tid = threadIdx.x, per = (count + ZKP_SCAN_THREADS - 1) / ZKP_SCAN_THREADS;
    const uint64_t a0 = (uint64_t)tid * per, a1 = a0 + per;
    const uint32_t f0 = (uint32_t)(a0 < count ? a0 : count), f1 = (uint32_t)(a1 < count ? a1 : count);
    ZkEncPlanSum mine = {0, 0, 0, 0};
    for (uint32_t f = f0; f < f1; f++) mine = zke_plan_sum_add(mine, zke_plan_frame_sum(off[f + 1] - off[f], prefix != 0));
    part[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < ZKP_SCAN_THREADS; d <<= 1) {
        ZkEncPlanSum v = {0, 0, 0, 0};
        if (tid >= d) v = part[tid - d];
        __syncthreads();
        part[tid] = zke_plan_sum_add(part[tid], v);
        __syncthreads();
    }
    ZkEncPlanSum run = {0, 0, 0, 0};
    if (tid) run = part[tid - 1];
    for (uint32_t f = f0; f < f1; f++) { sums[f] = run; run = zke_plan_sum_add(run, zke_plan_frame_sum(off[f + 1] - off[f], prefix != 0)); }
    if (tid == ZKP_SCAN_THREADS - 1) sums[count] = part[tid];
}

// A lane per frame of a CHECKED list (non-decreasing, no frame above the format's largest): the records zke_plan_fill_list makes.  The
// [history | frame] records of prefix mode follow one another, so frame f's starts at f * hist + its source offset.
__global__ __launch_bounds__(256) void zk_k_enc_plan_fill(const uint64_t *off, uint32_t count, int level, uint64_t prefix_len, uint32_t hist, const ZkEncPlanSum *sums,
                                                          ZkEncFrame *frames, ZkEncBlock *blocks, ZkEncFrame *segs, uint64_t *doff)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= count) return;
    const uint64_t src_off = off[f] - off[0];
    const ZkEncPlanSum s = sums[f];
    uint32_t bcount = s.nb, sc = s.nseg;
    uint64_t seq_total = s.seq, scratch_total = s.scratch;
    zke_plan_frame(f, src_off, (uint32_t)(off[f + 1] - off[f]), hist ? (uint64_t)f * hist + src_off : src_off, level, prefix_len, hist, frames, blocks, segs, &bcount, &sc,
                   &seq_total, &scratch_total);
    doff[f] = src_off;
    if (f == count - 1) doff[count] = off[count] - off[0];
}

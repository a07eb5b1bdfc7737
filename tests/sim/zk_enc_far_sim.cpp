// zk_enc_far_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels that feed the encoder's matcher its far history (zeekstd_amd/csrc/zk_enc_far.h, the very source hipcc compiles for
// gfx950) on the CPU, one workgroup at a time, under the fiber emulator of hip_wg_emu.h: with the plan the engine uses (zk_enc_plan.h),
// and the launchers' grids, the engine's slices and its buffer sizes out of the functions both of them call (zk_enc_sched.h).  tests/test_sim_enc_far.py compares what they leave -- every position's dense candidate,
// the sorted position lists, the sampled tables, the [prefix tail | frame] records -- with the tables of the CPU twin
// (oracle/zstd_oracle_enc.c: zko_enc_far_debug), entry by entry; tests/sim/enc_far_san.cpp runs the same under AddressSanitizer + UBSan.
// Every buffer a kernel sees is a heap allocation of EXACTLY the size the engine gives it, filled with a poison pattern first: an
// access outside it is a sanitizer report, an entry that was never written is a mismatch.
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_enc_far.h"
#include "../../zeekstd_amd/csrc/zk_enc_sched.h"
#include <memory>

constexpr uint32_t ZKF_POISON = 0xA5A5A5A5u;
template <class T> static std::unique_ptr<T[]> zkf_exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }
static std::unique_ptr<uint8_t[]> zkf_copy(const uint8_t *p, size_t n) { auto c = zkf_exact<uint8_t>(n); if (n) memcpy(c.get(), p, n); return c; }

// DENSE: zk_k_enc_dense_part, then zk_k_enc_dense_cand, for every workgroup of every slice of src[0, n) cut into frames of frame_size bytes.
// slice_bytes: what ZK_CHOICE_ENC_DENSE_SLICE_KIB sets (0: the default of 4 GiB).  Outputs: cand_out[n] (indexed like the source);
// part_out[n] (a segment's lists start at its first byte's index); poff_out[nseg * (ZKD_NBMAX + 1)] (a row per segment of the call).
// Returns the number of segments; -1: the call has no dense history; -2: a kernel wrote into the slack behind `cand` or `part`.
extern "C" int zk_enc_far_sim_dense(const uint8_t *src_in, uint64_t n, uint32_t frame_size, int level, uint64_t slice_bytes, int descending,
                                    uint32_t *cand_out, uint32_t *part_out, uint32_t *poff_out)
{
    ZkEncPlan pl;
    if (!n || !zke_plan_count(n, frame_size, 0, &pl)) return -1;
    const ZkEncCut cut = {nullptr, pl.nf, n, frame_size};
    const ZkEncFarPlan fp = zk_enc_far_plan(cut, level, 0, 0, pl.nseg, slice_bytes);
    if (!fp.dense_span) return -1;
    std::vector<ZkEncFrame> frames(pl.nf), segs(pl.nseg + 1);
    std::vector<ZkEncBlock> blocks(pl.nb + 1);
    zke_plan_fill(n, frame_size, level, 0, &pl, frames.data(), blocks.data(), segs.data(), nullptr);
    const auto src = zkf_copy(src_in, n);
    const size_t ncand = fp.cand_words, npoff = fp.poff_words;
    const auto cand = zkf_exact<uint32_t>(ncand), part = zkf_exact<uint32_t>(ncand), poff = zkf_exact<uint32_t>(npoff);
    emu_set_lane_order(descending != 0);
    int rc = (int)pl.nseg;
    for (uint32_t f0 = 0, s0 = 0; f0 < pl.nf;) {
        const ZkEncSlice end = zk_enc_slice_end(cut, 0, n, fp.slice_cap, pl.nseg, f0, s0);
        const uint64_t lo = zk_enc_frame_src(cut, f0), hi = end.f1 == pl.nf ? n : zk_enc_frame_src(cut, end.f1);
        for (size_t i = 0; i < ncand; i++) cand[i] = part[i] = ZKF_POISON;              // the scratch is reused slice after slice, never cleared
        for (size_t i = 0; i < npoff; i++) poff[i] = ZKF_POISON;
        ZkEncLdm sl = fp.ldm;
        sl.dense = cand.get() - lo;
        // gridDim.x is the slice's segment count, so the candidate kernel's XCD remap is live exactly when it is on the device
        const uint32_t nsegs = end.s1 - s0;
        const ZkEncFrame *sg = segs.data() + s0;
        for (uint32_t b = 0; b < nsegs; b++)
            emu_run_workgroup(1024, b, [&]() { zk_k_enc_dense_part(src.get(), sg, sl, part.get() - lo, poff.get()); }, nsegs);
        for (uint32_t b = 0; b < nsegs; b++)
            emu_run_workgroup(1024, b, [&]() { zk_k_enc_dense_cand(src.get(), sg, sl, part.get() - lo, poff.get(), cand.get() - lo); }, nsegs);
        memcpy(cand_out + lo, cand.get(), (size_t)(hi - lo) * sizeof(uint32_t));
        memcpy(part_out + lo, part.get(), (size_t)(hi - lo) * sizeof(uint32_t));
        memcpy(poff_out + (size_t)s0 * (ZKD_NBMAX + 1), poff.get(), (size_t)nsegs * (ZKD_NBMAX + 1) * sizeof(uint32_t));
        for (size_t i = (size_t)(hi - lo); i < ncand; i++) if (cand[i] != ZKF_POISON || part[i] != ZKF_POISON) rc = -2;
        f0 = end.f1; s0 = end.s1;
    }
    emu_set_lane_order(false);
    return rc;
}

// LDM_FRAMES: zk_k_enc_ldm_build_frames over all (blockIdx.x, blockIdx.y) of the launcher's grid.  table_out: nf << log entries (frame f's
// table at f << log).  Returns log = the common stride's; -1: the call has no in-frame far history.
extern "C" int zk_enc_far_sim_ldm_frames(const uint8_t *src_in, uint64_t n, uint32_t frame_size, int level, int descending, uint32_t *table_out, uint64_t table_cap)
{
    ZkEncPlan pl;
    if (!n || !zke_plan_count(n, frame_size, 0, &pl)) return -1;
    const ZkEncFarPlan fp = zk_enc_far_plan(ZkEncCut{nullptr, pl.nf, n, frame_size}, level, 0, 0, pl.nseg, 0);
    if (fp.kind != ZK_ENC_FAR_INFRAME || fp.entries > table_cap) return -1;
    const ZkEncLdm &ldm = fp.ldm;
    const auto src = zkf_copy(src_in, n);
    const auto table = zkf_exact<uint32_t>((size_t)fp.entries);
    emu_set_lane_order(descending != 0);
    memset(table.get(), 0xFF, fp.table_bytes);
    for (uint32_t f0 = 0; f0 < pl.nf; f0 += ZK_ENC_GRID_Y_MAX) {
        const uint32_t gx = fp.build_gx, cnt = zk_enc_ldm_frames_gy(pl.nf, f0);
        for (uint32_t by = 0; by < cnt; by++)
            for (uint32_t bx = 0; bx < gx; bx++)
                emu_run_workgroup(256, bx, [&]() { zk_k_enc_ldm_build_frames(src.get(), ldm, table.get(), f0); }, gx, by, cnt);
    }
    emu_set_lane_order(false);
    memcpy(table_out, table.get(), fp.table_bytes);
    return (int)ldm.log;
}

// LDM_PREFIX: zk_k_enc_ldm_build over the launcher's grid.  The device copy of the prefix has ZKE_LDM_SLACK readable bytes behind it; so
// has the copy here, and not one more.  table_out: 1 << log entries.  Returns log; -1: the ring holds this prefix, no table.
extern "C" int zk_enc_far_sim_ldm_prefix(const uint8_t *prefix, uint64_t prefix_len, int descending, uint32_t *table_out, uint64_t table_cap)
{
    // (the table depends on the prefix alone: any one frame stands for the call)
    const ZkEncFarPlan fp = zk_enc_far_plan(ZkEncCut{nullptr, 1, 1, 1}, 1, prefix_len, zke_prefix_hist(prefix_len), 1, 0);
    if (fp.kind != ZK_ENC_FAR_PREFIX || fp.entries > table_cap) return -1;
    ZkEncLdm ldm = fp.ldm;
    const auto pcopy = zkf_exact<uint8_t>((size_t)prefix_len + ZKE_LDM_SLACK);
    memcpy(pcopy.get(), prefix, (size_t)prefix_len);
    memset(pcopy.get() + prefix_len, 0xA5, ZKE_LDM_SLACK);
    ldm.pfx = pcopy.get();
    const auto table = zkf_exact<uint32_t>((size_t)fp.entries);
    emu_set_lane_order(descending != 0);
    memset(table.get(), 0xFF, fp.table_bytes);
    for (uint32_t bx = 0; bx < fp.build_gx; bx++)
        emu_run_workgroup(256, bx, [&]() { zk_k_enc_ldm_build(ldm, table.get()); }, fp.build_gx);
    emu_set_lane_order(false);
    memcpy(table_out, table.get(), fp.table_bytes);
    return (int)ldm.log;
}

// STAGE_HIST: zk_k_enc_stage_hist, a workgroup per frame.  stage_out: nf * (hist + frame_size) bytes, poison where no record byte lies.
// Returns hist (the bytes of prefix in front of every frame); -1: stage_cap too small.
extern "C" int zk_enc_far_sim_stage_hist(const uint8_t *src_in, uint64_t n, uint32_t frame_size, int level, const uint8_t *prefix, uint64_t prefix_len,
                                         uint8_t *stage_out, uint64_t stage_cap)
{
    const uint32_t hist = zke_prefix_hist(prefix_len);
    ZkEncPlan pl;
    if (!zke_plan_count(n, frame_size, hist, &pl)) return -1;
    std::vector<ZkEncFrame> frames(pl.nf), segs(pl.nseg + 1);
    std::vector<ZkEncBlock> blocks(pl.nb + 1);
    zke_plan_fill(n, frame_size, level, prefix_len, &pl, frames.data(), blocks.data(), segs.data(), nullptr);
    // the prefix route's buffer: all the records (without history the engine stages nothing; here the kernel copies the frames)
    const size_t bytes = hist ? zk_enc_stage_plan(ZkEncCut{nullptr, pl.nf, n, frame_size}, hist, false, 0).stage_bytes : (size_t)pl.nf * frame_size;
    if (bytes > stage_cap) return -1;
    const auto src = zkf_copy(src_in, n), pre = zkf_copy(prefix, prefix_len);
    const auto stage = zkf_exact<uint8_t>(bytes);
    memset(stage.get(), 0xA5, bytes);
    for (uint32_t f = 0; f < pl.nf; f++)
        emu_run_workgroup(256, f, [&]() { zk_k_enc_stage_hist(src.get(), pre.get() + (prefix_len - hist), frames.data(), stage.get()); }, pl.nf);
    memcpy(stage_out, stage.get(), bytes);
    return (int)hist;
}

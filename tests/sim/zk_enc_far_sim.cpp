// zk_enc_far_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels that feed the encoder's matcher its far history (zeekstd_amd/csrc/zk_enc_far.h, the very source hipcc compiles for
// gfx950) on the CPU, one workgroup at a time, under the fiber emulator of hip_wg_emu.h: with the plan the engine uses (zk_enc_plan.h),
// the launchers' grids and the engine's slices.  tests/test_sim_enc_far.py compares what they leave -- every position's dense candidate,
// the sorted position lists, the sampled tables, the [prefix tail | frame] records -- with the tables of the CPU twin
// (oracle/zstd_oracle_enc.c: zko_enc_far_debug), entry by entry; tests/sim/enc_far_san.cpp runs the same under AddressSanitizer + UBSan.
// Every buffer a kernel sees is a heap allocation of EXACTLY the size the engine gives it, filled with a poison pattern first: an
// access outside it is a sanitizer report, an entry that was never written is a mismatch.
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_enc_far.h"
#include "../../zeekstd_amd/csrc/zk_enc_plan.h"
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
    const uint64_t frame_max = frame_size < n ? frame_size : n;
    if (!zke_dense_in_frame(level, 0, frame_max)) return -1;
    std::vector<ZkEncFrame> frames(pl.nf), segs(pl.nseg + 1);
    std::vector<ZkEncBlock> blocks(pl.nb + 1);
    zke_plan_fill(n, frame_size, level, 0, &pl, frames.data(), blocks.data(), segs.data(), nullptr);
    const auto src = zkf_copy(src_in, n);
    // zk_enc_far_history (zk_engine_enc.hip): "ldm.inframe = 1; ... ldm.dlog = zke_dense_log(a.level);", then the scratch:
    // "L.dense_span = a.n < dense_slice ? a.n : (dense_slice / frame_size ? dense_slice / frame_size : 1) * frame_size", cand and part of
    // dense_span + ZKE_DENSE_SLACK entries each, poff of nseg * (ZKE_DENSE_PASSES_MAX + 1)
    ZkEncLdm ldm = {nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, nullptr, 0, 0};
    ldm.inframe = 1; ldm.frame_size = frame_size; ldm.n_total = n; ldm.log = zke_ldm_log(frame_max); ldm.dlog = zke_dense_log(level);
    const uint64_t dense_slice = slice_bytes ? slice_bytes : 4ull << 30;
    const size_t span = (size_t)(n < dense_slice ? n : (dense_slice / frame_size ? dense_slice / frame_size : 1) * (uint64_t)frame_size);
    const size_t ncand = span + ZKE_DENSE_SLACK, npoff = (size_t)pl.nseg * (ZKD_NBMAX + 1);
    const auto cand = zkf_exact<uint32_t>(ncand), part = zkf_exact<uint32_t>(ncand), poff = zkf_exact<uint32_t>(npoff);
    emu_set_lane_order(descending != 0);
    // zk_enc_match (zk_engine_enc.hip): "fpf = sliced ? dense_span / frame_size : nf, spf = (frame_size + ZKE_SEGMENT - 1) / ZKE_SEGMENT", per slice
    // "f1 = nf - f0 < fpf ? nf : f0 + fpf, s0 = f0 * spf, s1 = f1 == nf ? nseg : f1 * spf, lo = f0 * frame_size" and
    // "zk_launch_enc_dense_cand(st, L.src, L.d_segs + s0, s1 - s0, sl, L.cand - lo, L.part - lo, L.poff)"
    const uint32_t nf = pl.nf, nseg = pl.nseg;
    const bool sliced = span < n;
    const uint32_t fpf = sliced ? (uint32_t)(span / frame_size) : nf, spf = (frame_size + ZKE_SEGMENT - 1) / ZKE_SEGMENT;
    int rc = (int)nseg;
    for (uint32_t f0 = 0; f0 < nf; f0 += fpf) {
        const uint32_t f1 = nf - f0 < fpf ? nf : f0 + fpf, s0 = f0 * spf, s1 = f1 == nf ? nseg : f1 * spf;
        const uint64_t lo = (uint64_t)f0 * frame_size, hi = f1 == nf ? n : (uint64_t)f1 * frame_size;
        for (size_t i = 0; i < ncand; i++) cand[i] = part[i] = ZKF_POISON;              // the scratch is reused slice after slice, never cleared
        for (size_t i = 0; i < npoff; i++) poff[i] = ZKF_POISON;
        ZkEncLdm sl = ldm;
        sl.dense = cand.get() - lo;
        // zk_launch_enc_dense_cand (zk_encode.hip): "zk_k_enc_dense_part, dim3(nsegs), dim3(1024)", then "zk_k_enc_dense_cand, dim3(nsegs), dim3(1024)":
        // gridDim.x is the slice's segment count, so the candidate kernel's XCD remap is live exactly when it is on the device
        const uint32_t nsegs = s1 - s0;
        const ZkEncFrame *sg = segs.data() + s0;
        for (uint32_t b = 0; b < nsegs; b++)
            emu_run_workgroup(1024, b, [&]() { zk_k_enc_dense_part(src.get(), sg, sl, part.get() - lo, poff.get()); }, nsegs);
        for (uint32_t b = 0; b < nsegs; b++)
            emu_run_workgroup(1024, b, [&]() { zk_k_enc_dense_cand(src.get(), sg, sl, part.get() - lo, poff.get(), cand.get() - lo); }, nsegs);
        memcpy(cand_out + lo, cand.get(), (size_t)(hi - lo) * sizeof(uint32_t));
        memcpy(part_out + lo, part.get(), (size_t)(hi - lo) * sizeof(uint32_t));
        memcpy(poff_out + (size_t)s0 * (ZKD_NBMAX + 1), poff.get(), (size_t)nsegs * (ZKD_NBMAX + 1) * sizeof(uint32_t));
        for (size_t i = (size_t)(hi - lo); i < ncand; i++) if (cand[i] != ZKF_POISON || part[i] != ZKF_POISON) rc = -2;
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
    const uint64_t frame_max = frame_size < n ? frame_size : n;
    if (!zke_ldm_in_frame(level, 0, frame_max)) return -1;
    // zk_enc_far_history (zk_engine_enc.hip): "ldm.inframe = 1; ldm.frame_size = frame_size; ldm.n_total = a.n; ldm.log = zke_ldm_log(frame_max)"
    ZkEncLdm ldm = {nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, nullptr, 0, 0};
    ldm.inframe = 1; ldm.frame_size = frame_size; ldm.n_total = n; ldm.log = zke_ldm_log(frame_max);
    const size_t entries = (size_t)pl.nf << ldm.log;
    if (entries > table_cap) return -1;
    const auto src = zkf_copy(src_in, n);
    const auto table = zkf_exact<uint32_t>(entries);
    emu_set_lane_order(descending != 0);
    // zk_launch_enc_ldm_build_frames (zk_encode.hip): "hipMemsetAsync(table, 0xFF, (nframes * sizeof(uint32_t)) << ldm.log)", "wgs = (ldm.frame_size + 4095) / 4096",
    // launches of at most 65535 frames: "dim3(wgs < 1024 ? wgs : 1024, cnt), dim3(256), ..., src, ldm, table, f0"
    memset(table.get(), 0xFF, entries * sizeof(uint32_t));
    const uint64_t wgs = ((uint64_t)ldm.frame_size + 4095) / 4096;
    const uint32_t gx = (uint32_t)(wgs < 1024 ? wgs : 1024);
    for (uint32_t f0 = 0; f0 < pl.nf; f0 += 65535u) {
        const uint32_t cnt = pl.nf - f0 < 65535u ? pl.nf - f0 : 65535u;
        for (uint32_t by = 0; by < cnt; by++)
            for (uint32_t bx = 0; bx < gx; bx++)
                emu_run_workgroup(256, bx, [&]() { zk_k_enc_ldm_build_frames(src.get(), ldm, table.get(), f0); }, gx, by, cnt);
    }
    emu_set_lane_order(false);
    memcpy(table_out, table.get(), entries * sizeof(uint32_t));
    return (int)ldm.log;
}

// LDM_PREFIX: zk_k_enc_ldm_build over the launcher's grid.  The device copy of the prefix has ZKE_LDM_SLACK readable bytes behind it; so
// has the copy here, and not one more.  table_out: 1 << log entries.  Returns log; -1: the ring holds this prefix, no table.
extern "C" int zk_enc_far_sim_ldm_prefix(const uint8_t *prefix, uint64_t prefix_len, int descending, uint32_t *table_out, uint64_t table_cap)
{
    if (prefix_len <= ZKE_WINDOW) return -1;
    // zk_enc_far_history (zk_engine_enc.hip): "usable = zke_ldm_usable(a.prefix_len); ldm.pfx = a.d_prefix; ldm.plen = a.prefix_len; ldm.u0 = a.prefix_len - usable;
    // ldm.log = zke_ldm_log(usable)"
    const uint64_t usable = zke_ldm_usable(prefix_len);
    ZkEncLdm ldm = {nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, nullptr, 0, 0};
    ldm.plen = prefix_len; ldm.u0 = prefix_len - usable; ldm.log = zke_ldm_log(usable);
    const size_t entries = (size_t)1 << ldm.log;
    if (entries > table_cap) return -1;
    const auto pcopy = zkf_exact<uint8_t>((size_t)prefix_len + ZKE_LDM_SLACK);
    memcpy(pcopy.get(), prefix, (size_t)prefix_len);
    memset(pcopy.get() + prefix_len, 0xA5, ZKE_LDM_SLACK);
    ldm.pfx = pcopy.get();
    const auto table = zkf_exact<uint32_t>(entries);
    emu_set_lane_order(descending != 0);
    // zk_launch_enc_ldm_build (zk_encode.hip): "hipMemsetAsync(table, 0xFF, sizeof(uint32_t) << ldm.log)", "n = ldm.plen - ldm.u0, wgs = (n + 1023) / 1024",
    // "dim3(wgs < 4096 ? wgs : 4096), dim3(256), ..., ldm, table"
    memset(table.get(), 0xFF, entries * sizeof(uint32_t));
    const uint64_t nn = ldm.plen - ldm.u0, wgs = (nn + 1023) / 1024;
    const uint32_t gx = (uint32_t)(wgs < 4096 ? wgs : 4096);
    for (uint32_t bx = 0; bx < gx; bx++)
        emu_run_workgroup(256, bx, [&]() { zk_k_enc_ldm_build(ldm, table.get()); }, gx);
    emu_set_lane_order(false);
    memcpy(table_out, table.get(), entries * sizeof(uint32_t));
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
    // zk_enc_layout (zk_engine_enc.hip): the records take nf * (hist + frame_size) bytes;
    // "zk_launch_enc_stage_hist(st, L.src, a.d_prefix + (a.prefix_len - hist), L.d_frames, L.pl.nf, stage)" = "dim3(nframes), dim3(256)"
    const size_t bytes = (size_t)pl.nf * ((size_t)hist + frame_size);
    if (bytes > stage_cap) return -1;
    const auto src = zkf_copy(src_in, n), pre = zkf_copy(prefix, prefix_len);
    const auto stage = zkf_exact<uint8_t>(bytes);
    memset(stage.get(), 0xA5, bytes);
    for (uint32_t f = 0; f < pl.nf; f++)
        emu_run_workgroup(256, f, [&]() { zk_k_enc_stage_hist(src.get(), pre.get() + (prefix_len - hist), frames.data(), stage.get()); }, pl.nf);
    memcpy(stage_out, stage.get(), bytes);
    return (int)hist;
}

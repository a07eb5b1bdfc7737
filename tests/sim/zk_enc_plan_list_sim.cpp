// zk_enc_plan_list_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// An encode over a caller-given frame list (zk_encode_frame_list*) on the CPU: the list forms of the plan (zk_enc_plan.h), the plan kernels
// (zk_enc_plan_dev.h), the far-history kernels (zk_enc_far.h) and the match kernel (zk_enc_match.h) -- the very sources hipcc compiles --
// one workgroup at a time under the fiber emulator of hip_wg_emu.h, with the launchers' grids, the engine's slices and its buffer sizes out of
// the functions zk_enc_far_history and zk_enc_match call themselves (zk_enc_sched.h).  tests/test_enc_plan_list.py compares what they leave
// with the host plan, record by record, and with the CPU twin frame by frame; tests/sim/enc_plan_list_san.cpp runs the same under
// AddressSanitizer + UBSan.  Every buffer a kernel sees is a heap allocation of EXACTLY the engine's size, poisoned first.
#include "zk_enc_match_emu.h"
#include "../../zeekstd_amd/csrc/zk_enc_far.h"
#include "../../zeekstd_amd/csrc/zk_enc_plan_dev.h"
#include <memory>

constexpr uint32_t ZKL_POISON = 0xA5A5A5A5u;
template <class T> static std::unique_ptr<T[]> zkl_exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

struct ZklPlan {
    ZkEncPlan pl;
    std::vector<ZkEncFrame> frames, segs;
    std::vector<ZkEncBlock> blocks;
    std::vector<uint64_t> doff;
};
static void zkl_alloc(ZklPlan &p)
{
    ZkEncFrame zf; memset(&zf, 0xEE, sizeof zf);
    ZkEncBlock zb; memset(&zb, 0xEE, sizeof zb);
    p.frames.assign(p.pl.nf, zf); p.segs.assign(p.pl.nseg + 1, zf); p.blocks.assign(p.pl.nb + 1, zb); p.doff.assign((size_t)p.pl.nf + 1, 0xEEEEEEEEEEEEEEEEull);
}
static bool zkl_host_plan(const uint64_t *off, uint32_t count, int level, uint64_t prefix_len, ZklPlan &p)
{
    if (!zke_plan_count_list(off, count, zke_prefix_hist(prefix_len), &p.pl)) return false;
    zkl_alloc(p);
    zke_plan_fill_list(off, level, prefix_len, &p.pl, p.frames.data(), p.blocks.data(), p.segs.data(), p.doff.data());
    return true;
}
// 0: the same records and totals; else which array differs first (1 counts, 2 frames, 3 blocks, 4 segments, 5 offsets)
static int zkl_same(const ZklPlan &a, const ZklPlan &b)
{
    if (memcmp(&a.pl, &b.pl, sizeof a.pl)) return 1;
    if (a.pl.nf && memcmp(a.frames.data(), b.frames.data(), (size_t)a.pl.nf * sizeof(ZkEncFrame))) return 2;
    if (a.pl.nb && memcmp(a.blocks.data(), b.blocks.data(), (size_t)a.pl.nb * sizeof(ZkEncBlock))) return 3;
    if (a.pl.nseg && memcmp(a.segs.data(), b.segs.data(), (size_t)a.pl.nseg * sizeof(ZkEncFrame))) return 4;
    if (memcmp(a.doff.data(), b.doff.data(), ((size_t)a.pl.nf + 1) * 8)) return 5;
    return 0;
}

// zke_plan_fill_list on the equal sizes of (n, frame_size) against zke_plan_fill: 0 when frames, blocks, segments, offsets and totals are the
// same bytes.  `base`: what the list's first offset is (the records must not depend on it).
extern "C" int zk_plan_list_sim_equal(uint64_t n, uint32_t frame_size, int level, uint64_t prefix_len, uint64_t base)
{
    ZklPlan u, l;
    if (!zke_plan_count(n, frame_size, zke_prefix_hist(prefix_len), &u.pl)) return -1;
    zkl_alloc(u);
    zke_plan_fill(n, frame_size, level, prefix_len, &u.pl, u.frames.data(), u.blocks.data(), u.segs.data(), u.doff.data());
    std::vector<uint64_t> off((size_t)u.pl.nf + 1);
    for (uint32_t f = 0; f <= u.pl.nf; f++) off[f] = base + ((uint64_t)f * frame_size < n ? (uint64_t)f * frame_size : n);
    if (!zkl_host_plan(off.data(), u.pl.nf, level, prefix_len, l)) return -1;
    return zkl_same(u, l);
}

// The plan kernels (zk_launch_enc_plan_scan: one workgroup of ZKP_SCAN_THREADS; zk_launch_enc_plan_fill: a lane per frame, workgroups of 256)
// against zke_plan_fill_list: 0 when every record, the offsets and the totals agree; 10 + k: the blocks or segments counted in front of frame k are
// not the host's (reported before the fill, which writes where the sums say).
extern "C" int zk_plan_list_sim_dev(const uint64_t *off_in, uint32_t count, int level, uint64_t prefix_len, int descending)
{
    ZklPlan h, d;
    if (!count || !zkl_host_plan(off_in, count, level, prefix_len, h)) return -1;
    const uint32_t hist = zke_prefix_hist(prefix_len);
    const auto off = zkl_exact<uint64_t>((size_t)count + 1);
    memcpy(off.get(), off_in, ((size_t)count + 1) * 8);
    const auto sums = zkl_exact<ZkEncPlanSum>((size_t)count + 1);
    memset(sums.get(), 0xA5, ((size_t)count + 1) * sizeof(ZkEncPlanSum));
    emu_set_lane_order(descending != 0);
    emu_run_workgroup(ZKP_SCAN_THREADS, 0, [&]() { zk_k_enc_plan_scan(off.get(), count, hist ? 1u : 0u, sums.get()); }, 1);
    // (the fill writes a frame's blocks and segments where its sums say: those two are checked before it runs, the rest by the records)
    for (uint32_t f = 0, nseg = 0; f < count; f++) {
        if (sums[f].nb != h.frames[f].block_base || sums[f].nseg != nseg) { emu_set_lane_order(false); return 10 + (int)f; }
        nseg += (h.frames[f].d_size + ZKE_SEGMENT - 1) / ZKE_SEGMENT;
    }
    const ZkEncPlanSum t = sums[count];
    d.pl = ZkEncPlan{count, t.nb, t.nseg, hist, t.seq, t.scratch};
    if (memcmp(&d.pl, &h.pl, sizeof d.pl)) { emu_set_lane_order(false); return 1; }
    zkl_alloc(d);
    const uint32_t wgs = (count + 255) / 256;
    for (uint32_t b = 0; b < wgs; b++)
        emu_run_workgroup(256, b, [&]() { zk_k_enc_plan_fill(off.get(), count, level, prefix_len, hist, sums.get(), d.frames.data(), d.blocks.data(), d.segs.data(), d.doff.data()); }, wgs);
    emu_set_lane_order(false);
    return zkl_same(h, d);
}

// the host pipeline's chunks of a list (zke_list_chunk_end): cuts_out[k] = first frame of chunk k, then count; returns the number of chunks
extern "C" int zk_plan_list_sim_chunks(const uint64_t *off, uint32_t count, uint64_t min_bytes, uint32_t min_frames, uint64_t max_bytes, uint32_t *cuts_out, uint32_t cap)
{
    uint32_t k = 0;
    for (uint32_t f0 = 0; f0 < count;) {
        if (k + 1 >= cap) return -1;
        cuts_out[k++] = f0;
        const uint32_t f1 = zke_list_chunk_end(off, count, f0, min_bytes, min_frames, max_bytes);
        if (f1 <= f0 || f1 > count) return -2;
        f0 = f1;
    }
    cuts_out[k] = count;
    return (int)k;
}

// One encode's far history and match pass over the list off[count + 1] of src (no prefix), as zk_enc_far_history and zk_enc_match run them:
// the sampled tables of the frames that qualify (zk_k_enc_ldm_build_frames, list form), then slice after slice of whole frames (slice_bytes:
// what ZK_CHOICE_ENC_DENSE_SLICE_KIB sets, 0 = 4 GiB) the dense kernels and the match kernel.
//   lf_out[3 * k] = (start, first entry in table_out, size) of the k-th frame with a table; table_out[table_cap]; cand_out[n] (zeros where the
//   call has no dense history); per block b in plan order blk_nseq / blk_nlit / blk_bsz / seq_at / lit_at, seqs, lits as zk_enc_sim_match.
// with_match = 0 stops before the match kernel.  Returns the number of blocks; -1: an output is too small; -2: a dense kernel wrote into its slack.
extern "C" int zk_plan_list_sim_encode(const uint8_t *src_in, const uint64_t *off, uint32_t count, int level, uint64_t slice_bytes, int descending, int with_match,
                                       uint64_t *lf_out, uint32_t lf_cap, uint32_t *nlf_out, uint32_t *table_out, uint64_t table_cap, uint32_t *cand_out,
                                       uint32_t blk_cap, uint32_t *blk_nseq, uint32_t *blk_nlit, uint32_t *blk_bsz, uint64_t *seq_at, uint64_t *lit_at,
                                       uint64_t *seqs_out, uint64_t seq_cap, uint8_t *lits_out, uint64_t lit_cap)
{
    ZklPlan p;
    if (!count || !zkl_host_plan(off, count, level, 0, p)) return -1;
    const ZkEncPlan &pl = p.pl;
    const uint64_t n = off[count] - off[0];
    if (pl.nb > blk_cap || pl.seq_total + 1 > seq_cap || n > lit_cap) return -1;
    uint32_t frame_max = 1;                     // (what the entry point hands on as frame_size: the largest frame, at least 1)
    for (uint32_t f = 0; f < count; f++) if (p.frames[f].d_size > frame_max) frame_max = p.frames[f].d_size;
    const ZkEncCut cut = {off, count, n, frame_max};
    const ZkEncFarPlan fp = zk_enc_far_plan(cut, level, 0, 0, pl.nseg, slice_bytes);
    const auto src = zkl_exact<uint8_t>(n);
    if (n) memcpy(src.get(), src_in + off[0], n);
    ZkEncLdm ldm = fp.ldm;
    std::unique_ptr<ZkEncLdmFrame[]> lf;
    std::unique_ptr<uint32_t[]> table, cand, part, poff;
    const size_t ncand = fp.cand_words;
    *nlf_out = 0;
    emu_set_lane_order(descending != 0);
    if (fp.kind == ZK_ENC_FAR_INFRAME) {
        const uint32_t nlf = ldm.nlf;
        if (nlf > lf_cap || fp.entries > table_cap) { emu_set_lane_order(false); return -1; }
        lf = zkl_exact<ZkEncLdmFrame>(nlf);
        zk_enc_far_list_frames(cut, level, 0, lf.get());
        table = zkl_exact<uint32_t>((size_t)fp.entries);
        memset(table.get(), 0xFF, fp.table_bytes);
        ldm.lf = lf.get();
        for (uint32_t f0 = 0; f0 < nlf; f0 += ZK_ENC_GRID_Y_MAX) {
            const uint32_t gx = fp.build_gx, cnt = zk_enc_ldm_frames_gy(nlf, f0);
            for (uint32_t by = 0; by < cnt; by++)
                for (uint32_t bx = 0; bx < gx; bx++)
                    emu_run_workgroup(256, bx, [&]() { zk_k_enc_ldm_build_frames(src.get(), ldm, table.get(), f0); }, gx, by, cnt);
        }
        ldm.table = table.get();
        for (uint32_t k = 0; k < nlf; k++) { lf_out[3 * k] = lf[k].start; lf_out[3 * k + 1] = lf[k].tbase; lf_out[3 * k + 2] = lf[k].size; }
        *nlf_out = nlf;
        memcpy(table_out, table.get(), fp.table_bytes);
        if (fp.dense_span) {
            cand = zkl_exact<uint32_t>(ncand); part = zkl_exact<uint32_t>(ncand); poff = zkl_exact<uint32_t>(fp.poff_words);
            ldm.dense = cand.get();
        }
    }
    memset(cand_out, 0, (size_t)n * sizeof(uint32_t));
    const auto seqs = zkl_exact<uint64_t>(pl.seq_total + 1);
    const auto lits = zkl_exact<uint8_t>(n + 64);
    int rc = (int)pl.nb;
    for (uint32_t f0 = 0, s0 = 0; f0 < count;) {
        const ZkEncSlice end = zk_enc_slice_end(cut, 0, n, fp.slice_cap, pl.nseg, f0, s0);
        const uint64_t lo = p.doff[f0], hi = p.doff[end.f1];
        const uint32_t nsegs = end.s1 - s0;
        const ZkEncFrame *sg = p.segs.data() + s0;
        ZkEncLdm sl = ldm;
        if (sl.dense && nsegs) {
            for (size_t i = 0; i < ncand; i++) cand[i] = part[i] = ZKL_POISON;
            sl.dense = cand.get() - lo;
            for (uint32_t b = 0; b < nsegs; b++)
                emu_run_workgroup(1024, b, [&]() { zk_k_enc_dense_part(src.get(), sg, sl, part.get() - lo, poff.get()); }, nsegs);
            for (uint32_t b = 0; b < nsegs; b++)
                emu_run_workgroup(1024, b, [&]() { zk_k_enc_dense_cand(src.get(), sg, sl, part.get() - lo, poff.get(), cand.get() - lo); }, nsegs);
            memcpy(cand_out + lo, cand.get(), (size_t)(hi - lo) * sizeof(uint32_t));
            for (size_t i = (size_t)(hi - lo); i < ncand; i++) if (cand[i] != ZKL_POISON || part[i] != ZKL_POISON) rc = -2;
        }
        if (with_match) zk_emu_enc_match(src.get(), sg, nsegs, p.blocks.data(), seqs.get(), lits.get(), level, sl);
        f0 = end.f1; s0 = end.s1;
    }
    emu_set_lane_order(false);
    if (with_match) {
        zk_emu_enc_blocks_out(p.blocks.data(), pl.nb, blk_nseq, blk_nlit, blk_bsz, seq_at, lit_at);
        memcpy(seqs_out, seqs.get(), (size_t)(pl.seq_total + 1) * 8);
        memcpy(lits_out, lits.get(), (size_t)n);
    }
    return rc;
}

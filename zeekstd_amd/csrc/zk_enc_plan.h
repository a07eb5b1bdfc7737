// zk_enc_plan.h -- host arithmetic of one encode: where the frames, their blocks and the matcher's segments lie.
// Frame boundaries are the policy's (lib/src/encode.rs:528-544, FrameSizePolicy::Uncompressed: frame i covers input bytes
// [i * L, min((i + 1) * L, n))); blocks and segments are this engine's own cut (zk_enc_device.h).  Used by the engine
// (zk_engine_enc.hip) and by the CPU emulation of the match kernel (tests/sim/zk_enc_sim.cpp).
#pragma once
#include <stdint.h>
#include <string.h>
#include "zk_enc_device.h"

struct ZkEncPlan {
    uint32_t nf, nb, nseg;                  // frames, blocks, matcher segments
    uint32_t hist;                          // bytes of prefix laid out before every frame in the matcher's source (a multiple of 4)
    uint64_t seq_total, scratch_total;      // entries of the sequence buffer, bytes of the entropy stage's scratch
};

// bytes of a prefix the matcher can reach: its window, rounded down to a multiple of 4 (a lane takes four positions out of
// aligned ring words, so every record starts on a word)
inline uint32_t zke_prefix_hist(uint64_t prefix_len) { return (uint32_t)(prefix_len < ZKE_WINDOW ? prefix_len : ZKE_WINDOW) & ~3u; }

// counts only; false: too many blocks / segments for 32-bit indices
inline bool zke_plan_count(uint64_t n, uint32_t frame_size, uint32_t hist, ZkEncPlan *pl)
{
    const uint64_t nf64 = n == 0 ? 1 : (n + frame_size - 1) / frame_size;
    uint64_t nb64 = 0, nseg64 = 0;
    // all frames but the last have the same size
    const uint64_t last = n - (nf64 - 1) * (uint64_t)frame_size;
    for (int w = 0; w < 2; w++) {
        const uint64_t cnt = w == 0 ? nf64 - 1 : 1, dsz = w == 0 ? frame_size : last;
        if (!cnt || !dsz) continue;
        const uint32_t bm = zke_block_max((uint32_t)dsz, hist != 0);
        nb64 += cnt * ((dsz + bm - 1) / bm);
        nseg64 += cnt * ((dsz + ZKE_SEGMENT - 1) / ZKE_SEGMENT);
    }
    if (nb64 > 0xFFFFFFF0ull || nseg64 > 0xFFFFFFF0ull || nf64 > 0xFFFFFFF0ull) return false;
    pl->nf = (uint32_t)nf64; pl->nb = (uint32_t)nb64; pl->nseg = (uint32_t)nseg64; pl->hist = hist;
    pl->seq_total = 0; pl->scratch_total = 0;
    return true;
}

// One frame's records: frames[f], its blocks from blocks[*bcount] on, its segments from segs[*sc] on; the running totals go on.
// Both fills below are loops over this, so a list of equal sizes and the uniform cut give the same records.
ZK_HD void zke_plan_frame(uint32_t f, uint64_t src_off, uint32_t d_size, uint64_t m_off, int level, uint64_t prefix_len, uint32_t hist, ZkEncFrame *frames,
                           ZkEncBlock *blocks, ZkEncFrame *segs, uint32_t *bcount, uint32_t *sc, uint64_t *seq_total, uint64_t *scratch_total)
{
    ZkEncFrame &fr = frames[f];
    fr.src_off = src_off;
    fr.d_size = d_size;
    uint32_t wlog = 10;
    while ((1u << wlog) < fr.d_size && wlog < 17) wlog++;
    if (hist) wlog = 17;                                 // covers every offset the matcher can produce, into the prefix too
    if (hist && prefix_len > ZKE_WINDOW) while ((1ull << wlog) < prefix_len + fr.d_size && wlog < 27) wlog++;   // long-distance offsets: < 2^27
    if (zke_ldm_in_frame(level, prefix_len, fr.d_size)) while ((1ull << wlog) < fr.d_size && wlog < 27) wlog++;     // in-frame far history: the window covers the frame
    fr.window_log = wlog;
    fr.block_max = zke_block_max(fr.d_size, hist != 0);
    fr.n_blocks = fr.d_size ? (fr.d_size + fr.block_max - 1) / fr.block_max : 0;
    fr.block_base = *bcount;
    fr.hist = fr.d_size ? hist : 0;
    fr.m_off = m_off;
    fr.minmatch = zke_minmatch2(level, prefix_len); fr.seg_at = 0;
    for (uint32_t b = 0; b < fr.n_blocks; b++) {
        ZkEncBlock &k = blocks[(*bcount)++];
        memset(&k, 0, sizeof k);
        k.frame = f; k.bs = b * fr.block_max;
        k.bsz = fr.d_size - k.bs < fr.block_max ? fr.d_size - k.bs : fr.block_max;
        k.seq_base = *seq_total; *seq_total += k.bsz / 4 + 2;
        k.lit_base = fr.src_off + k.bs;
        k.scratch_base = *scratch_total;
        const uint32_t q = (k.bsz + 3) / 4;
        *scratch_total += ZKE_SMALL + 4ull * (q + (q >> 1) + 16) + (uint64_t)k.bsz + 64;   // small parts, 4 literal streams, the sequence bitstream + its slack
    }
    const uint32_t per = ZKE_SEGMENT / fr.block_max;      // blocks per segment (frames above ZKE_SEGMENT have 16 or 32 KiB blocks)
    for (uint32_t at = 0; at < fr.d_size; at += ZKE_SEGMENT) {
        ZkEncFrame &sg = segs[(*sc)++];
        sg = fr;
        sg.d_size = fr.d_size - at < ZKE_SEGMENT ? fr.d_size - at : ZKE_SEGMENT;
        sg.n_blocks = (sg.d_size + fr.block_max - 1) / fr.block_max;
        sg.block_base = fr.block_base + (at / ZKE_SEGMENT) * per;
        sg.seg_at = at;
        if (at) { sg.hist = ZKE_WINDOW; sg.m_off = fr.m_off + fr.hist + at - ZKE_WINDOW; }
    }
}

// frames[nf], blocks[nb], segs[nseg] (a segment record is a ZkEncFrame that covers <= ZKE_SEGMENT bytes of its frame:
// d_size / n_blocks / block_base are the segment's, hist / m_off its history), doff[nf + 1] (may be null)
// prefix_len: the whole prefix (0: none); above ZKE_WINDOW the matcher also finds long-distance matches into it
// (ZkEncLdm) and the frames' windows cover prefix + frame
inline void zke_plan_fill(uint64_t n, uint32_t frame_size, int level, uint64_t prefix_len, ZkEncPlan *pl, ZkEncFrame *frames, ZkEncBlock *blocks, ZkEncFrame *segs, uint64_t *doff)
{
    const uint32_t hist = pl->hist;
    uint64_t seq_total = 0, scratch_total = 0;
    uint32_t bcount = 0, sc = 0;
    for (uint32_t f = 0; f < pl->nf; f++) {
        const uint64_t src_off = (uint64_t)f * frame_size;
        const uint32_t d_size = (uint32_t)(n - src_off < frame_size ? n - src_off : frame_size);
        zke_plan_frame(f, src_off, d_size, hist ? (uint64_t)f * ((uint64_t)hist + frame_size) : src_off, level, prefix_len, hist, frames, blocks, segs, &bcount, &sc, &seq_total, &scratch_total);
        if (doff) doff[f] = src_off;
    }
    if (doff) doff[pl->nf] = n;
    pl->seq_total = seq_total; pl->scratch_total = scratch_total;
}

// ---- a caller-given frame list: off[count + 1] non-decreasing prefix sums, frame i = source bytes [off[i] - off[0], off[i + 1] - off[0]); every
// frame is at most a uint32_t (the entry points check the list before they plan).  count >= 1.
inline bool zke_plan_count_list(const uint64_t *off, uint32_t count, uint32_t hist, ZkEncPlan *pl)
{
    uint64_t nb64 = 0, nseg64 = 0;
    for (uint32_t f = 0; f < count; f++) {
        const uint64_t dsz = off[f + 1] - off[f];
        if (!dsz) continue;
        const uint32_t bm = zke_block_max((uint32_t)dsz, hist != 0);
        nb64 += (dsz + bm - 1) / bm;
        nseg64 += (dsz + ZKE_SEGMENT - 1) / ZKE_SEGMENT;
    }
    if (nb64 > 0xFFFFFFF0ull || nseg64 > 0xFFFFFFF0ull || count > 0xFFFFFFF0ull) return false;
    pl->nf = count; pl->nb = (uint32_t)nb64; pl->nseg = (uint32_t)nseg64; pl->hist = hist;
    pl->seq_total = 0; pl->scratch_total = 0;
    return true;
}
// the records of zke_plan_fill for the list's frames; the [history | frame] records of prefix mode follow one another, so m_off is a running
// sum of hist + size.
inline void zke_plan_fill_list(const uint64_t *off, int level, uint64_t prefix_len, ZkEncPlan *pl, ZkEncFrame *frames, ZkEncBlock *blocks, ZkEncFrame *segs, uint64_t *doff)
{
    const uint32_t hist = pl->hist;
    uint64_t seq_total = 0, scratch_total = 0, m_off = 0;
    uint32_t bcount = 0, sc = 0;
    for (uint32_t f = 0; f < pl->nf; f++) {
        const uint64_t src_off = off[f] - off[0];
        const uint32_t d_size = (uint32_t)(off[f + 1] - off[f]);
        zke_plan_frame(f, src_off, d_size, hist ? m_off : src_off, level, prefix_len, hist, frames, blocks, segs, &bcount, &sc, &seq_total, &scratch_total);
        m_off += (uint64_t)hist + d_size;
        if (doff) doff[f] = src_off;
    }
    if (doff) doff[pl->nf] = off[pl->nf] - off[0];
    pl->seq_total = seq_total; pl->scratch_total = scratch_total;
}

// ---- the same plan made on the device (zk_enc_plan_dev.h has the kernels): what the host and the kernels share
struct ZkEncPlanSum {
    uint64_t seq, scratch;      // entries of the sequence buffer, bytes of the entropy stage's scratch
    uint32_t nb, nseg;          // blocks, matcher segments
};
static_assert(sizeof(ZkEncPlanSum) == 24, "three words on their way to the host");
ZK_HD ZkEncPlanSum zke_plan_sum_add(ZkEncPlanSum a, const ZkEncPlanSum &b) { a.seq += b.seq; a.scratch += b.scratch; a.nb += b.nb; a.nseg += b.nseg; return a; }
// what zke_plan_frame adds to the running totals for a frame of d_size bytes: all its blocks but the last are block_max bytes
ZK_HD ZkEncPlanSum zke_plan_frame_sum(uint64_t d_size64, bool prefix)
{
    ZkEncPlanSum s = {0, 0, 0, 0};
    // (the scan may run before the host has checked the list: a size no frame can have counts as the largest, the totals are dropped then)
    const uint32_t d_size = (uint32_t)(d_size64 < 0x40000000ull ? d_size64 : 0x40000000ull);
    if (!d_size) return s;
    const uint32_t bm = zke_block_max(d_size, prefix), nb = (d_size + bm - 1) / bm, last = d_size - (nb - 1) * bm;
    const uint32_t qf = (bm + 3) / 4, ql = (last + 3) / 4;
    s.nb = nb; s.nseg = (d_size + ZKE_SEGMENT - 1) / ZKE_SEGMENT;
    s.seq = (uint64_t)(nb - 1) * (bm / 4 + 2) + (last / 4 + 2);
    s.scratch = (uint64_t)(nb - 1) * (ZKE_SMALL + 4ull * (qf + (qf >> 1) + 16) + (uint64_t)bm + 64) + (ZKE_SMALL + 4ull * (ql + (ql >> 1) + 16) + (uint64_t)last + 64);
    return s;
}

// ZK_CHOICE_ENC_PLAN = 0: lists of at least this many frames are planned on the device.  profiles/frame_list_probe.txt (tools/frame_list_probe.py):
// the device plan is the faster one at every count measured, from 1000 records (0.03 of 0.31 ms) to half a million (3.4 of 38 ms); nothing
// smaller was measured, so nothing smaller is switched.
constexpr uint32_t ZK_ENC_PLAN_DEV_FRAMES = 1000;

// The host pipeline's chunks of a frame list: whole frames from f0 on until the chunk has min_bytes and min_frames, never past max_bytes
// (but never less than a frame); a rest of at most a quarter of the chunk goes with it if that fits, so that no short chunk ends the call.
// Returns the first frame of the next chunk.  (The uniform cut's targets by bytes: 256 MiB, 128 frames, 2 GiB.)
inline uint32_t zke_list_chunk_end(const uint64_t *off, uint32_t count, uint32_t f0, uint64_t min_bytes, uint32_t min_frames, uint64_t max_bytes)
{
    uint32_t f1 = f0;
    while (f1 < count && (off[f1] - off[f0] < min_bytes || f1 - f0 < min_frames)) {
        if (f1 > f0 && off[f1 + 1] - off[f0] > max_bytes) break;
        f1++;
    }
    const uint64_t have = off[f1] - off[f0], rest = off[count] - off[f1];
    if (f1 < count && rest <= have / 4 && have + rest <= max_bytes) f1 = count;
    return f1;
}

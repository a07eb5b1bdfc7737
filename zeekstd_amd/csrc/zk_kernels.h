// zk_kernels.h -- host-callable launchers of the gfx950 kernels (zk_decode.hip, zk_encode.hip, zk_ranges.hip).  The decode launchers decide
// nothing: which kernel, which template instance and how many blocks or frames per workgroup come in a plan struct of zk_dec_plan.h
// (where ZkKernelChoice lives too), filled by the engine.
#pragma once
#include <hip/hip_runtime.h>
#include "zk_device.h"
#include "zk_dec_plan.h"

// scratch of the segmented executor (zk_engine.hip sizes it; zk_device.h: zk_seg_region)
struct ZkSegScratch { ZkSeg *segs; uint32_t *nsegs, *segn; ZkHole *holes; uint32_t *tilecnt; uint32_t max_segs, seg_bytes; };

// A loaded dictionary as the frame walk sees it (zk_dict.h).  on: one is loaded; id: its Dictionary_ID (0: raw content); def: the index of the
// block entry that describes its tables = the batch's block count (ZK_DEF_NONE: raw content, no tables); tmpl / img (device memory): that
// entry and the "block content" it describes -- the fill pass writes the entry to blocks[def].
struct ZkWalkDict { uint32_t on = 0, id = 0, def = ZK_DEF_NONE; const ZkBlock *tmpl = nullptr; const uint8_t *img = nullptr; };
struct ZkRepInit { uint32_t r[3]; };                     // the repeat offsets a frame starts with (zk_k_exec with a prefix)
void zk_launch_walk(hipStream_t st, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, const uint64_t *d_off, uint32_t first,
                    uint32_t count, const uint32_t *ids, const uint64_t *out_off, uint64_t dst_cap, const ZkFrameBase *bases, ZkBlock *blocks, ZkFrameInfo *infos,
                    const ZkWalkDict &wd = ZkWalkDict());
void zk_launch_frame_sizes(hipStream_t st, const ZkFrameInfo *infos, const ZkFrameBase *bases, const ZkBlock *blocks, uint32_t count, uint64_t *sizes, int32_t *status_out);
void zk_launch_scan(hipStream_t st, const ZkFrameInfo *infos, uint32_t count, ZkFrameBase *bases, uint64_t *totals, const uint64_t *d_off, uint32_t first, const uint64_t *out_off);
void zk_launch_huf(hipStream_t st, const uint8_t *comp, ZkBlock *blocks, uint32_t nblocks, uint8_t *lit);
// the sequences of a batch: p.quads / p.shared, then p.rest (p.fused is the caller's: zk_launch_entropy in place of zk_launch_huf || zk_launch_fse)
void zk_launch_fse(hipStream_t st, const uint8_t *comp, ZkBlock *blocks, uint32_t nblocks, ZkSeqP *seqs, const ZkEntropyPlan &p);
// zk_k_entropy_frame, then p.rest
void zk_launch_entropy(hipStream_t st, const uint8_t *comp, ZkBlock *blocks, uint32_t nblocks, ZkSeqP *seqs, uint8_t *lit, const ZkEntropyPlan &p);
void zk_launch_exec(hipStream_t st, const uint8_t *comp, const uint64_t *d_off, uint32_t first, uint32_t count,
                    const uint32_t *ids, const uint64_t *out_off, const ZkBlock *blocks, const ZkFrameBase *bases, ZkFrameInfo *infos, const ZkSeqP *seqs,
                    const uint8_t *lit, uint8_t *dst, const uint8_t *prefix, uint64_t plen, const ZkExecPlan &p,      // p: planned with has_prefix = prefix && plen
                    uint64_t *progress = nullptr,       // progress: one word per frame for zk_launch_xxh64_follow (zk_decode.hip: zk_publish)
                    const uint32_t *rep_init = nullptr); // with a prefix: the three repeat offsets every frame starts with (a dictionary's; nullptr = 1 / 4 / 8)
void zk_launch_exec_seg(hipStream_t st, const uint8_t *comp, const uint64_t *d_off, uint32_t first, uint32_t count,
                        const uint32_t *ids, const uint64_t *out_off, const ZkBlock *blocks, const ZkFrameBase *bases, ZkFrameInfo *infos, const ZkSeqP *seqs,
                        const uint8_t *lit, uint8_t *dst, const ZkSegScratch &sg, const ZkExecSegPlan &p, uint64_t *progress = nullptr);
// skip (the progress words zk_launch_xxh64_follow left): frames marked there are done -- the plan was made with skip = true
void zk_launch_xxh64(hipStream_t st, const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count,
                     ZkFrameInfo *infos, uint64_t *hashes, const ZkXxhPlan &p, const uint64_t *skip = nullptr);
// the checksums beside the executor that publishes `progress` (launched on another queue); frames it verifies are marked in `progress`,
// zk_launch_xxh64(..., skip = progress) behind the executor takes the rest
void zk_launch_xxh64_follow(hipStream_t st, const uint8_t *data, const uint64_t *d_off, uint32_t first, uint32_t count, const ZkFrameInfo *infos, uint64_t *progress,
                            const ZkXxhFollowPlan &p);
void zk_launch_status(hipStream_t st, const ZkFrameInfo *infos, uint32_t count, int32_t *status_out, uint64_t *first_err,
                      const uint64_t *progress = nullptr, uint64_t *followed = nullptr);

// small batches (a seek): no host round trip, no copy commands -- see zk_decode.hip
void zk_launch_small_walk(hipStream_t st, const uint8_t *h_comp, uint64_t comp_bytes, const uint64_t *h_offs, uint32_t count, uint64_t dst_cap,
                          uint32_t block_cap, uint64_t seq_cap, uint8_t *d_comp, uint64_t *d_offs, ZkFrameInfo *infos, ZkFrameBase *bases, ZkBlock *blocks, uint64_t *words);
void zk_launch_small_entropy(hipStream_t st, const uint8_t *comp, ZkBlock *blocks, const uint64_t *words, uint8_t *lit, ZkSeqP *seqs, uint32_t groups, bool split);
void zk_launch_small_publish(hipStream_t st, const ZkFrameInfo *infos, const uint64_t *d_offs, uint32_t count, const uint8_t *dst, uint8_t *h_out,
                             int32_t *d_status, int32_t *h_status, uint64_t *words, uint32_t *h_flag, uint32_t gen);

// ---- encoder (zk_encode.hip)
#include "zk_enc_device.h"
struct ZkEncDictDev; struct ZkEncDictId;                // zk_enc_dict.h; a null pointer = the launch of every route without a formatted dictionary
struct ZkEncPlanSum;
void zk_launch_enc_plan_scan(hipStream_t st, const uint64_t *d_off, uint32_t count, bool prefix, ZkEncPlanSum *sums);
void zk_launch_enc_plan_fill(hipStream_t st, const uint64_t *d_off, uint32_t count, int level, uint64_t prefix_len, uint32_t hist, const ZkEncPlanSum *sums,
                             ZkEncFrame *frames, ZkEncBlock *blocks, ZkEncFrame *segs, uint64_t *doff);
void zk_launch_enc_stage_hist(hipStream_t st, const uint8_t *src, const uint8_t *prefix_tail, const ZkEncFrame *frames, uint32_t nframes, uint8_t *stage);
void zk_launch_enc_match(hipStream_t st, const uint8_t *src, const ZkEncFrame *segs, uint32_t nsegs, ZkEncBlock *blocks, uint64_t *seqs, uint8_t *lits, int level, const ZkEncLdm &ldm);
int zk_launch_enc_ldm_build(hipStream_t st, const ZkEncLdm &ldm, uint32_t *table, size_t table_bytes, uint32_t gx);     // 0, or -1: the table could not be cleared (sizes: ZkEncFarPlan)
// cand, part: an entry per input byte + ZKE_DENSE_SLACK; poff: (ZKE_DENSE_PASSES_MAX + 1) words per segment; every entry that is read is written first: no clear
void zk_launch_enc_dense_cand(hipStream_t st, const uint8_t *src, const ZkEncFrame *segs, uint32_t nsegs, const ZkEncLdm &ldm, uint32_t *cand, uint32_t *part, uint32_t *poff);
int zk_launch_enc_ldm_build_frames(hipStream_t st, const uint8_t *src, const ZkEncLdm &ldm, uint32_t *table, uint32_t nframes, size_t table_bytes, uint32_t gx);
void zk_launch_enc_fse_build(hipStream_t st, const uint8_t *src, const ZkEncFrame *frames, uint32_t nframes, const ZkEncBlock *blocks, uint64_t *seqs, uint32_t *mpos,
                             const ZkEncTables *predef, ZkEncTables *ftab, const ZkEncDictDev *dd = nullptr);
void zk_launch_enc_entropy(hipStream_t st, const uint8_t *src, const ZkEncFrame *frames, ZkEncBlock *blocks, uint32_t nblocks,
                           uint64_t *seqs, uint32_t *mpos, const uint8_t *lits, uint8_t *scratch, const ZkEncTables *ftab,
                           uint32_t nframes = 0, const ZkEncDictDev *dd = nullptr);       // dd: zk_k_enc_dict_lits over the nframes frames' first blocks behind it
void zk_launch_enc_sizes(hipStream_t st, const ZkEncFrame *frames, uint32_t nframes, ZkEncBlock *blocks, const ZkEncTables *ftab, int checksum,
                         uint64_t *c_size64, uint32_t *c_sizes, uint32_t *d_sizes, const ZkEncDictId *did = nullptr);
void zk_launch_scan64(hipStream_t st, const uint64_t *in, uint32_t n, uint64_t *out);
void zk_launch_enc_assemble(hipStream_t st, const uint8_t *src, const ZkEncFrame *frames, uint32_t nframes, const ZkEncBlock *blocks, uint32_t nblocks, const ZkEncTables *ftab,
                            const uint8_t *lits, const uint8_t *scratch, const uint64_t *out_off, const uint64_t *c_size64, const uint64_t *hashes, int checksum, uint8_t *dst,
                            const ZkEncDictId *did = nullptr);

// ---- byte-range reads (zk_ranges.hip; the per-range arithmetic: zk_ranges.h)
struct ZkRangeArgs { const uint64_t *d_off; uint32_t n_frames; const uint64_t *offs, *lens, *dst_off; uint32_t count; void *dst; uint64_t dst_cap; };
struct ZkRangeCopy { uint64_t src, dst, n; };           // n bytes from scratch + src to dst + dst: what one decode pass holds of a range
constexpr uint64_t ZK_RANGE_SMALL = 16u << 10;          // copies up to here are a wave's, longer ones are dealt to workgroups in chunks of
constexpr uint64_t ZK_RANGE_CHUNK = 64u << 10;
// validation, first / last frame per range, the sorted unique touched frames (ids, uoff: n + 1 prefix sums of their sizes; slot: frame -> position) and
// words[0..1] = their number and bytes.  r.dst_off == nullptr: the destinations are packed (prefix sums of the valid lengths, eff -> packed).  cover
// (n_frames + 1 words) must be zero.
void zk_launch_range_plan(hipStream_t st, const ZkRangeArgs &r, uint64_t *eff, uint64_t *packed, uint32_t *rfirst, uint32_t *rlast, int32_t *status, uint32_t *cover,
                          uint32_t *slot, uint32_t *ids, uint64_t *uoff, uint64_t *words);
// zk_k_range_compact alone, over a difference array that somebody else filled (zk_view.hip: the frames a view's touched entries name)
void zk_launch_range_compact(hipStream_t st, const uint64_t *d_off, uint32_t n_frames, const uint32_t *cover, uint32_t *slot, uint32_t *ids, uint64_t *uoff, uint64_t *words);
void zk_launch_range_rebase(hipStream_t st, const uint64_t *uoff, uint32_t a, uint32_t n, uint64_t *poff);
// the pass that holds positions [a, b) of the unique list: one copy per range (copies) and the chunk prefix sums of the large ones (cnt -> coff, count + 1)
void zk_launch_range_pieces(hipStream_t st, const ZkRangeArgs &r, const uint64_t *dst_off, const uint32_t *rfirst, const uint32_t *rlast, const uint32_t *slot,
                            const uint32_t *ids, const uint64_t *uoff, uint32_t a, uint32_t b, ZkRangeCopy *copies, uint64_t *cnt, uint64_t *coff);
void zk_launch_range_gather(hipStream_t st, const uint8_t *scratch, uint8_t *dst, const ZkRangeCopy *copies, const uint64_t *coff, uint32_t count, uint64_t pass_bytes);
void zk_launch_range_status(hipStream_t st, const ZkRangeArgs &r, const uint32_t *rfirst, const uint32_t *rlast, const uint32_t *slot, const int32_t *fstat,
                            bool any_failed, const uint64_t *pass_err, int32_t *status, uint64_t *first_err);

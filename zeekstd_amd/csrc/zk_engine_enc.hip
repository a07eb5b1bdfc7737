// zk_engine_enc.hip -- encode half of the batch engine (Level A of include/zeekstd_amd.h).
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_kernels.h"
#include "zk_enc_plan.h"
#include "zk_enc_sched.h"
#include "zk_enc_dict.h"
#include "zk_dict.h"

// Per frame: header (6) + checksum (4) + a 3-byte header for more blocks than a frame can have.  A frame has one block up to 4 KiB and blocks
// of at least 4 KiB above that (zke_block_max), so ceil(frame_size / 1024) + 8 leaves at least 8 block headers (24 bytes) spare, and three per
// KiB from 4 KiB on.  A raw block is its input, every other block is smaller than its input (zk_k_enc_entropy: total < bsz) -- except the one
// defining block of a frame with >= 256 sequences, which zk_k_enc_sizes grows by the table descriptions (<= 108 bytes at accuracy log 6,
// <= 150 at 9 / 8 / 9).  The spare headers cover those from 37 889 bytes on; below that what the >= 256 sequences save does (DESIGN.md
// 5.2f: argued and measured, not proven; tests/test_encode_bound.py).  zk_host_encode reserves exactly this much: it is not advisory.
extern "C" uint64_t zk_compress_bound(uint64_t n, uint32_t frame_size)
{
    if (frame_size == 0) return 0;
    const uint64_t nf = n == 0 ? 1 : (n + frame_size - 1) / frame_size;
    const uint64_t blocks_per_frame = ((uint64_t)frame_size + 1023) / 1024 + 8;
    return n + nf * (6 + 4 + 3 * blocks_per_frame) + 16;
}

// The dictionary route adds the largest Dictionary_ID field to every frame and nothing else: a block is stored raw unless its compressed form
// is smaller, a dictionary table replaces a description (the one thing that lets a block outgrow its input) and never adds one, and a
// Treeless literals section is taken only where it is smaller than the section it replaces.
extern "C" uint64_t zk_compress_bound_dict(uint64_t n, uint32_t frame_size)
{
    if (frame_size == 0) return 0;
    const uint64_t nf = n == 0 ? 1 : (n + frame_size - 1) / frame_size;
    return zk_compress_bound(n, frame_size) + 4 * nf;
}
// A frame list: the sum of the frames' own bounds, zk_compress_bound(s, max(s, 1)) (+ 4 with a dictionary) = s + 3 * ceil(max(s, 1) / 1024) + 50 (+ 4),
// from above: every ceil is at most s / 1024 + 1, and the sum of the floors at most n / 1024.
extern "C" uint64_t zk_compress_bound_list(uint64_t n, uint32_t count, int with_dictionary)
{
    return n + 3 * (n / 1024) + (uint64_t)(53 + (with_dictionary ? 4 : 0)) * count;
}
uint64_t zk_enc_bound(const zk_enc_args &a)
{
    if (a.list) return zk_compress_bound_list(a.n, a.list_count, a.cdict != nullptr);
    return a.cdict ? zk_compress_bound_dict(a.n, a.frame_size) : zk_compress_bound(a.n, a.frame_size);
}
int zk_enc_list_check(const uint64_t *off, uint32_t count, uint64_t *max_frame)
{
    uint64_t mx = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > ZK_SEEKABLE_MAX_FRAME_SIZE) return ZK_ERR_ARGUMENT;
        if (off[i + 1] - off[i] > mx) mx = off[i + 1] - off[i];
    }
    *max_frame = mx;
    return 0;
}

extern "C" int zk_encode_frames_dev(zk_engine *e, const void *d_src, uint64_t n, uint32_t frame_size, int level, int checksum,
                                    void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint32_t *n_frames_out,
                                    uint64_t *written_out, void *stream)
{
    return zk_encode_frames_prefix_dev(e, d_src, n, frame_size, level, checksum, nullptr, 0, d_dst, dst_cap, d_c_sizes, d_d_sizes,
                                       n_frames_out, written_out, stream);
}

// ---------------------------------------------------------------- one encode: where everything lies
// Filled by zk_enc_layout from the plan; the stages below read and write nothing of the engine's encode buffers but through it.
namespace {
struct ZkEncLayout {
    ZkEncPlan pl;
    ZkEncCut cut;                           // the call's frames, from the arguments alone (zk_enc_sched.h)
    // pinned (zk_engine::Enc::pin), rounded to 64 bytes each: frames | blocks (+ 1) | doff | the predefined tables | segs
    ZkEncFrame *frames; ZkEncBlock *blocks; uint64_t *doff; ZkEncTables *htab; ZkEncFrame *segs;
    size_t frames_bytes;                    // of the frame list, rounded: the block list follows it on both sides, so one copy uploads both
    // device twins: Enc::lists (frames | blocks), Enc::seg
    ZkEncFrame *d_frames; ZkEncBlock *d_blocks; ZkEncFrame *d_segs;
    // Enc::words: nf + 1 words each, then the predefined tables
    uint64_t *c64, *out_off, *hashes, *d_doff; ZkEncTables *dtab;
    uint64_t *seqs; uint32_t *mpos;         // Enc::seqs: seq_total + 1 packed sequences, the match positions behind them
    uint8_t *lits, *scratch;                // Enc::lits, Enc::scratch
    ZkEncTables *ftab;                      // Enc::ftab
    // what the stages hand on
    const uint8_t *src, *msrc;              // the input; what the matcher reads (prefix mode: the staged [prefix tail | frame] records)
    ZkEncLdm ldm;                           // far history of this call (zk_enc_far_history)
    size_t dense_span;                      // input bytes the dense scratch covers: a slice of whole frames, or all of it
    uint64_t rec_total;                     // bytes of all the matcher's records: the input, in prefix mode with a history before every frame
    uint64_t slice_cap;                     // zk_enc_match's slices of whole frames: at most this many bytes each (never less than a frame); 0: one slice
    uint32_t *cand, *part, *poff;           // Enc::dense: dense_span + ZKE_DENSE_SLACK candidates, as many sorted positions, the pass offsets
    bool cks_beside;                        // the checksums run on the second queue and are joined before the assembly
    // the dictionary route
    uint8_t *stage;                         // the staged records of one slice (Enc::hist)
    const ZkEncDictDev *dd;                 // a formatted dictionary's tables, or null
    ZkEncDictId did; const ZkEncDictId *pdid;   // the Dictionary_ID field (pdid: null on every other route and for a raw-content dictionary)
};
template <class T> int zk_enc_reserve(zk_engine *e, zk_devbuf &b, size_t bytes, T **p)
{
    const int rc = zk_devbuf_reserve(e, b, bytes);
    *p = (T *)b.p;
    return rc;
}
}  // namespace

// Counts come in with pl (zke_plan_count); the lists are filled in between the two halves, since the sequence and scratch totals
// that size the device side come out of the fill.  (A list planned on the device comes with all its totals: nothing is filled here.)
static int zk_enc_layout(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L)
{
    zk_engine::Enc &c = e->enc;
    ZkEncPlan &pl = L.pl;
    const uint32_t nf = pl.nf, nb = pl.nb, nseg = pl.nseg;
    const size_t frames_bytes = ((size_t)nf * sizeof(ZkEncFrame) + 63) & ~(size_t)63;
    const size_t blocks_bytes = ((size_t)(nb + 1) * sizeof(ZkEncBlock) + 63) & ~(size_t)63;
    const size_t doff_bytes = ((size_t)(nf + 1) * 8 + 63) & ~(size_t)63;
    const size_t segs_bytes = ((size_t)(nseg + 1) * sizeof(ZkEncFrame) + 63) & ~(size_t)63;
    const size_t segs_at = (frames_bytes + blocks_bytes + doff_bytes + sizeof(ZkEncTables) + 63) & ~(size_t)63;
    int rc;
    L.frames_bytes = frames_bytes;
    if (a.d_plan_sums) {
        // planned on the device: the records exist there only (zk_enc_plan_upload launches the fill), the host holds the tables
        if ((rc = zk_pin_reserve(e, c.pin, c.pin_cap, sizeof(ZkEncTables) + 64))) return rc;
        L.frames = nullptr; L.blocks = nullptr; L.doff = nullptr; L.segs = nullptr;
        L.htab = (ZkEncTables *)c.pin;
    } else {
        if ((rc = zk_pin_reserve(e, c.pin, c.pin_cap, frames_bytes + blocks_bytes + doff_bytes + sizeof(ZkEncTables) + 64 + segs_bytes))) return rc;
        L.frames = (ZkEncFrame *)c.pin;
        L.blocks = (ZkEncBlock *)(c.pin + frames_bytes);
        L.doff = (uint64_t *)(c.pin + frames_bytes + blocks_bytes);
        L.htab = (ZkEncTables *)(c.pin + frames_bytes + blocks_bytes + doff_bytes);
        L.segs = (ZkEncFrame *)(c.pin + segs_at);
        if (a.list) zke_plan_fill_list(a.list, a.level, a.d_prefix ? a.prefix_len : 0, &pl, L.frames, L.blocks, L.segs, L.doff);
        else zke_plan_fill(a.n, a.frame_size, a.level, a.d_prefix ? a.prefix_len : 0, &pl, L.frames, L.blocks, L.segs, L.doff);
    }
    uint8_t *lists;
    if ((rc = zk_enc_reserve(e, c.lists, frames_bytes + blocks_bytes + 256, &lists))) return rc;
    if ((rc = zk_enc_reserve(e, c.seqs, (size_t)(pl.seq_total + 1) * 12 + 64, &L.seqs))) return rc;       // packed sequences (u64) + match positions (u32)
    if ((rc = zk_enc_reserve(e, c.lits, (size_t)a.n + 64, &L.lits))) return rc;
    if ((rc = zk_enc_reserve(e, c.scratch, (size_t)pl.scratch_total + 64, &L.scratch))) return rc;
    if ((rc = zk_enc_reserve(e, c.words, (size_t)(nf + 1) * 8 * 4 + 64 + sizeof(ZkEncTables), &L.c64))) return rc;
    if ((rc = zk_enc_reserve(e, c.ftab, (size_t)nf * sizeof(ZkEncTables) + 64, &L.ftab))) return rc;
    if ((rc = zk_enc_reserve(e, c.seg, segs_bytes + 64, &L.d_segs))) return rc;
    L.d_frames = (ZkEncFrame *)lists;
    L.d_blocks = (ZkEncBlock *)(lists + frames_bytes);
    L.mpos = (uint32_t *)(L.seqs + pl.seq_total + 1);
    L.out_off = L.c64 + (nf + 1); L.hashes = L.out_off + (nf + 1); L.d_doff = L.hashes + (nf + 1);
    L.dtab = (ZkEncTables *)(L.d_doff + (nf + 1));
    return 0;
}

// ---------------------------------------------------------------- the stages of an encode, in the order zk_encode_enqueue runs them
// frame / block / segment lists (host arithmetic only: zk_enc_plan.h), then lists, frame offsets and predefined tables go up
static int zk_enc_plan_upload(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    // the matcher sees the last `hist` bytes of the prefix right before every frame
    const uint32_t hist = a.d_prefix ? zke_prefix_hist(a.prefix_len) : 0;
    if (a.d_plan_sums) {
        // a list planned on the device: the totals are here (zk_encode_frame_list_dev waited for them with the offsets)
        const ZkEncPlanSum &t = *a.plan_totals;
        if (t.nb > 0xFFFFFFF0u || t.nseg > 0xFFFFFFF0u) return -(int)ZK_E_GENERIC;
        L.pl = ZkEncPlan{a.list_count, t.nb, t.nseg, hist, t.seq, t.scratch};
    }
    else if (!(a.list ? zke_plan_count_list(a.list, a.list_count, hist, &L.pl) : zke_plan_count(a.n, a.frame_size, hist, &L.pl))) return -(int)ZK_E_GENERIC;
    L.cut = ZkEncCut{a.list, L.pl.nf, a.n, a.frame_size};
    int rc;
    if ((rc = zk_enc_layout(e, a, L))) return rc;
    if (!e->enc.tables_ready) { zk_build_enc_tables(&e->enc.tables); e->enc.tables_ready = true; }
    *L.htab = e->enc.tables;
    if (a.d_plan_sums) zk_launch_enc_plan_fill(st, a.d_list, a.list_count, a.level, a.d_prefix ? a.prefix_len : 0, hist, a.d_plan_sums, L.d_frames, L.d_blocks, L.d_segs, L.d_doff);
    else {
        ZK_HIP(hipMemcpyAsync(L.d_frames, L.frames, L.frames_bytes + (size_t)L.pl.nb * sizeof(ZkEncBlock), hipMemcpyHostToDevice, st));   // frames + blocks are contiguous
        ZK_HIP(hipMemcpyAsync(L.d_doff, L.doff, (size_t)(L.pl.nf + 1) * 8, hipMemcpyHostToDevice, st));
    }
    ZK_HIP(hipMemcpyAsync(L.dtab, L.htab, sizeof(ZkEncTables), hipMemcpyHostToDevice, st));
    zk_profile_begin(e);
    L.src = L.msrc = (const uint8_t *)a.d_src;
    L.stage = nullptr; L.slice_cap = 0;
    L.dd = a.cdict && a.cdict->formatted ? a.cdict->d_tab : nullptr;
    L.did = ZkEncDictId{a.cdict ? a.cdict->id : 0u, a.cdict ? a.cdict->id_width : 0u};
    L.pdid = L.dd ? &L.did : nullptr;
    return 0;
}

// prefix mode: [prefix tail | frame] records for the matcher; and the records its workgroups are launched over, the segments
// (one per <= 256 KiB of a frame)
static int zk_enc_stage_hist(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    const uint32_t hist = L.pl.hist;
    const ZkEncStagePlan p = zk_enc_stage_plan(L.cut, hist, a.cdict != nullptr, e->enc.dict_slice_bytes);
    L.rec_total = p.rec_total;
    if (hist) {
        uint8_t *stage;
        int rc;
        if ((rc = zk_enc_reserve(e, e->enc.hist, p.stage_bytes + 64, &stage))) return rc;
        // the dictionary route: slices of whole frames, staged by zk_enc_match right before each slice is matched
        if (a.cdict) { L.stage = stage; L.slice_cap = p.slice_cap; }
        else {
            zk_launch_enc_stage_hist(st, L.src, (const uint8_t *)a.d_prefix + (a.prefix_len - hist), L.d_frames, L.pl.nf, stage);
            L.msrc = stage;
        }
    }
    if (L.segs) ZK_HIP(hipMemcpyAsync(L.d_segs, L.segs, (size_t)L.pl.nseg * sizeof(ZkEncFrame), hipMemcpyHostToDevice, st));
    return 0;
}

// far history (ZkEncLdm), one of: none; a table per frame over its own bytes, with the dense candidates on top at the dense
// levels; a table over a prefix the ring cannot hold (rebuilt per call: the bytes are the caller's) -- zk_enc_far_plan says which
static int zk_enc_far_history(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    const uint64_t plen = a.d_prefix ? a.prefix_len : 0;
    const ZkEncFarPlan p = zk_enc_far_plan(L.cut, a.level, plen, L.pl.hist, L.pl.nseg, e->enc.dense_slice_bytes);
    ZkEncLdm &ldm = L.ldm;
    ldm = p.ldm;
    L.dense_span = p.dense_span;
    int rc;
    uint32_t *table;
    if (p.kind == ZK_ENC_FAR_INFRAME) {
        uint8_t *buf;
        if (a.list) {
            // the records of the frames with a table go up in front of the tables
            if ((rc = zk_pin_reserve(e, e->enc.pin_lf, e->enc.pin_lf_cap, p.lf_bytes))) return rc;
            zk_enc_far_list_frames(L.cut, a.level, plen, (ZkEncLdmFrame *)e->enc.pin_lf);
        }
        if ((rc = zk_enc_reserve(e, e->enc.ldm, p.lf_bytes + p.table_bytes + 64, &buf))) return rc;
        if (a.list) {
            ZK_HIP(hipMemcpyAsync(buf, e->enc.pin_lf, (size_t)ldm.nlf * sizeof(ZkEncLdmFrame), hipMemcpyHostToDevice, st));
            ldm.lf = (const ZkEncLdmFrame *)buf;
        }
        table = (uint32_t *)(buf + p.lf_bytes);
        if (zk_launch_enc_ldm_build_frames(st, L.src, ldm, table, a.list ? ldm.nlf : L.pl.nf, p.table_bytes, p.build_gx)) { e->last_err = "hipMemsetAsync (in-frame long-distance table)"; return ZK_ERR_HIP; }
        ldm.table = table;
        if (p.dense_span) {
            L.slice_cap = p.slice_cap;
            if ((rc = zk_enc_reserve(e, e->enc.dense, (2 * p.cand_words + p.poff_words) * sizeof(uint32_t) + 64, &L.cand))) return rc;
            L.part = L.cand + p.cand_words; L.poff = L.part + p.cand_words;
            ldm.dense = L.cand;
        }
    }
    if (p.kind == ZK_ENC_FAR_PREFIX) {
        ldm.pfx = (const uint8_t *)a.d_prefix;
        if ((rc = zk_enc_reserve(e, e->enc.ldm, p.table_bytes + 64, &table))) return rc;
        if (zk_launch_enc_ldm_build(st, ldm, table, p.table_bytes, p.build_gx)) { e->last_err = "hipMemsetAsync (long-distance table)"; return ZK_ERR_HIP; }
        ldm.table = table;
    }
    return 0;
}

// the match pass, slice after slice of whole frames (zk_enc_slice_end): the dense candidates of a slice, then the matcher over its
// segments.  Without dense history, or when its scratch spans the whole input, everything is one slice.  The candidate arrays are indexed
// like the source, so a slice's kernels get them shifted by the slice's first byte.  Timed: the two kernels of one slice each by itself;
// of several, the whole loop as the match kernel.
static int zk_enc_match(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    const uint32_t nf = L.pl.nf;
    const bool sliced = L.slice_cap != 0;   // (dense scratch or staged records below the call's size; never both: a prefix has no dense history)
    zk_kernel_timer whole(e, ZK_K_ENC_MATCH, st, sliced);
    for (uint32_t f0 = 0, s0 = 0; f0 < nf;) {
        const ZkEncSlice end = zk_enc_slice_end(L.cut, L.pl.hist, L.rec_total, L.slice_cap, L.pl.nseg, f0, s0);
        const uint32_t f1 = end.f1, s1 = end.s1;
        const uint64_t lo = zk_enc_frame_src(L.cut, f0);
        ZkEncLdm sl = L.ldm;
        if (sl.dense) {
            sl.dense = L.cand - lo;
            zk_kernel_timer t(e, ZK_K_ENC_DENSE, st, !sliced);
            zk_launch_enc_dense_cand(st, L.src, L.d_segs + s0, s1 - s0, sl, L.cand - lo, L.part - lo, L.poff);
        }
        zk_kernel_timer t(e, ZK_K_ENC_MATCH, st, !sliced);
        if (L.stage) {
            // the slice's [content tail | frame] records: the frames' m_off count from the call's first record, so the buffer is handed on
            // shifted by the slice's first record (the next slice's staging runs behind this slice's matcher on the same queue)
            L.msrc = L.stage - zk_enc_frame_rec(L.cut, L.pl.hist, f0);
            zk_launch_enc_stage_hist(st, L.src, (const uint8_t *)a.d_prefix + (a.prefix_len - L.pl.hist), L.d_frames + f0, f1 - f0, (uint8_t *)L.msrc);
        }
        zk_launch_enc_match(st, L.msrc, L.d_segs + s0, s1 - s0, L.d_blocks, L.seqs, L.lits, a.level, sl);
        f0 = f1; s0 = s1;
    }
    return 0;
}

// the frames' FSE tables from their sequences
static int zk_enc_table_build(zk_engine *e, const zk_enc_args &, ZkEncLayout &L, hipStream_t st)
{
    zk_kernel_timer t(e, ZK_K_ENC_FSE_BUILD, st);
    zk_launch_enc_fse_build(st, L.src, L.d_frames, L.pl.nf, L.d_blocks, L.seqs, L.mpos, L.dtab, L.ftab, L.dd);
    return 0;
}

// the checksums: on the second queue beside the entropy stage (which waits on its own chains; beside the matcher they cost it
// 2 ms of vector issue slots), joined by zk_enc_assemble; on st when profiling, or when the second queue cannot be had
static int zk_enc_checksums_fork(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    zk_engine::Enc &c = e->enc;
    L.cks_beside = false;
    if (!a.checksum) return 0;
    if (!e->profiling && !c.aux) {
        if (hipStreamCreateWithFlags(&c.aux, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c.ev_join, hipEventDisableTiming) != hipSuccess) { c.aux = nullptr; (void)hipGetLastError(); }
    }
    if (!e->profiling && c.aux) {
        L.cks_beside = true;                // from here on an early return of zk_encode_enqueue waits for the second queue
        ZK_HIP(hipEventRecord(c.ev_fork, st));
        ZK_HIP(hipStreamWaitEvent(c.aux, c.ev_fork, 0));
        zk_launch_xxh64(c.aux, L.src, L.d_doff, 0, L.pl.nf, nullptr, L.hashes, zk_xxh_plan_enc(L.pl.nf, e->choice));
        ZK_HIP(hipEventRecord(c.ev_join, c.aux));
    } else { zk_kernel_timer t(e, ZK_K_ENC_XXH64, st); zk_launch_xxh64(st, L.src, L.d_doff, 0, L.pl.nf, nullptr, L.hashes, zk_xxh_plan_enc(L.pl.nf, e->choice)); }
    return 0;
}

static int zk_enc_entropy(zk_engine *e, const zk_enc_args &, ZkEncLayout &L, hipStream_t st)
{
    zk_kernel_timer t(e, ZK_K_ENC_ENTROPY, st);
    zk_launch_enc_entropy(st, L.src, L.d_frames, L.d_blocks, L.pl.nb, L.seqs, L.mpos, L.lits, L.scratch, L.ftab, L.pl.nf, L.dd);
    return 0;
}

// frame sizes (the caller's seek entries too), their prefix sums, and the total on its way to the pinned word ZK_HW_ENC_TOTAL
static int zk_enc_sizes_total(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    const uint32_t nf = L.pl.nf;
    zk_launch_enc_sizes(st, L.d_frames, nf, L.d_blocks, L.ftab, a.checksum, L.c64, (uint32_t *)a.d_c_sizes, (uint32_t *)a.d_d_sizes, L.pdid);
    zk_launch_scan64(st, L.c64, nf, L.out_off);
    ZK_HIP(hipMemcpyAsync(e->h_words + ZK_HW_ENC_TOTAL, L.out_off + nf, 8, hipMemcpyDeviceToHost, st));
    return 0;
}

// a destination below the bound: the frames may not fit, and the total decides before anything is written
static int zk_enc_fit_check(zk_engine *e, const zk_enc_args &a, ZkEncLayout &, hipStream_t st)
{
    if (a.dst_cap >= zk_enc_bound(a)) return 0;
    ZK_HIP(hipStreamSynchronize(st));
    return e->h_words[ZK_HW_ENC_TOTAL] > a.dst_cap ? -(int)ZK_E_DST_TOO_SMALL : 0;
}

// the checksums join, then the frames are put together at their offsets
static int zk_enc_assemble(zk_engine *e, const zk_enc_args &a, ZkEncLayout &L, hipStream_t st)
{
    if (L.cks_beside) ZK_HIP(hipStreamWaitEvent(st, e->enc.ev_join, 0));
    zk_kernel_timer t(e, ZK_K_ENC_COMPACT, st);
    zk_launch_enc_assemble(st, L.src, L.d_frames, L.pl.nf, L.d_blocks, L.pl.nb, L.ftab, L.lits, L.scratch, L.out_off, L.c64, L.hashes, a.checksum, (uint8_t *)a.d_dst, L.pdid);
    return 0;
}

// Enqueue one encode on `st`.  With dst_cap >= zk_compress_bound(n, frame_size) nothing blocks: the total size arrives in
// the engine's pinned word ZK_HW_ENC_TOTAL once the stream has run (zk_encode_finish); a smaller destination needs the
// total before the frames may be assembled, so the stream is synchronised once in the middle (zk_enc_fit_check).
// The frame / block lists are built in pinned host memory that stays untouched until the next enqueue: one encode in flight.
// A stage that refuses the call (-70 from zk_enc_fit_check, a failed reservation or launch) leaves through the loop's one exit, which waits
// for the second queue if zk_enc_checksums_fork has put the checksums there: zk_enc_assemble, which joins them, has not run then.
int zk_encode_enqueue(zk_engine *e, const zk_enc_args &a, hipStream_t st, uint32_t *nf_out)
{
    if (!e || a.frame_size == 0 || a.frame_size > ZK_SEEKABLE_MAX_FRAME_SIZE || !a.d_dst || (a.n && !a.d_src)) return ZK_ERR_ARGUMENT;
    if ((a.list ? a.list_count : a.n == 0 ? 1 : (a.n + a.frame_size - 1) / a.frame_size) > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (a.list && !a.list_count) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    static int (*const stages[])(zk_engine *, const zk_enc_args &, ZkEncLayout &, hipStream_t) = {
        zk_enc_plan_upload, zk_enc_stage_hist, zk_enc_far_history, zk_enc_match, zk_enc_table_build, zk_enc_checksums_fork,
        zk_enc_entropy, zk_enc_sizes_total, zk_enc_fit_check, zk_enc_assemble};
    ZkEncLayout L;
    L.cks_beside = false;
    for (auto stage : stages) {
        if (const int rc = stage(e, a, L, st)) {
            // the checksum kernel on the second queue reads the caller's source: nothing of this call runs on once it has returned
            if (L.cks_beside) (void)hipStreamSynchronize(e->enc.aux);
            return rc;
        }
        if (a.matched && stage == zk_enc_match) { *a.matched = ZkEncMatched{L.d_blocks, L.pl.nb, L.seqs, L.lits}; break; }
    }
    if (nf_out) *nf_out = L.pl.nf;
    return 0;
}

int zk_encode_finish(zk_engine *e, hipStream_t st, uint64_t *written_out)
{
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    if (written_out) *written_out = e->h_words[ZK_HW_ENC_TOTAL];
    return 0;
}

extern "C" int zk_encode_frames_prefix_dev(zk_engine *e, const void *d_src, uint64_t n, uint32_t frame_size, int level, int checksum,
                                           const void *d_prefix, uint64_t prefix_len, void *d_dst, uint64_t dst_cap, void *d_c_sizes,
                                           void *d_d_sizes, uint32_t *n_frames_out, uint64_t *written_out, void *stream)
{
    if (!e) return ZK_ERR_ARGUMENT;
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    zk_enc_args a{d_src, n, frame_size, level, checksum, d_prefix, prefix_len, d_dst, dst_cap, d_c_sizes, d_d_sizes};
    uint32_t nf = 0;
    int rc = zk_encode_enqueue(e, a, st, &nf);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = zk_encode_finish(e, st, &total))) return rc;
    if (n_frames_out) *n_frames_out = nf;
    if (written_out) *written_out = total;
    return 0;
}

// ---------------------------------------------------------------- the dictionary route (zk_enc_dict.h)
extern "C" int zk_cdict_create(zk_engine *e, const zk_dict *d, zk_cdict **out)
{
    if (!e || !d || !out) return ZK_ERR_ARGUMENT;
    *out = nullptr;
    ZK_HIP(hipSetDevice(e->device));
    zk_cdict *c = new zk_cdict();
    c->e = e; c->formatted = d->L.formatted; c->id = d->L.id; c->id_width = zke_dict_id_width(d->L.id);
    const uint8_t *content = d->bytes.data() + d->L.content_off;
    const uint64_t clen = d->bytes.size() - d->L.content_off;
    // what the matcher can reach of the content: its ring's window and, beyond it, the long-distance table's span
    c->content_len = zke_ldm_usable(clen);
    auto fail = [&](int rc) { zk_cdict_free(c); return rc; };
    if (hipMalloc(&c->d_content, (size_t)c->content_len + ZKE_LDM_SLACK) != hipSuccess) { (void)hipGetLastError(); e->last_err = "hipMalloc (dictionary content)"; return fail(ZK_ERR_HIP); }
    if (hipMemset(c->d_content, 0, (size_t)c->content_len + ZKE_LDM_SLACK) != hipSuccess ||
        (c->content_len && hipMemcpy(c->d_content, content + (clen - c->content_len), c->content_len, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError(); e->last_err = "hipMemcpy (dictionary content)"; return fail(ZK_ERR_HIP);
    }
    if (c->formatted) {
        if (!e->enc.tables_ready) { zk_build_enc_tables(&e->enc.tables); e->enc.tables_ready = true; }
        ZkEncDictDev *h = new ZkEncDictDev;
        const uint32_t r = zke_dict_build(d->bytes.data(), d->L, e->enc.tables, h);
        hipError_t he = r ? hipSuccess : hipMalloc((void **)&c->d_tab, sizeof(ZkEncDictDev));
        if (!r && he == hipSuccess) he = hipMemcpy(c->d_tab, h, sizeof(ZkEncDictDev), hipMemcpyHostToDevice);
        delete h;
        if (r) return fail(-(int)r);
        if (he != hipSuccess) { (void)hipGetLastError(); e->last_err = "hipMalloc / hipMemcpy (dictionary tables)"; return fail(ZK_ERR_HIP); }
    }
    *out = c;
    return 0;
}
extern "C" void zk_cdict_free(zk_cdict *c)
{
    if (!c) return;
    if (c->e) (void)hipSetDevice(c->e->device);
    if (c->d_content) (void)hipFree(c->d_content);
    if (c->d_tab) (void)hipFree(c->d_tab);
    delete c;
}
extern "C" uint32_t zk_cdict_id(const zk_cdict *c) { return c ? c->id : 0; }

extern "C" int zk_encode_frames_dict_dev(zk_engine *e, const void *d_src, uint64_t n, uint32_t frame_size, int level, int checksum, const zk_cdict *cdict,
                                         void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint32_t *n_frames_out, uint64_t *written_out, void *stream)
{
    if (!e || !cdict || cdict->e != e) return ZK_ERR_ARGUMENT;
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    // a dictionary without content (a formatted one may have none) leaves nothing to stage: the frames still name it and may use its tables
    zk_enc_args a{d_src, n, frame_size, level, checksum, cdict->content_len ? cdict->d_content : nullptr, cdict->content_len, d_dst, dst_cap, d_c_sizes, d_d_sizes, cdict};
    uint32_t nf = 0;
    int rc = zk_encode_enqueue(e, a, st, &nf);
    if (rc) return rc;
    uint64_t total = 0;
    if ((rc = zk_encode_finish(e, st, &total))) return rc;
    if (n_frames_out) *n_frames_out = nf;
    if (written_out) *written_out = total;
    return 0;
}

// ---------------------------------------------------------------- frames of caller-given sizes
// The offsets come to the host first (8 bytes per frame, one wait for `st`): the list is checked there, and the slices, the far-history tables
// and -- unless the device makes it -- the plan are host arithmetic on it.  From there on it is the one pipeline above -- zk_enc_args::list --
// on the plain, the prefix or the dictionary route.
static int zk_enc_frame_list_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, int checksum,
                                 const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict,
                                 void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint64_t *written_out, void *stream, ZkEncMatched *matched)
{
    if (!e || (cdict && cdict->e != e) || (cdict && d_prefix && prefix_len)) return ZK_ERR_ARGUMENT;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) { if (written_out) *written_out = 0; return 0; }
    if (!d_off || !d_dst) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    int rc;
    if ((rc = zk_pin_reserve(e, e->enc.pin_off, e->enc.pin_off_cap, ((size_t)count + 1) * 8))) return rc;
    uint64_t *off = (uint64_t *)e->enc.pin_off;
    ZK_HIP(hipMemcpyAsync(off, d_off, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, st));
    if (!d_prefix) prefix_len = 0;
    if (cdict) { d_prefix = cdict->content_len ? cdict->d_content : nullptr; prefix_len = cdict->content_len; }
    // The plan on the device (ZK_CHOICE_ENC_PLAN): the running sums are made from the offsets as the caller left them, before the host has seen
    // them -- arithmetic on their differences, nothing is addressed by them -- so that the totals arrive with the offsets in the one wait.
    const bool dev_plan = e->enc.plan_choice == 2 || (e->enc.plan_choice == 0 && count >= ZK_ENC_PLAN_DEV_FRAMES);
    ZkEncPlanSum *d_sums = nullptr, *totals = (ZkEncPlanSum *)(e->h_words + ZK_HW_ENC_PLAN);
    if (dev_plan) {
        if ((rc = zk_enc_reserve(e, e->enc.plan, ((size_t)count + 1) * sizeof(ZkEncPlanSum) + 64, &d_sums))) return rc;
        zk_launch_enc_plan_scan(st, (const uint64_t *)d_off, count, zke_prefix_hist(prefix_len) != 0, d_sums);
        ZK_HIP(hipMemcpyAsync(totals, d_sums + count, sizeof(ZkEncPlanSum), hipMemcpyDeviceToHost, st));
    }
    ZK_HIP(hipStreamSynchronize(st));
    uint64_t max_frame = 0;
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    const uint64_t n = off[count] - off[0];
    if (n && !d_src) return ZK_ERR_ARGUMENT;
    zk_enc_args a{d_src ? (const uint8_t *)d_src + off[0] : nullptr, n, (uint32_t)(max_frame ? max_frame : 1), level, checksum, prefix_len ? d_prefix : nullptr, prefix_len,
                  d_dst, dst_cap, d_c_sizes, d_d_sizes, cdict, off, count};
    if (dev_plan) { a.d_list = (const uint64_t *)d_off; a.d_plan_sums = d_sums; a.plan_totals = totals; }
    a.matched = matched;
    if ((rc = zk_encode_enqueue(e, a, st, nullptr))) return rc;
    if (matched) return 0;
    uint64_t total = 0;
    if ((rc = zk_encode_finish(e, st, &total))) return rc;
    if (written_out) *written_out = total;
    return 0;
}
extern "C" int zk_encode_frame_list_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, int checksum,
                                        const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict,
                                        void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint64_t *written_out, void *stream)
{
    return zk_enc_frame_list_dev(e, d_src, d_off, count, level, checksum, d_prefix, prefix_len, cdict, d_dst, dst_cap, d_c_sizes, d_d_sizes, written_out, stream, nullptr);
}
int zk_encode_frame_list_matched(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, const void *d_prefix, uint64_t prefix_len,
                                 void *d_dst, uint64_t dst_cap, ZkEncMatched *matched, hipStream_t st)
{
    return zk_enc_frame_list_dev(e, d_src, d_off, count, level, 0, d_prefix, prefix_len, nullptr, d_dst, dst_cap, nullptr, nullptr, nullptr, st, matched);
}

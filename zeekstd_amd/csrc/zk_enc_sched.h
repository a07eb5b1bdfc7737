// zk_enc_sched.h -- what one encode decides from the shape of its call: the far history it gets, how many table entries that takes, how the call
// is cut into slices of whole frames, how big the scratch is, which grid a far-history kernel gets and which match-kernel instance runs.
// Plain C++ over zk_enc_plan.h / zk_enc_device.h, no HIP and no engine types: the stages of zk_engine_enc.hip and the launchers of
// zk_encode.hip carry these decisions out, the CPU harnesses of tests/sim/ allocate and iterate from the same functions, and
// tests/test_enc_sched.py pins every function at its edges.  (The counterpart of zk_dec_plan.h.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "zk_enc_device.h"
#include "zk_enc_plan.h"

// ---------------------------------------------------------------- the cut of a call into frames
// `count` frames: of frame_size bytes over n input bytes (the last one shorter), or the caller's list[count + 1] (frame_size: its largest frame;
// null: the uniform cut).  Host arithmetic from the arguments alone (what zke_plan_frame is handed), so that nothing on the host reads the
// frame records: they may have been made on the device.
struct ZkEncCut { const uint64_t *list; uint32_t count; uint64_t n; uint32_t frame_size; };
// where frame f starts in the source, its bytes, and where its record starts in the matcher's source (hist bytes of history before every frame)
inline uint64_t zk_enc_frame_src(const ZkEncCut &c, uint32_t f) { return c.list ? c.list[f] - c.list[0] : (uint64_t)f * c.frame_size; }
inline uint32_t zk_enc_frame_bytes(const ZkEncCut &c, uint32_t f)
{
    if (c.list) return (uint32_t)(c.list[f + 1] - c.list[f]);
    const uint64_t at = (uint64_t)f * c.frame_size;
    return (uint32_t)(c.n - at < c.frame_size ? c.n - at : c.frame_size);
}
inline uint64_t zk_enc_frame_rec(const ZkEncCut &c, uint32_t hist, uint32_t f)
{
    if (!hist) return zk_enc_frame_src(c, f);
    return c.list ? (uint64_t)f * hist + zk_enc_frame_src(c, f) : (uint64_t)f * ((uint64_t)hist + c.frame_size);
}

// ---------------------------------------------------------------- the grids of the far-history kernels
constexpr uint32_t ZK_ENC_GRID_Y_MAX = 65535;       // a grid's y dimension ends here (4 GiB of 64 KiB frames are 65536 of them): frames in launches of at most that many
// zk_k_enc_ldm_build_frames: gridDim.x from the bytes of the largest frame, gridDim.y = the frames of one launch from frame f0 on
inline uint32_t zk_enc_ldm_frames_gx(uint32_t frame_bytes) { const uint64_t wgs = ((uint64_t)frame_bytes + 4095) / 4096; return (uint32_t)(wgs < 1024 ? wgs : 1024); }
inline uint32_t zk_enc_ldm_frames_gy(uint32_t nframes, uint32_t f0) { return nframes - f0 < ZK_ENC_GRID_Y_MAX ? nframes - f0 : ZK_ENC_GRID_Y_MAX; }
// zk_k_enc_ldm_build: gridDim.x from the prefix bytes the table covers (plen - u0)
inline uint32_t zk_enc_ldm_prefix_gx(uint64_t bytes) { const uint64_t wgs = (bytes + 1023) / 1024; return (uint32_t)(wgs < 4096 ? wgs : 4096); }

// ---------------------------------------------------------------- far history (ZkEncLdm)
// none: the ring is all the matcher has; a table per frame over its own bytes, with the dense candidates on top at the dense levels
// (ZkEncFarPlan::dense_span != 0); a table over a prefix the ring cannot hold
enum ZkEncFarKind { ZK_ENC_FAR_NONE, ZK_ENC_FAR_INFRAME, ZK_ENC_FAR_PREFIX };
struct ZkEncFarPlan {
    ZkEncFarKind kind;
    // inframe, frame_size, n_total, log, dlog, plen, u0, and nlf: of a list the frames with a table of their own (their ZkEncLdmFrame records go
    // up in front of the tables).  Every pointer is null: they are the caller's to set
    ZkEncLdm ldm;
    size_t lf_bytes;            // those records, rounded to 64 bytes
    uint64_t entries;           // of the table(s); a list's include the shared empty ones
    size_t table_bytes;         // what is cleared to 0xFF before the build kernel runs: all the entries
    uint32_t build_gx;          // gridDim.x of the kernel that fills the table(s)
    // dense far history, for a SLICE of whole frames at a time: the dense kernels and the match kernel run slice after slice over the same scratch
    uint64_t slice_cap;         // bytes of a slice at most (never less than a frame); 0: the scratch spans the call, one slice
    size_t dense_span;          // input bytes the scratch covers; 0: no dense history
    size_t cand_words;          // dense_span + ZKE_DENSE_SLACK: the words of `cand`, and of `part` behind it
    size_t poff_words;          // nseg * (ZKE_DENSE_PASSES_MAX + 1), behind `part`
};
// prefix_len: 0 without a prefix; hist = zke_prefix_hist(prefix_len); nseg: the plan's; dense_slice: the engine's override of the dense slice (0 = 4 GiB)
inline ZkEncFarPlan zk_enc_far_plan(const ZkEncCut &c, int level, uint64_t prefix_len, uint32_t hist, uint32_t nseg, uint64_t dense_slice)
{
    ZkEncFarPlan p = {};
    // (a prefix of one to three bytes leaves no history -- hist is a multiple of 4 -- but it is a prefix: the frames' windows were planned without
    //  far history, as the twin does; found by reading, round 6: such a frame would have carried offsets beyond its window)
    const uint64_t frame_max = c.frame_size < c.n ? c.frame_size : c.n;
    if (!hist && zke_ldm_in_frame(level, prefix_len, frame_max)) {
        // in-frame far history (level >= 2, no prefix, frames beyond the ring's reach): one table per frame over its own bytes
        p.kind = ZK_ENC_FAR_INFRAME;
        p.ldm.inframe = 1; p.ldm.frame_size = c.frame_size; p.ldm.n_total = c.n; p.ldm.log = zke_ldm_log(frame_max);
        if (c.list) {
            // a table only for the frames that qualify, one behind the other after the shared empty one
            p.entries = zke_ldm_list_shared();
            for (uint32_t f = 0; f < c.count; f++) if (zke_ldm_in_frame(level, prefix_len, zk_enc_frame_bytes(c, f))) {
                p.ldm.nlf++;
                p.entries += 1ull << zke_ldm_log(zk_enc_frame_bytes(c, f));
            }
            p.lf_bytes = ((size_t)p.ldm.nlf * sizeof(ZkEncLdmFrame) + 63) & ~(size_t)63;
            p.build_gx = zk_enc_ldm_frames_gx((uint32_t)frame_max);
        } else {
            p.entries = (uint64_t)c.count << p.ldm.log;
            p.build_gx = zk_enc_ldm_frames_gx(c.frame_size);
        }
        p.table_bytes = (size_t)p.entries * sizeof(uint32_t);
        if (zke_dense_in_frame(level, prefix_len, frame_max)) {
            // dense far history (level 0 / >= 3): 4 bytes per input byte (with the sorted positions 8 x the input: HBM is what this device has),
            // for at most dense_slice bytes of input at a time, so a call of any size takes at most 8 x 4 GiB of it
            p.ldm.dlog = zke_dense_log(level);
            if (!dense_slice) dense_slice = 4ull << 30;
            p.slice_cap = dense_slice > c.frame_size ? dense_slice : c.frame_size;
            p.dense_span = (size_t)(c.n < p.slice_cap ? c.n : p.slice_cap);
            if (p.slice_cap >= c.n) p.slice_cap = 0;
            p.cand_words = p.dense_span + ZKE_DENSE_SLACK;
            p.poff_words = (size_t)nseg * (ZKE_DENSE_PASSES_MAX + 1);
        }
    }
    if (hist && prefix_len > ZKE_WINDOW) {
        const uint64_t usable = zke_ldm_usable(prefix_len);
        p.kind = ZK_ENC_FAR_PREFIX;
        p.ldm.plen = prefix_len; p.ldm.u0 = prefix_len - usable; p.ldm.log = zke_ldm_log(usable);
        p.entries = 1ull << p.ldm.log;
        p.table_bytes = (size_t)p.entries * sizeof(uint32_t);
        p.build_gx = zk_enc_ldm_prefix_gx(usable);
    }
    return p;
}
// the records of a list's frames that qualify, lf[ZkEncFarPlan::ldm.nlf] by ascending start: each frame's table starts where the one before it ends
inline void zk_enc_far_list_frames(const ZkEncCut &c, int level, uint64_t prefix_len, ZkEncLdmFrame *lf)
{
    uint64_t tbase = zke_ldm_list_shared();
    for (uint32_t f = 0, k = 0; f < c.count; f++) if (zke_ldm_in_frame(level, prefix_len, zk_enc_frame_bytes(c, f))) {
        lf[k++] = ZkEncLdmFrame{zk_enc_frame_src(c, f), tbase, zk_enc_frame_bytes(c, f), 0};
        tbase += 1ull << zke_ldm_log(zk_enc_frame_bytes(c, f));
    }
}

// ---------------------------------------------------------------- the staged [history | frame] records of prefix and dictionary mode
// rec_total: bytes of all the matcher's records, the input with `hist` bytes of history before every frame; slice_cap: the dictionary route
// stages slices of whole frames, at most this many record bytes each (never less than a frame's; 0: one slice; dict_slice: the engine's
// override, 0 = 1 GiB); stage_bytes: of the stage buffer, all the records or a slice of them (0 without history)
struct ZkEncStagePlan { uint64_t rec_total, slice_cap; size_t stage_bytes; };
inline ZkEncStagePlan zk_enc_stage_plan(const ZkEncCut &c, uint32_t hist, bool dict, uint64_t dict_slice)
{
    ZkEncStagePlan p = {c.n, 0, 0};
    if (!hist) return p;
    // all the records: as many as frames, one behind the other (a list's are as long as its frames)
    p.rec_total = c.list ? (uint64_t)c.count * hist + c.n : (uint64_t)c.count * ((uint64_t)hist + c.frame_size);
    if (dict) {
        // a bounded buffer for slices of whole frames
        const uint64_t rec = (uint64_t)hist + c.frame_size, cap = dict_slice ? dict_slice : 1ull << 30;
        p.slice_cap = cap > rec ? cap : rec;
    }
    p.stage_bytes = (size_t)(p.slice_cap && p.slice_cap < p.rec_total ? p.slice_cap : p.rec_total);
    if (p.slice_cap >= p.rec_total) p.slice_cap = 0;
    return p;
}

// ---------------------------------------------------------------- the slices of the match pass
// The slice that starts at frame f0 / segment s0 ends in front of frame f1 / segment s1: whole frames while their records fit in slice_cap
// bytes of the matcher's source (without a prefix the frames' bytes in the input), never less than one; a frame has a segment per ZKE_SEGMENT
// bytes.  slice_cap 0: everything that is left (nseg: the plan's).
struct ZkEncSlice { uint32_t f1, s1; };
inline ZkEncSlice zk_enc_slice_end(const ZkEncCut &c, uint32_t hist, uint64_t rec_total, uint64_t slice_cap, uint32_t nseg, uint32_t f0, uint32_t s0)
{
    if (!slice_cap) return ZkEncSlice{c.count, nseg};
    uint32_t f1 = f0, s1 = s0;
    for (; f1 < c.count; f1++) {
        const uint64_t rec_end = f1 + 1 < c.count ? zk_enc_frame_rec(c, hist, f1 + 1) : rec_total;
        if (f1 != f0 && rec_end - zk_enc_frame_rec(c, hist, f0) > slice_cap) break;
        s1 += (zk_enc_frame_bytes(c, f1) + ZKE_SEGMENT - 1) / ZKE_SEGMENT;
    }
    return ZkEncSlice{f1, s1};
}

// ---------------------------------------------------------------- which instance of the match kernel runs
// One instance per setting of zk_enc_device.h (zke_hash_log / zke_lazy / zke_step), without far history, with a sampled table, with dense
// candidates on top.  X(enumerator, the kernel, whether it takes the ZkEncLdm): the launcher (zk_encode.hip) expands this into launches, the
// harnesses of tests/sim/ into calls, with ZK_ENC_MATCH_LDM_<0|1>(ldm) as the last argument.
#define ZK_ENC_MATCH_KERNELS(X) \
    X(ZK_ENC_MATCH_FAST2,         (zk_k_enc_match2<14>),                       0)   /* zke_fast2(): the plan set minmatch 5 */ \
    X(ZK_ENC_MATCH_LAZY,          (zk_k_enc_match<15, 1, 4096, false>),        1) \
    X(ZK_ENC_MATCH_LAZY_1K,       (zk_k_enc_match<15, 1, 1024, false>),        1) \
    X(ZK_ENC_MATCH_FAST_TABLE,    (zk_k_enc_match<14, 0, 4096, true>),         1) \
    X(ZK_ENC_MATCH_LAZY_TABLE,    (zk_k_enc_match<15, 1, 4096, true>),         1) \
    X(ZK_ENC_MATCH_LAZY_1K_TABLE, (zk_k_enc_match<15, 1, 1024, true>),         1) \
    X(ZK_ENC_MATCH_LAZY_DENSE,    (zk_k_enc_match<15, 1, 4096, true, true>),   1) \
    X(ZK_ENC_MATCH_LAZY_1K_DENSE, (zk_k_enc_match<15, 1, 1024, true, true>),   1)
#define ZK_ENC_MATCH_LDM_0(ldm)
#define ZK_ENC_MATCH_LDM_1(ldm) , ldm
enum ZkEncMatchKernel {
#define ZK_ENC_MATCH_ENUM(name, kernel, takes_ldm) name,
    ZK_ENC_MATCH_KERNELS(ZK_ENC_MATCH_ENUM)
#undef ZK_ENC_MATCH_ENUM
};
// has_table / has_dense: ZkEncLdm::table / ::dense of the call
inline ZkEncMatchKernel zk_enc_match_kernel(int level, bool has_table, bool has_dense)
{
    const bool fast = zke_fast(level), step_1k = zke_step(level) == 1024;
    if (has_dense) return step_1k ? ZK_ENC_MATCH_LAZY_1K_DENSE : ZK_ENC_MATCH_LAZY_DENSE;      // (level 0 / >= 3 in frame: never the fast setting)
    if (has_table) return fast ? ZK_ENC_MATCH_FAST_TABLE : step_1k ? ZK_ENC_MATCH_LAZY_1K_TABLE : ZK_ENC_MATCH_LAZY_TABLE;
    return fast ? ZK_ENC_MATCH_FAST2 : step_1k ? ZK_ENC_MATCH_LAZY_1K : ZK_ENC_MATCH_LAZY;
}

// zk_dec_plan.h -- what a decode decides from the shape of its batch, as pure functions: do the checksums run beside the executor,
// does the executor run in segments, and of what size.  Plain C++ (no HIP, no engine): zk_engine.hip, zk_engine_host.hip and
// tests/test_dec_plan.py (which compiles this file with g++) run the same code.
#pragma once
#include <stdint.h>
#include "zk_device.h"      // ZK_SEG_BYTES

// The words zk_k_scan (zk_decode.hip) leaves for the host, read back once per batch into DecCtx::h_words.  ([3] and [6] are
// zk_k_status's: the first error and the frames zk_k_xxh64_follow verified.)
enum { ZK_SCAN_BLOCKS = 0, ZK_SCAN_SEQS = 1, ZK_SCAN_LITS = 2, ZK_SCAN_OWN_TABLES = 4 /* blocks that need per-block sequence tables */,
       ZK_SCAN_OUT_BYTES = 5, ZK_SCAN_MAX_FRAME = 7 /* the longest frame's output */, ZK_SCAN_CHECKSUMMED = 8 /* frames with a Content_Checksum */,
       ZK_SCAN_WORDS = 9 };

// the checksums of a verified batch beside its executor (zk_k_xxh64_follow) or behind it: zk_follow_wanted;
// ZK_CHOICE_XXH64 = 4 asks for "beside" whatever the batch looks like, 1..3 for one of the passes behind the executor
constexpr uint64_t ZK_FOLLOW_MIN_FRAME_BYTES = 512u << 10;

// What the decisions depend on.  nblocks: the batch's block count (the device path: zk_k_scan's; the small path: the host's own
// walk over short frames, 0 when it was not asked for or a frame failed it).
struct ZkDecShape {
    int xxh, exec_seg, seg_kib;             // of ZkKernelChoice
    bool profiling;
    uint32_t count; uint64_t out_bytes, max_frame, nblocks;
    bool has_prefix, alone, follow;         // alone: nothing else of the engine is in flight; follow: zk_follow_wanted said yes
};

// Where the checksums of a verified batch run: beside the executor (zk_k_xxh64_follow) or behind it.  Measured on 16 / 128 / 512 /
// 2048 frames of 2 MiB (profiles/r04_follow_by_batch_size.txt; ms one batch at a time | two in flight; behind = the better of
// the two passes behind the executor):   16: 4.27 -> 3.50 | 2.19 -> 1.91     128: 5.20 -> 5.77 | 3.03 -> 3.07
//                                       512: 6.48 -> 6.76 | 5.32 -> 5.13    2048: 16.7 -> 15.7 | 14.56 -> 14.49 (at four executor
// workgroups per CU; five, the in-flight default, and a checksum wave do not fit a SIMD).  A few frames leave most CUs to the checksum
// waves; a batch that fills the device alone trades 2.7 ms of an idle device for 1.7 ms of the executor; in between a frame IS a
// workgroup and the slowest one -- the one that shares its SIMD -- ends the kernel.  Frames of less than 512 KiB are short chains.
inline bool zk_follow_wanted(const ZkDecShape &s)
{
    if (s.profiling) return false;                          // (per-kernel timing serialises the kernels)
    if (s.xxh) return s.xxh == 4;
    if (s.out_bytes < (uint64_t)s.count * ZK_FOLLOW_MIN_FRAME_BYTES) return false;
    if (s.count <= 64) return true;
    return s.alone ? s.count >= 1024 : s.count < 1024;
}

// Several workgroups per frame (zk_k_exec_seg + zk_k_exec_fill) instead of one (zk_k_exec)?  on: yes, in segments of seg_bytes, at
// most max_segs of them per frame (a frame of n segments' worth of output is cut into at most 2 n + 1).
struct ZkSegPlan { bool on; uint32_t seg_bytes, max_segs; };
// Never with a prefix (history below the frame's first byte is the serial kernel's), never when a frame could have more segments
// than a grid has rows; ZK_CHOICE_EXEC_SEG = 1 / 2 says never / wherever that allows, otherwise the path's verdict by batch shape.
inline ZkSegPlan zk_seg_plan(const ZkDecShape &s, uint32_t default_bytes, bool by_shape)
{
    ZkSegPlan p{false, s.seg_kib ? (uint32_t)s.seg_kib << 10 : default_bytes, 0};
    const uint64_t max_segs = 2 * ((s.max_frame + p.seg_bytes - 1) / p.seg_bytes) + 1;
    if (s.has_prefix || s.exec_seg == 1 || max_segs > 65535) return p;
    p.max_segs = (uint32_t)max_segs;
    p.on = s.exec_seg == 2 || by_shape;
    return p;
}

// The two verdicts by batch shape.  They DISAGREE, and are kept as they were measured: the small path takes segments beside the
// checksum follower at 16 frames or fewer, the device path does not (nor does it know the small path's short frames); the small path
// has no upper bound of 32 frames but its own of 64 (zk_host_decode).
//
// The device path (zk_decode_enqueue): a handful of long frames, where a frame as ONE workgroup leaves the device idle (2 MiB frames,
// HBM-resident, unverified, ms: 1 / 5 / 16 / 32 frames 2.58 / 2.60 / 2.62 / 2.65 -> 1.79 / 1.83 / 1.85 / 2.39; 64 frames 2.80 -> 2.88:
// profiles/r06_seg_probe.txt).  Not where the checksums run beside the executor: a frame's four XXH64 chains (1.7-2.3 ms per 2 MiB,
// whoever runs them) then end the decode, not the executor (verified, 16 frames: 3.52 ms either way).
// (r6, with a wave per frame behind the progress words -- zk_k_xxh64_follow1 -- verified, ms, frame executor | segments: 1 frame 2.94 | 3.01,
//  5: 3.05 | 3.14, 16: 3.08 | 3.31, 32: 3.69 | 3.33)
inline ZkSegPlan zk_seg_plan_dev(const ZkDecShape &s)
{
    if (!s.count || !s.nblocks) return ZkSegPlan{false, 0, 0};
    return zk_seg_plan(s, ZK_SEG_BYTES, (!s.follow || s.count > 16) && s.count <= 32 && s.out_bytes >= (uint64_t)s.count * (4u * ZK_SEG_BYTES));
}
// The small path (zk_decode_small), where the host knows the frames' sizes.  Long frames (a read of one or two 2 MiB frames -- zeekstd's
// default frame size): zk_k_seg_prep / zk_k_exec_seg / zk_k_exec_fill_lds, 1.37 -> 0.6 ms for a 2 MiB frame.  ... and SHORT frames in a
// handful (a seek into 64 KiB frames: sixteen blocks of 4 KiB as this encoder writes them, executed one after the other at ~7 us each by
// a frame's workgroup): a segment per block -- 4 KiB unless ZK_CHOICE_SEG_KIB says otherwise --, all at once, and one turn of the fill
// pass for the frame ...
inline bool zk_small_long_frames(const ZkDecShape &s) { return s.out_bytes >= (uint64_t)s.count * (4u * ZK_SEG_BYTES); }
inline bool zk_small_short_shape(const ZkDecShape &s)
{
    const ZkSegPlan p = zk_seg_plan(s, 4096u, false);       // (max_segs 0: no segments whatever the shape)
    return p.max_segs && !zk_small_long_frames(s) && s.max_frame >= 32768 && s.max_frame <= ZK_SEG_BYTES && (uint64_t)s.count * p.max_segs <= 256;
}
// ... if they HAVE blocks to deal out: the reference's own 64 KiB frames are one block (+ an empty last one), executed by one
// workgroup either way -- the extra launches would only cost them ~25 us.  Does the verdict need the host to count the blocks?
inline bool zk_small_wants_blocks(const ZkDecShape &s) { return zk_small_short_shape(s) && s.exec_seg != 2; }
inline ZkSegPlan zk_seg_plan_small(const ZkDecShape &s)
{
    const bool long_frames = zk_small_long_frames(s);
    const bool short_frames = zk_small_short_shape(s) && (s.exec_seg == 2 || s.nblocks >= 6ull * s.count);
    return zk_seg_plan(s, long_frames ? ZK_SEG_BYTES : 4096u, long_frames || short_frames);
}

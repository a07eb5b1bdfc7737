// zk_dec_plan.h -- what a decode decides from the shape of its batch, as pure functions: do the checksums run beside the executor,
// does the executor run in segments, and of what size; and which kernel, in which template instance and with what grid unit, each stage
// launches (zk_entropy_plan, zk_exec_plan, zk_exec_seg_plan, zk_xxh_plan / zk_xxh_plan_enc, zk_xxh_follow_plan).  The launchers of
// zk_decode.hip take these plans and only launch.  Plain C++ (no HIP, no engine): zk_engine.hip, zk_engine_host.hip, zk_engine_enc.hip
// and tests/test_dec_plan.py (which compiles this file with g++ and pins every threshold and override) run the same code.
#pragma once
#include <stdint.h>
#include "zk_device.h"      // ZK_SEG_BYTES

// Which kernel variant a plan picks.  0 everywhere = by batch shape (what production runs); the other values pin one
// variant whatever the batch looks like, so that tests/ can put every kernel of the large-batch path under a small, exhaustively
// checked input (zk_engine_set_kernel_choice, include/zeekstd_amd.h) and tools/ can time one against the other.
struct ZkKernelChoice {
    int fse_own = 0;        // blocks with tables of their own: 1 zk_k_fse (a lane per block), 2 zk_k_fse_quad in the 56-block layout
    int fse_shared = 0;     // blocks that share tables: 1 zk_k_fse_predef, 2 zk_k_fse_predef_fed, 3 zk_k_fse_sets
    int exec_lanes = 0;     // zk_k_exec tile: 128 / 256 / 512 / 1024 lanes
    int exec_ring = 0;      // 256-lane tiles: 1 a ring of 2 T records, 2 of 4 T
    int xxh = 0;            // 1 zk_k_xxh64 (a wave per frame), 2 zk_k_xxh64_wide (sixteen frames per wave), 3 zk_k_xxh64_lean (the same in 64 registers),
                            // 4 zk_k_xxh64_follow beside the executor (zk_engine.hip)
    int exec_resident = 0;  // zk_k_exec<256>: workgroups per CU (4 / 5) through LDS the launch asks for and does not use
    int small_path = 0;     // host-pointer decode of <= 64 frames: 1 the general pipeline instead, 2 the small path's entropy roles as two kernels
    int exec_seg = 0;       // the executor in segments (zk_k_seg_prep / zk_k_exec_seg / zk_k_exec_fill): 1 never, 2 always (without a prefix); 0 by batch shape
    int seg_kib = 0;        // ... output KiB per segment (1..128; 0 = 128, or 4 for short frames on the small path: zk_seg_plan_small)
    int seg_fill = 0;       // ... the fill pass: 1 zk_k_exec_fill<1024> (rounds through memory), 2 zk_k_exec_fill<256>, 3 zk_k_exec_fill_lds (the segment's holes in LDS); 0 by batch size
    int entropy = 0;        // literals and sequences of a batch: 1 zk_k_huf || the sequence kernels on two queues, 2 zk_k_entropy_frame wherever a batch qualifies
                            // (ZkEntropyPlan::fused); 0 by batch shape
};
// blocks per workgroup of the kernels whose grids the plans and the launchers count in (zk_decode.hip)
constexpr int ZK_HUF_BLOCKS = 16;                        // zk_k_huf
constexpr int ZK_FSEP_LANES = 64;                        // the shared-table sequence kernels and zk_k_entropy_frame (one wave of walkers)

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
    ZkKernelChoice k;
    bool profiling;
    uint32_t count; uint64_t out_bytes, max_frame, nblocks;
    bool has_prefix, alone, follow;         // alone: nothing else of the engine is in flight; follow: zk_follow_wanted said yes
};

// Where the checksums of a verified batch run: beside the executor (zk_k_xxh64_follow) or behind it.  Measured on 16 / 128 / 512 /
// 2048 frames of 2 MiB (profiles/r04_follow_by_batch_size.txt; ms one batch at a time | two in flight; behind = the better of
// the two passes behind the executor):   16: 4.27 -> 3.50 | 2.19 -> 1.91     128: 5.20 -> 5.77 | 3.03 -> 3.07
//                                       512: 6.48 -> 6.76 | 5.32 -> 5.13    2048: 16.7 -> 15.7 | 14.56 -> 14.49 (at four executor
// workgroups per CU; five, the in-flight default when this was measured, and a checksum wave do not fit a SIMD).  A few frames leave most CUs to the checksum
// waves; a batch that fills the device alone trades 2.7 ms of an idle device for 1.7 ms of the executor; in between a frame IS a
// workgroup and the slowest one -- the one that shares its SIMD -- ends the kernel.  Frames of less than 512 KiB are short chains.
inline bool zk_follow_wanted(const ZkDecShape &s)
{
    if (s.profiling) return false;                          // (per-kernel timing serialises the kernels)
    if (s.k.xxh) return s.k.xxh == 4;
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
    ZkSegPlan p{false, s.k.seg_kib ? (uint32_t)s.k.seg_kib << 10 : default_bytes, 0};
    const uint64_t max_segs = 2 * ((s.max_frame + p.seg_bytes - 1) / p.seg_bytes) + 1;
    if (s.has_prefix || s.k.exec_seg == 1 || max_segs > 65535) return p;
    p.max_segs = (uint32_t)max_segs;
    p.on = s.k.exec_seg == 2 || by_shape;
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
inline bool zk_small_wants_blocks(const ZkDecShape &s) { return zk_small_short_shape(s) && s.k.exec_seg != 2; }
inline ZkSegPlan zk_seg_plan_small(const ZkDecShape &s)
{
    const bool long_frames = zk_small_long_frames(s);
    const bool short_frames = zk_small_short_shape(s) && (s.k.exec_seg == 2 || s.nblocks >= 6ull * s.count);
    return zk_seg_plan(s, long_frames ? ZK_SEG_BYTES : 4096u, long_frames || short_frames);
}

// ---------------------------------------------------------------------------------------------- which kernels a stage launches
// One plain struct per stage, filled by one function: the kernel, its template instance (the integers the template takes), the blocks
// or frames a workgroup takes, the LDS a launch asks for beyond the kernel's own.  The launchers (zk_decode.hip) switch over these and
// compute a grid; every threshold and every ZkKernelChoice override is here.

// ---- literals and sequences (zk_launch_huf || zk_launch_fse, or zk_launch_entropy)
constexpr bool ZK_ENTROPY_FUSED_DEFAULT = true;
// the pass behind the shared-table kernel or zk_k_entropy_frame, for the blocks they have not marked done
enum ZkFseRest { ZK_FSE_REST_NONE = 0, ZK_FSE_REST_LANE_56x8 /* zk_k_fse<ZkCells16, 56, 8> */, ZK_FSE_REST_QUAD_16x1 /* zk_k_fse_quad<ZkCellsX16, 16, 1> */,
                 ZK_FSE_REST_QUAD_56x4 /* zk_k_fse_quad<ZkCellsX16, 56, 4> */ };
// quads: every block takes a quad of lanes, 8 blocks per workgroup (zk_k_fse_quad<ZkCells64, 8, 1>) or 16 (<ZkCellsX16, 16, 1>), and nothing
// follows; otherwise shared: 1 zk_k_fse_predef<ZkRevU>, 2 zk_k_fse_predef_fed, 3 zk_k_fse_sets (ZK_FSEP_LANES blocks per workgroup), then rest.
// fused: zk_k_entropy_frame takes the place of zk_k_huf AND of the kernel that quads / shared name (which then say what it replaced); rest
// follows it.  A batch without blocks launches nothing: all zero.
struct ZkEntropyPlan { bool fused; int quads, shared; ZkFseRest rest; };
// n_own_tables counts the DEFINING blocks; frames = 0: unknown.  rest_always: the rest pass runs although no block of the batch defines a
// table -- blocks that repeat a loaded dictionary's tables define none, yet a workgroup of the shared-table kernel may leave them to that pass
// (a block that mixes the dictionary's tables with predefined ones matches no neighbour).  no_fusion: per-kernel timing, a caller that
// keeps the batch on one queue (the host pipeline's chunks), or one that wants no literals.
inline ZkEntropyPlan zk_entropy_plan(uint32_t nblocks, uint32_t n_own_tables, uint32_t frames, const ZkKernelChoice &k, bool rest_always, bool no_fusion)
{
    ZkEntropyPlan p{false, 0, 0, ZK_FSE_REST_NONE};
    if (!nblocks) return p;
    // reader choice (zk_device.h): with >= 6 workgroups per CU the memory pipeline is the limit (aligned words, each
    // loaded once); below that a lane's instruction count is (one unaligned load per sequence).  Measured crossover
    // on 32 KiB blocks between 1024 and 2048 frames of 2 MiB.
    const uint32_t wgs = (nblocks + ZK_FSEP_LANES - 1) / ZK_FSEP_LANES;
    if (k.fse_own == 0 && k.fse_shared == 0 && nblocks <= 16u * 256u) {
        // a small batch (a seek, a handful of frames) is all chain latency: every block, predefined tables or not, takes a
        // quad of lanes (each block builds its own copy of the tables: microseconds)
        // ... and while 8-block workgroups (8-byte cells: ~63 instead of ~80 instructions per sequence of a chain, 10 KiB of tables per
        // block, one workgroup per CU) hold every block in one round, those (what the small path's kernel runs: zk_k_small_entropy)
        p.quads = nblocks <= 8u * 256u ? 8 : 16;
    } else {
        // blocks that share their tables with their neighbours (predefined, or one set per frame): one lane each
        // frames of fewer than 64 blocks: a workgroup's 64 blocks span several frames = several table sets
        p.shared = k.fse_shared ? k.fse_shared : (frames && (uint64_t)nblocks < 64ull * frames) ? 3 : wgs >= 6 * 256 ? 2 : 1;
    }
    // Literals and sequences in ONE kernel (zk_k_entropy_frame) where the sequences would get zk_k_fse_predef_fed and the batch's frames
    // each define at most one set of tables (this engine's encoder); k.entropy == 2 asks for it whatever the batch's size -- also where
    // every block would have taken a quad of lanes.
    if (no_fusion || k.entropy == 1 || k.fse_own || n_own_tables > frames) p.fused = false;
    else if (k.entropy == 2) p.fused = k.fse_shared == 0 || k.fse_shared == 2;
    else p.fused = ZK_ENTROPY_FUSED_DEFAULT && p.shared == 2;
    if (p.quads && !p.fused) return p;
    // blocks with their own tables (every block is visited, the others return at once): a quad of lanes per block.
    // While everything fits in one round, small workgroups (16 blocks, one walking wave + the toucher: 45 KiB of LDS,
    // three per CU) spread the blocks over the CUs and a block's chain latency is all that counts (measured, 2048
    // blocks of ~10 k sequences: 4.13 ms; 56-block workgroups 4.41; one lane per block 4.57).  Beyond that, 56 blocks
    // per CU on four waves (32768 blocks: 20.6 ms with one lane per block, 13.2 with quads).
    // k.fse_own: 1 = the lane-per-block kernel, 2 = quads in the large layout.
    if (!n_own_tables && !rest_always) return p;    // no block defines a table: everything was shared (predefined)
    // (every block the shared-table kernel has not marked done is taken, predefined tables or not.  An archive of this engine's
    // encoder has one defining block per frame, its blocks were all shared, and the pass that finds nothing left must not wait for
    // a whole CU's LDS -- the small layout fits beside whatever else is resident)
    p.rest = k.fse_own == 1 ? ZK_FSE_REST_LANE_56x8 : k.fse_own != 2 && n_own_tables <= 48u * 256u ? ZK_FSE_REST_QUAD_16x1 : ZK_FSE_REST_QUAD_56x4;
    return p;
}

// ---- the executor, one workgroup per frame (zk_launch_exec): zk_k_exec<lanes, prefix, ring>
struct ZkExecPlan { int lanes, ring; uint32_t lds_pad; };     // lanes 128 / 256 / 512 / 1024; a ring of ring x lanes records; lds_pad: LDS asked for and not used
// follow: the checksums run beside this executor (zk_k_xxh64_follow) and want registers left on every SIMD.  (The small path passes
// nseq = 0 -- it does not read the totals back -- and follow = false although its checksums may run beside: kept as it was measured.)
// beside: a batch of the engine was in flight on the other context when this one was enqueued (zk_dec_args::neighbour) and this batch took
// zk_k_entropy_frame -- batches follow each other alike, so that kernel of the next batch is what shares the CUs with this executor.
inline ZkExecPlan zk_exec_plan(uint32_t count, uint64_t nseq, uint64_t out_bytes, bool has_prefix, bool follow, const ZkKernelChoice &k, bool beside = false)
{
    // ... what a frame's matches reach: dense sequence streams (fewer than 10 output bytes per sequence: libzstd from level 3 up, whose
    // window is the whole 2 MiB frame -- every far match a line from beyond the L2) run better with FEWER frames resident: 512-lane tiles
    // hold 512 frames' histories live instead of 1 280 (4 GiB of the reference's level-3 frames: executor 17.0 -> 15.6 ms, the step with
    // two batches in flight 30.6 -> 29.5 ms; level 1, whose matches stay near: 8.4 -> 9.3 ms -- hence only there; tools/gpu_calls/r6a.sh, r6n.sh)
    const bool dense = nseq * 10 > out_bytes;
    // one workgroup per frame: the tile width trades bytes in flight per frame against workgroups per CU
    // (measured on 2 MiB frames: 2048 frames -> 256 lanes.  128 lanes run the kernel alone in 8.9 instead of 9.5 ms -- eight
    // 2-wave workgroups per CU hold all 2048 frames in one round -- but leave no room for the neighbouring batch: with two
    // batches in flight the step is 18.8 ms against 17.2.  1024 frames: 256 lanes 4.95 ms, 128 lanes 6.9; 512 -> 512, 128 -> 1024)
    const int lanes = k.exec_lanes ? k.exec_lanes : count >= 1024 ? (dense ? 512 : 256) : count >= 256 ? 512 : 1024;
    ZkExecPlan p{1024, 2, 0};
    if (has_prefix) p.lanes = lanes <= 256 ? 256 : lanes == 512 ? 512 : 1024;       // (no 128-lane instance with a prefix, and no 4 T ring)
    else {
        if (lanes == 128 || lanes == 256 || lanes == 512) p.lanes = lanes;
        // fewer than 10 output bytes per sequence (libzstd from level 3 up: ~8): a ring of 2 T records ends most 4 KiB tiles
        // early; 4 T keep them whole (executor -8.5 % there, +2 % on sparser streams, hence the switch)
        if (lanes == 256 && (k.exec_ring ? k.exec_ring == 2 : (count >= 1024 && dense))) p.ring = 4;
    }
    // 93 registers and 31 032 bytes of LDS: five 256-lane workgroups per CU.  Four of them leave 128 registers on every SIMD (room for
    // checksum waves, zk_k_xxh64_follow); a launch that asks for 2.5 KiB more LDS than the kernel uses gets four
    // (tests/test_entropy_budget.py pins the size both counts rest on).
    // Four, too, beside another batch of long frames that takes zk_k_entropy_frame: the fifth executor workgroup of a CU costs the
    // neighbour's entropy kernel more than it gives this one.  2 048 frames of 2 MiB, two batches in flight: the step 12.64-12.67 -> 12.25-12.34 ms;
    // three per CU, and four beside the other entropy kernels, are slower (profiles/r09_entropy_resident.txt).  Measured on that shape only.
    const bool long_frames = out_bytes >= (uint64_t)count * ZK_FOLLOW_MIN_FRAME_BYTES;
    const int resident = k.exec_resident ? k.exec_resident : follow || (beside && long_frames) ? 4 : 0;
    if (p.lanes == 256 && resident == 4) p.lds_pad = 2560u;
    return p;
}

// ---- the executor in segments (zk_launch_exec_seg): zk_k_seg_prep, zk_k_exec_seg<lanes, ring>, a fill pass, and the redo pass for
// frames a segment gave up on, always zk_k_exec<256, false, 2, true>
struct ZkExecSegPlan { int lanes, ring, fill_lanes; bool fill_lds; };        // zk_k_exec_fill<fill_lanes>, or zk_k_exec_fill_lds<fill_lanes>
// max_segs: ZkSegPlan's.  (The small path passes nseq = 0 here too.)
inline ZkExecSegPlan zk_exec_seg_plan(uint32_t count, uint32_t max_segs, uint64_t nseq, uint64_t out_bytes, const ZkKernelChoice &k)
{
    const bool dense = nseq * 10 > out_bytes;
    // a segment is a workgroup: wide tiles while the segments alone do not fill the device (a lone frame of 2 MiB: 16 segments), the
    // executor's 256 lanes beyond that.  (exec_lanes = 128 / 512 have no instance here and are ignored.)
    const uint64_t wgs = (uint64_t)count * max_segs;
    ZkExecSegPlan p{256, 2, 1024, true};
    p.lanes = k.exec_lanes == 256 || k.exec_lanes == 1024 ? k.exec_lanes : wgs >= 1024 ? 256 : 1024;
    // (this ring follows `dense` whatever the batch's size, zk_exec_plan's only from 1024 frames: kept as they were)
    if (p.lanes == 256 && (k.exec_ring ? k.exec_ring == 2 : dense)) p.ring = 4;
    if (k.seg_fill ? k.seg_fill == 2 : count >= 512) { p.fill_lanes = 256; p.fill_lds = false; }
    else if (k.seg_fill == 1) p.fill_lds = false;
    return p;
}

// ---- XXH64 (zk_launch_xxh64): a wave per frame, sixteen frames per wave (wide; lean: the same in 64 registers), or four frames per
// workgroup (zk_k_xxh64_fed<4>)
enum ZkXxhKernel { ZK_XXH_FRAME = 0 /* zk_k_xxh64 */, ZK_XXH_WIDE, ZK_XXH_LEAN, ZK_XXH_FED4 };
struct ZkXxhPlan { ZkXxhKernel kernel; uint32_t frames_per_wg; };
// a large batch: sixteen frames per wave (the chains' latency is the same, the instruction slots a sixteenth).  From how many frames (wide_from):
// the decoder's pass runs alone on the device or beside a neighbour's entropy stage -- 512 frames of 2 MiB: a wave per frame 5.3 / 6.5 ms
// per step against 5.9 / 7.6 (two batches in flight / one at a time), hence 1024; the encoder's runs beside its matcher, which pays for
// every instruction slot the checksums take -- measured from 512 frames in round 3, and left there
// (r6) the decoder's large batches: FOUR frames per workgroup, sixteen chains in one wave fed by another (zk_k_xxh64_fed<4>: 1.65 instead
// of 2.7 ms per 2 MiB frame, three times the instructions); the encoder's pass, beside its entropy stage and shorter than it either way
// (beside), keeps sixteen frames per wave; 2 / 3 pin the earlier forms for the tests and the probes.
// skip: the pass takes what zk_k_xxh64_follow left.  (With skip, xxh = 3 is the fed kernel, not the lean one, which knows no skip words,
// while xxh = 2 stays wide; xxh = 1 pins a wave per frame only without skip: kept as they were.)
inline ZkXxhPlan zk_xxh_plan_from(uint32_t count, const ZkKernelChoice &k, bool skip, uint32_t wide_from, bool beside)
{
    if (!skip && k.xxh == 3) return ZkXxhPlan{ZK_XXH_LEAN, 16};
    if (k.xxh == 2 || (beside && k.xxh == 0 && count >= wide_from)) return ZkXxhPlan{ZK_XXH_WIDE, 16};
    if (skip || k.xxh >= 4 || (k.xxh == 0 && count >= wide_from)) return ZkXxhPlan{ZK_XXH_FED4, 4};
    return ZkXxhPlan{ZK_XXH_FRAME, 1};
}
// the decoder's pass, with or without a follower before it, and zk_xxh64_frames_dev
inline ZkXxhPlan zk_xxh_plan(uint32_t count, const ZkKernelChoice &k, bool skip) { return zk_xxh_plan_from(count, k, skip, 1024, false); }
// the encoder's pass
inline ZkXxhPlan zk_xxh_plan_enc(uint32_t count, const ZkKernelChoice &k) { return zk_xxh_plan_from(count, k, false, 512, true); }

// the checksums beside the executor (zk_launch_xxh64_follow), in waves of 64 lanes
struct ZkXxhFollowPlan { bool follow1; uint32_t grid; };      // zk_k_xxh64_follow1 (a wave per frame) or zk_k_xxh64_follow
inline ZkXxhFollowPlan zk_xxh_follow_plan(uint32_t count)
{
    // a handful of frames: a wave per frame (a frame's chains run 1.7 ms per 2 MiB there, 2.25 ms sixteen frames to a wave)
    if (count <= 32) return ZkXxhFollowPlan{true, 8 * ((count + 7) / 8)};
    // eight waves per 128 frames: each takes the frames of one XCD
    return ZkXxhFollowPlan{false, 8 * ((count + 127) / 128)};
}

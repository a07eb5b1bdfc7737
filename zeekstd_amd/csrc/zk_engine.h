// zk_engine.h -- engine object shared by the decode / encode halves of the C ABI
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "zk_enc_device.h"
#include "zk_kernels.h"
#include "zk_dec_plan.h"

enum { ZK_K_WALK_COUNT = 0, ZK_K_SCAN, ZK_K_WALK_FILL, ZK_K_HUF, ZK_K_FSE, ZK_K_EXEC, ZK_K_XXH64, ZK_K_STATUS,
       ZK_K_ENC_MATCH, ZK_K_ENC_ENTROPY, ZK_K_ENC_COMPACT, ZK_K_ENC_XXH64, ZK_K_ENC_FSE_BUILD, ZK_K_ENC_DENSE,
       ZK_K_RANGE_PLAN, ZK_K_RANGE_PIECES, ZK_K_RANGE_GATHER, ZK_K_RANGE_STATUS,
       ZK_K_TRAIN_COUNT, ZK_K_TRAIN_SELECT, ZK_K_TRAIN_STATS, ZK_K_CDC_MARK, ZK_K_CDC_SELECT,
       ZK_K_DEDUP_HASH, ZK_K_DEDUP_INSERT, ZK_K_DEDUP_VERIFY, ZK_K_DEDUP_VERIFY_LONG, ZK_K_DEDUP_COMPACT, ZK_K_DEDUP_GATHER,
       ZK_K_DXI_INSERT, ZK_K_DXI_LOOKUP, ZK_K_DXI_COMPARE, ZK_K_DXI_EMIT,
       ZK_K_CMP_MARK, ZK_K_CMP_EMIT, ZK_K_CMP_MOVE, ZK_K_CMP_REMAP, ZK_K_CMP_TAKE,
       ZK_K_VIEW_PLAN, ZK_K_VIEW_MARK, ZK_K_VIEW_GATHER, ZK_K_VIEW_STATUS,
       ZK_K_DIGEST_PLAN, ZK_K_DIGEST_LEAVES, ZK_K_DIGEST_ROOTS, ZK_NKERNELS };

struct zk_devbuf { void *p = nullptr; size_t cap = 0; };
enum { ZK_MAX_CTX = 6 };

struct zk_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    char devname[320] = {0};
    std::string last_err;
    uint64_t *h_words = nullptr;            // pinned: small read-backs of the encoder (total size)
    // decode contexts: own queues (st + aux: kernels with no mutual dependency overlap, huf || fse), scratch and pinned
    // read-back words, so that several batches can be in flight -- the tail of one (checksum kernel: a per-frame serial
    // chain) overlaps the head of the next.  Context 0 serves the synchronous entry points (its main queue is the engine's
    // `stream`), 0 and 1 zk_decode_submit_dev, all of them the host-pointer pipeline; created on first use.
    struct DecCtx {
        hipStream_t st = nullptr, aux = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_exec = nullptr;
        zk_devbuf infos, bases, words, blocks, seqs, lit, prog;     // prog: the executor's progress words (zk_k_xxh64_follow)
        zk_devbuf seg_tab, seg_cnt, seg_holes, seg_tiles;            // the executor in segments: ZkSeg records, per-frame / per-segment counts, hole records, tile counts
        zk_devbuf rng, rng_meta;     // byte-range reads (zk_engine_ranges.hip): the decoded frames of one pass, the plan's arrays
        uint64_t *h_words = nullptr;
        bool ready = false;
        bool fused = false;          // the batch enqueued last took zk_k_entropy_frame
    } dctx[ZK_MAX_CTX];
    bool slot_busy[2] = {false, false};
    int next_slot = 0;
    // staging for the host-pointer entry points
    zk_devbuf st_comp, st_off, st_dst, st_misc;
    zk_devbuf rf_entries, rf_frames;        // zk_refine_entries_dev (zk_refine.hip): scratch per entry, per piece
    // staged device copy of a raw-content prefix.  The host-pointer Level-A calls upload it on EVERY call (no caching by
    // address: a caller may reuse one buffer for different bases).  A zeekstd::Decoder / Encoder, whose contract is the
    // reference's borrow ("the prefix stays unchanged while it is referenced", decode.rs:201), keeps its upload across its
    // own calls through zk_engine_stage_prefix: owner + address + length name the staged bytes.
    zk_devbuf st_prefix;
    const void *st_prefix_owner = nullptr, *st_prefix_src = nullptr; uint64_t st_prefix_len = 0;
    // the dictionary every decode call applies (zk_engine_set_dictionary; zk_dict.h): the engine's own device copy --
    // [block entry | entropy section as a block's content | content] -- uploaded once
    struct Dict {
        bool on = false, tables = false;    // tables: a formatted dictionary
        uint32_t id = 0, rep[3] = {1, 4, 8};
        zk_devbuf buf;
        const ZkBlock *d_tmpl = nullptr; const uint8_t *d_img = nullptr, *d_content = nullptr;
        uint64_t content_len = 0;
    } dict;
    struct zk_hostpipe *hp = nullptr;       // host-pointer pipeline (pinned staging, copy queues, worker threads): zk_engine_host.hip
    int host_threads = 0;                   // zk_engine_set_host_threads (0 = default)
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg)
    bool profiling = false;
    ZkKernelChoice choice;           // zk_engine_set_kernel_choice: all zero = by batch shape
    uint64_t followed = 0;           // frames of the last finished decode whose checksums zk_k_xxh64_follow verified (zk_engine_checksums_followed)
    bool entropy_fused = false;      // the last finished decode ran zk_k_entropy_frame, not zk_k_huf || the sequence kernels (zk_engine_entropy_fused)
    int pipe_contexts = 0;           // host pipeline: decode contexts in flight (0 = default) and chunk size, zk_hostpipe_tune
    uint64_t pipe_chunk_bytes = 0;
    uint64_t range_pass_bytes = 0;   // zk_read_ranges*: decoded bytes per pass (0 = ZK_RANGE_PASS_DEFAULT), ZK_CHOICE_RANGE_PASS_MIB
    uint64_t ranges_frames = 0;      // frames the last zk_read_ranges* call decoded (zk_engine_ranges_frames_decoded)
    hipEvent_t ev_start[ZK_NKERNELS] = {}, ev_stop[ZK_NKERNELS] = {};
    bool ev_used[ZK_NKERNELS] = {};
    float kernel_ms[ZK_NKERNELS] = {};
    // the encoder: one encode in flight (zk_engine_enc.hip).  Device scratch, named as the launchers of zk_kernels.h name what it holds
    struct Enc {
        zk_devbuf lists;                    // frames | blocks: the device copy of the pinned lists
        zk_devbuf seqs;                     // packed sequences, behind them the match positions (mpos)
        zk_devbuf lits;                     // literals
        zk_devbuf scratch;                  // per-block output of the entropy stage
        zk_devbuf words;                    // per frame: c_size64, out_off, hashes, d_off; behind them the predefined tables
        zk_devbuf ftab;                     // the frames' tables
        uint8_t *pin = nullptr; size_t pin_cap = 0;   // pinned host copy of the frame / block lists of the encode in flight
        uint8_t *pin_off = nullptr; size_t pin_off_cap = 0;   // zk_encode_frame_list_dev: the caller's offsets, brought to the host
        uint8_t *pin_lf = nullptr; size_t pin_lf_cap = 0;     // ... and, under a frame list with in-frame far history, of the records of the frames that have a table (ZkEncLdmFrame)
        zk_devbuf hist;                     // prefix mode: [prefix tail | frame] records for the matcher
        zk_devbuf seg;                      // frames above ZKE_SEGMENT: the matcher's segment records
        zk_devbuf dense;                    // dense far history (level 0 / >= 3, frames beyond the ring's reach): a candidate per input byte (ZkEncLdm::dense)
        zk_devbuf ldm;                      // prefix beyond the matcher's ring: the long-distance table (ZkEncLdm)
        zk_devbuf plan;                     // a frame list planned on the device: the frames' running sums (ZkEncPlanSum, zk_enc_plan_dev.h)
        zk_devbuf train, train_src;         // zk_train_dictionary*: its scratch (zk_train.hip); the host entry point's upload of the samples and their offsets
        zk_devbuf cdc, cdc_src, cdc_off;    // zk_chunk_boundaries*: a slice's scratch (zk_cdc.hip); the host entry point's upload of a slice, and its offsets
        zk_devbuf dd, dd_src, dd_off, dd_dry, dd_up, dd_out;    // zk_dedup_frames* / zk_encode_dedup* (zk_dedup.hip): the map's scratch (ZkDedupLayout); a gathered slice of unique frames and its offsets; a slice encoded for its size only; the host entry points' upload of source and offsets, and their outputs
        uint8_t *pin_dd = nullptr; size_t pin_dd_cap = 0;     // ... the caller's offsets and the unique frames' indices, brought to the host
        zk_devbuf dx;                       // zk_dedup_against_dev / zk_encode_dedup_against_dev (zk_dedup_index.hip): the lookup's scratch (ZkDxLayout); the decoded candidates of a pass lie in dctx[0].rng
        zk_devbuf cmp, cmp_gaps, cmp_stage; // zk_compact_archive_dev and its siblings (zk_compact.hip): the scratch (ZkCmpLayout); the gaps of an in-place compaction's steps; a staged step's bytes
        zk_devbuf dg, dg_up;                // zk_frame_digests* / zk_archive_digests_dev (zk_digest.hip): the leaf counts, their prefix sums and the leaf digests (ZkgLayout); the host entry point's upload of source and offsets, and its digests
        int plan_choice = 0;                // ZK_CHOICE_ENC_PLAN
        uint32_t dedup_key_bits = 0;        // zk_dedup_frames*: bits of a frame's key that are kept (0 = all 64), ZK_CHOICE_DEDUP_KEY_BITS
        uint64_t dedup_slice_bytes = 0;     // zk_encode_dedup*: bytes of unique frames gathered and encoded at a time (0 = 1 GiB), ZK_CHOICE_DEDUP_SLICE_KIB
        uint64_t dedup_pass_bytes = 0;      // zk_dedup_against_dev, zk_dedup_index_add_archive_dev: decoded bytes of archive frames held at a time (0 = 1 GiB), ZK_CHOICE_DEDUP_PASS_KIB
        uint64_t compact_slice_bytes = 0;   // zk_compact_archive_dev in place: destination bytes moved per step (0 = 256 MiB), ZK_CHOICE_COMPACT_SLICE_KIB
        uint64_t cdc_slice_bytes = 0;       // zk_chunk_boundaries*: input bytes whose candidates are held at a time (0 = 64 MiB), ZK_CHOICE_CDC_SLICE_KIB
        uint64_t train_trial_bytes = 0;     // zk_train_dictionary*: sample bytes the candidates are tried on (0 = 64 MiB), ZK_CHOICE_TRAIN_TRIAL_KIB
        uint64_t dense_slice_bytes = 0;     // input bytes the dense scratch is reserved for (0 = 4 GiB), ZK_CHOICE_ENC_DENSE_SLICE_KIB
        uint64_t dict_slice_bytes = 0;      // dictionary route: bytes of [content tail | frame] records staged at a time (0 = 1 GiB), ZK_CHOICE_ENC_DICT_SLICE_KIB
        ZkEncTables tables;
        bool tables_ready = false;
        // second queue: the checksum kernel (one serial chain per frame) runs beside the entropy stage; created on first use
        hipStream_t aux = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    } enc;
};

// every HIP call of the engine's host code: the error text is kept for zk_engine_last_hip_error
#define ZK_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t _e = (call);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            e->last_err = std::string(#call) + ": " + hipGetErrorString(_e);                         \
            return ZK_ERR_HIP;                                                                       \
        }                                                                                            \
    } while (0)

int zk_devbuf_reserve(zk_engine *e, zk_devbuf &b, size_t bytes);
int zk_pin_reserve(zk_engine *e, uint8_t *&p, size_t &cap, size_t bytes);      // the same for a pinned host buffer (contents are not kept)

// ---- decode plumbing shared by zk_engine.hip (device-pointer entry points), zk_engine_host.hip (host pipeline, small path) and
// zk_engine_ranges.hip.  Every stage takes the context and the queue to run on: zk_dec_stream.
struct zk_dec_args {
    const void *d_comp; uint64_t comp_size; const void *d_c_off, *d_d_off; uint32_t first, count;
    const uint32_t *ids; const uint64_t *out_off;       // frame list (device arrays, both or neither)
    void *d_dst; uint64_t dst_cap; int verify; void *d_frame_status;
    const void *d_prefix; uint64_t prefix_len;
    bool alone = false;                                 // nothing else of this engine is in flight (the synchronous entry points): zk_k_xxh64_follow
    bool neighbour = false;                             // a batch of this engine is in flight on the other context as this one is enqueued: zk_exec_plan
    bool single_queue = false;                          // huf and fse on the context's main queue (the host pipeline overlaps whole chunks instead)
    bool mark_exec = false;                             // record the context's ev_exec behind the executor (output bytes final, checksums pending)
};
int zk_dec_ctx_aux(zk_engine *e, zk_engine::DecCtx &c); // the context's second queue + fork / join events, on first use
int zk_dec_ctx_ready(zk_engine *e, int slot);           // creates the context's queues / events on first use
// the queue a decode on context c runs on: the caller's for context 0 when one is given, the context's own otherwise
inline hipStream_t zk_dec_stream(zk_engine *e, zk_engine::DecCtx &c, void *stream) { return &c == &e->dctx[0] && stream ? (hipStream_t)stream : c.st; }
inline ZkDecShape zk_dec_shape(const zk_engine *e, uint32_t count, uint64_t out_bytes, uint64_t max_frame, uint64_t nblocks, bool has_prefix, bool alone)
{
    return ZkDecShape{e->choice, e->profiling, count, out_bytes, max_frame, nblocks, has_prefix, alone, false};
}
int zk_decode_enqueue(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a);
int zk_decode_finish(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st);
// the stages of a decode (zk_engine.hip), in the order zk_decode_enqueue runs them; a.d_comp ... a.dst_cap name the frames
int zk_dec_frame_tables(zk_engine *e, zk_engine::DecCtx &c, uint32_t count);            // infos / bases / words for `count` frames
// counting walk + scan; blocks until the first `nwords` of the ZK_SCAN_* words are in c.h_words
int zk_dec_count_pass(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a, bool with_dict, uint32_t nwords);
int zk_dec_block_scratch(zk_engine *e, zk_engine::DecCtx &c, uint64_t nblocks, uint64_t nseq);    // blocks / seqs
// the frame walk: the counting pass's (fill = false: no block entries yet), the filling one
void zk_dec_walk(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a, bool with_dict, uint64_t nblocks, bool fill);
// scratch of the executor in segments; nblocks: the batch's block count or a bound of it
int zk_dec_seg_scratch(zk_engine *e, zk_engine::DecCtx &c, uint32_t count, const ZkSegPlan &sp, uint64_t out_bytes, uint64_t nblocks, ZkSegScratch &sgs);
// the checksums beside the executor: its progress words (cleared on st) and the context's second queue
int zk_dec_follow_prepare(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, uint32_t count, uint64_t **prog);
int zk_dec_fork(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st);     // the second queue goes on from where st is now
// the executor (sgs: in segments; its kernels planned from shape and nseq, 0 = not known), ev_exec when a.mark_exec, then the checksums: zk_k_xxh64_follow
// on the second queue and what it left when `prog` (zk_dec_follow_prepare + zk_dec_fork came first), the plain pass when a.verify, else none
int zk_dec_exec_checksums(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a, const ZkSegScratch *sgs, const ZkDecShape &shape,
                          uint64_t nseq, uint64_t *prog, const uint32_t *rep_init);
// does this call decode against the engine's dictionary?  (an explicit prefix overrides it, as ZSTD_DCtx_refPrefix does)
// is a batch of zk_decode_submit_dev outstanding?  What an entry point refuses for (the table above zk_decode_submit_dev, zeekstd_amd.h) it refuses
// with this, before it reserves, uploads or waits for anything
inline bool zk_batch_outstanding(const zk_engine *e) { return e->slot_busy[0] || e->slot_busy[1]; }
inline bool zk_dict_applies(const zk_engine *e, const void *d_prefix) { return e->dict.on && !d_prefix; }
// what zk_dedup_index_compact_dev (zk_compact.hip) reaches the index through (zk_dedup_index.hip): its arrays, and the table rebuilt for m
// frames whose keys and lengths are in place (zk_dedup_index_truncate's path; the stream is synchronised)
struct zk_dedup_index;
struct ZkDxArrays { zk_engine *e; uint32_t m; uint64_t *keys; uint32_t *lens; };
ZkDxArrays zk_dedup_index_arrays(zk_dedup_index *x);
int zk_dedup_index_rebuilt(zk_dedup_index *x, hipStream_t st, uint32_t m);
namespace zeekstd { class SeekTable; }
struct zk_seek_table;
zk_seek_table *zk_seek_table_from_cpp(const zeekstd::SeekTable *t);
int zk_hostpipe_create(zk_engine *e);
void zk_hostpipe_destroy(zk_engine *e);
void zk_hostpipe_tune(zk_engine *e);                    // applies zk_engine::pipe_contexts / pipe_chunk_bytes (between calls)
enum { ZK_HW_ENC_TOTAL = 8, ZK_HW_RANGES = 10, ZK_HW_ENC_PLAN = 13 };   // index into zk_engine::h_words of the encoder's total-size read-back; of the three words zk_read_ranges_dev reads back; of the three words of a device plan's totals (ZkEncPlanSum)
constexpr uint64_t ZK_RANGE_PASS_DEFAULT = 1ull << 30;
// A compiled dictionary (zk_cdict_create; zk_enc_dict.h): the device copies an encode against it reads.  It belongs to the engine it was made on.
struct ZkEncDictDev;
struct zk_cdict {
    zk_engine *e = nullptr;
    uint32_t id = 0, id_width = 0;
    bool formatted = false;
    void *d_content = nullptr;              // the content's last `content_len` bytes (what the matcher can reach: zke_ldm_usable) + ZKE_LDM_SLACK
    uint64_t content_len = 0;
    ZkEncDictDev *d_tab = nullptr;          // formatted dictionaries: the compression side of the four tables
};
// where the matcher left its output: what an encode that stops behind zk_enc_match hands back (zk_enc_args::matched)
struct ZkEncMatched { const ZkEncBlock *blocks; uint32_t nb; const uint64_t *seqs; const uint8_t *lits; };
struct zk_enc_args {
    const void *d_src; uint64_t n; uint32_t frame_size; int level, checksum;
    const void *d_prefix; uint64_t prefix_len; void *d_dst; uint64_t dst_cap; void *d_c_sizes, *d_d_sizes;
    // the dictionary route: d_prefix / prefix_len are the dictionary's content (the caller sets them from it); the frames name cdict->id, the
    // records are staged in slices, and with a formatted dictionary the entropy stage runs its dictionary variants
    const zk_cdict *cdict = nullptr;
    // a caller-given frame list (zk_encode_frame_list*): list[list_count + 1] non-decreasing prefix sums in HOST memory, checked by the entry
    // point; frame i is d_src[list[i] - list[0], list[i + 1] - list[0]), n = list[list_count] - list[0], and frame_size is the largest frame
    // (at least 1).  nullptr: frames of frame_size bytes.
    const uint64_t *list = nullptr; uint32_t list_count = 0;
    // ... planned on the device (zk_enc_plan_dev.h): the caller's offsets there, the frames' running sums (zk_k_enc_plan_scan has run) and, on the
    // host, the totals behind them; all null: the host plans
    const uint64_t *d_list = nullptr; const struct ZkEncPlanSum *d_plan_sums = nullptr, *plan_totals = nullptr;
    // run the stages up to and including zk_enc_match only, and say here where the blocks, sequences and literals lie (device memory of the
    // engine, valid until its next encode); nothing is written to d_dst.  nullptr: the whole encode
    ZkEncMatched *matched = nullptr;
};
// the entry points' check of a frame list (ZK_ERR_ARGUMENT / ZK_ERR_FRAME_INDEX_TOO_LARGE); *max_frame: the largest frame
int zk_enc_list_check(const uint64_t *off, uint32_t count, uint64_t *max_frame);
// what a destination of an encode must hold for the call never to ask: zk_compress_bound, on the dictionary route zk_compress_bound_dict
uint64_t zk_enc_bound(const zk_enc_args &a);
int zk_encode_enqueue(zk_engine *e, const zk_enc_args &a, hipStream_t st, uint32_t *nf_out);
int zk_encode_finish(zk_engine *e, hipStream_t st, uint64_t *written_out);
// zk_encode_frame_list_dev on the prefix route up to and including the match stage (zk_enc_args::matched); the stream is left running
int zk_encode_frame_list_matched(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, const void *d_prefix, uint64_t prefix_len,
                                 void *d_dst, uint64_t dst_cap, ZkEncMatched *matched, hipStream_t st);

// ---- host pipeline, C++ face (the C ABI's host-pointer functions and the zeekstd:: host classes sit on these)
// Where the compressed bytes of a host decode come from: contiguous memory, or a pull callback that delivers the n bytes
// at payload offset `off` straight into pinned staging (Seekable sources: files, callbacks).  Returns bytes delivered.
struct zk_host_src {
    const uint8_t *mem = nullptr;
    size_t (*read)(void *user, uint64_t off, uint8_t *dst, size_t n) = nullptr;
    void *user = nullptr;
};
// Decode frames [first, first + count) into dst (frame `first` at dst[0]); c_off / d_off are the archive's prefix sums and
// the source is addressed with them.  d_prefix: DEVICE copy of the raw-content prefix (or nullptr).  n_ok (optional):
// number of leading frames that decoded fine (bytes of those frames in dst are valid even when the call fails).
int zk_host_decode(zk_engine *e, const zk_host_src &src, const uint64_t *c_off, const uint64_t *d_off, uint32_t first, uint32_t count,
                   const void *d_prefix, uint64_t prefix_len, uint8_t *dst, uint64_t dst_cap, int verify, int32_t *frame_status,
                   uint32_t *n_ok);
// Encode src[0, n) as frames of frame_size bytes; every finished chunk of frames is handed to `sink` (pinned memory,
// valid during the call): the compressed bytes and the chunk's seek entries.  sink returns 0 to go on.
typedef int (*zk_host_sink)(void *user, const uint8_t *data, uint64_t n, const uint32_t *c_sizes, const uint32_t *d_sizes, uint32_t n_frames);
int zk_host_encode(zk_engine *e, const uint8_t *src, uint64_t n, uint32_t frame_size, int level, int checksum, const void *d_prefix,
                   uint64_t prefix_len, zk_host_sink sink, void *user, const zk_cdict *cdict = nullptr,      // cdict: d_prefix / prefix_len are its content
                   const uint64_t *list = nullptr, uint32_t list_count = 0);                                // a frame list (zk_enc_args::list): src is its first byte, frame_size its largest frame
// Upload (or reuse) the device copy of a prefix on behalf of `owner`; returns the device pointer in *d_out.
int zk_engine_stage_prefix(zk_engine *e, const void *owner, const uint8_t *prefix, uint64_t len, bool force, const void **d_out);
// multi-threaded memcpy on the engine's worker threads (large host-side copies of the zeekstd:: classes)
void zk_host_copy(zk_engine *e, void *dst, const void *src, size_t n);

// RAII-free helper: brackets one launch with events when profiling is on (and `on`)
struct zk_kernel_timer {
    zk_engine *e; int k; hipStream_t st; bool on;
    zk_kernel_timer(zk_engine *e_, int k_, hipStream_t st_, bool on_ = true) : e(e_), k(k_), st(st_), on(on_ && e_->profiling) {
        if (on) { (void)hipEventRecord(e->ev_start[k], st); e->ev_used[k] = true; }
    }
    ~zk_kernel_timer() { if (on) (void)hipEventRecord(e->ev_stop[k], st); }
};
// per-kernel events describe one synchronous batch: everything else runs with profiling off for a scope
struct zk_profiling_off {
    zk_engine *e; bool was;
    explicit zk_profiling_off(zk_engine *e_, bool off = true) : e(e_), was(e_->profiling) { if (off) e->profiling = false; }
    ~zk_profiling_off() { e->profiling = was; }
};
void zk_profile_begin(zk_engine *e);
void zk_profile_collect(zk_engine *e);

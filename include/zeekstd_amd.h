/*
 * zeekstd_amd.h -- C ABI of the MI355X-native seekable-zstd engine (libzeekstd_amd.so).
 *
 * This is the FFI a Rust/C/C++/Python host binds instead of the libzstd symbols that
 * zeekstd reaches through zstd-safe (reference boundary: SURVEY.md 8b; call sites
 * lib/src/encode.rs:281-284,336,341-345,444-448,504-506,599 and
 * lib/src/decode.rs:181,184,213,243-245,250-253,354-356).  libzstd's streaming ABI moves
 * <= 128 KiB per call through one context; a GPU wants whole frames, many at a time, so the
 * boundary is re-cut one level up: "N frames in, N frames out" (Level A below), and the
 * zeekstd types (EncodeOptions / RawEncoder / Encoder / DecodeOptions / Decoder / SeekTable /
 * Serializer / Seekable / BytesWrapper) are restated on top of it (Level B, zk_* handle API
 * further down and the C++ classes in zeekstd_amd/csrc/host/zeekstd.hpp).
 *
 * Conventions
 *   - plain pointers and sizes, no C++/torch types; all functions are thread-compatible:
 *     one handle may be used by one thread at a time (libzstd CCtx/DCtx rule).
 *   - return value: 0 on success, negative on error.  -(ZSTD_ErrorCode) for codec errors
 *     (e.g. -20 corruption_detected, -22 checksum_wrong, -10 prefix_unknown, -70
 *     dstSize_tooSmall, -72 srcSize_wrong) exactly the codes zeekstd wraps in Kind::Zstd
 *     (lib/src/error.rs:40-45); zeekstd's own kinds map to the ZK_ERR_* values below.
 *   - "_dev" entry points take DEVICE pointers (HBM resident) and a hipStream_t passed as
 *     void*; the plain ones take HOST pointers and stage through the engine's buffers.
 *     The engine launches on its OWN queues (non-blocking streams; the stream argument, where
 *     there is one, replaces the main one): work the caller still has in flight on other
 *     streams for a buffer it passes -- the kernel that produces the input, the fill of a fresh
 *     output -- must have completed before the call, as for any two unordered HIP streams.
 *   - there is no CPU fallback: if no gfx950 device is usable, zk_engine_create fails.
 */
#ifndef ZEEKSTD_AMD_H
#define ZEEKSTD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_ABI_VERSION 2

/* zeekstd error kinds (lib/src/error.rs:101-113) that are not ZSTD_ErrorCode values */
#define ZK_ERR_OFFSET_OUT_OF_RANGE (-1001)
#define ZK_ERR_FRAME_INDEX_TOO_LARGE (-1002)
#define ZK_ERR_NUMBER_CONVERSION (-1003)
#define ZK_ERR_IO (-1004)
/* engine-level failures (no reference counterpart) */
#define ZK_ERR_HIP (-2001)       /* a HIP runtime call failed; see zk_engine_last_hip_error */
#define ZK_ERR_NO_DEVICE (-2002) /* no usable gfx950 device / kernels not loadable */
#define ZK_ERR_ARGUMENT (-2003)

/* format constants (lib/src/lib.rs:52-62) */
#define ZK_SEEKABLE_MAGIC_NUMBER 0x8F92EAB1u
#define ZK_SEEKABLE_MAX_FRAMES 0x08000000u
#define ZK_SEEK_TABLE_INTEGRITY_SIZE 9
#define ZK_SEEKABLE_MAX_FRAME_SIZE 0x40000000u
#define ZK_SKIPPABLE_HEADER_SIZE 8

typedef struct zk_engine zk_engine;

int zk_abi_version(void);
/* Human readable name of an error code returned by any function here
 * (ZSTD_getErrorName strings for codec errors: lib/src/error.rs:68). */
const char *zk_error_name(int code);

/* ---------------------------------------------------------------- Level A: batch engine */
/* Owns one GPU (device ordinal), its scratch buffers and a private stream.
 * Replaces CCtx::create/DCtx::create (encode.rs:130, decode.rs:31). */
int zk_engine_create(int device, zk_engine **out);
void zk_engine_destroy(zk_engine *e);
const char *zk_engine_last_hip_error(const zk_engine *e);
/* name of the device the engine runs on, e.g. "gfx950..." */
const char *zk_engine_device_name(const zk_engine *e);

/* Per-kernel timing for roofline reports: when on, every kernel launch of the next decode/encode call is
 * bracketed by HIP events on the launch stream; zk_engine_kernel_times returns the last call's
 * durations in ms, indexed like zk_engine_kernel_name (0 <= k < zk_engine_kernel_count()). */
int zk_engine_set_profiling(zk_engine *e, int on);
/* Kernel selection of the sequence decoder for blocks that carry their own FSE tables (archives written by libzstd):
 * 0 = by batch size (default), 1 = one lane per block (zk_k_fse), 2 = a quad of lanes per block (zk_k_fse_quad).
 * Results are identical; the tests use it to run both kernels on small inputs. */
int zk_engine_set_fse_kernel(zk_engine *e, int mode);                /* = zk_engine_set_kernel_choice(e, ZK_CHOICE_FSE_OWN, mode) */
/* Pins one kernel variant whatever the batch looks like (value 0 = by batch shape, the default and what production runs).
 * Every variant computes the same bytes: the point is that tests/ can put the kernels of the large-batch path (which a 4 GiB
 * batch selects) under small, exhaustively checked inputs, and that tools/ can time one variant against another.  Replaces the
 * environment switches of round 3.  ZK_ERR_ARGUMENT for an unknown key or value. */
enum {
    ZK_CHOICE_RESET = 0,          /* every key back to 0 (value ignored) */
    ZK_CHOICE_FSE_OWN = 1,        /* blocks with own FSE tables: 1 zk_k_fse (a lane per block), 2 zk_k_fse_quad in its 56-block layout */
    ZK_CHOICE_FSE_SHARED = 2,     /* blocks that share tables: 1 zk_k_fse_predef, 2 zk_k_fse_predef_fed, 3 zk_k_fse_sets (any of them
                                   * also switches the small-batch shortcut "every block a quad" off) */
    ZK_CHOICE_EXEC_LANES = 3,     /* zk_k_exec tile: 128 / 256 / 512 / 1024 lanes */
    ZK_CHOICE_EXEC_RING = 4,      /* 256-lane tiles: 1 = a ring of 2 T records, 2 = 4 T */
    ZK_CHOICE_XXH64 = 5,          /* 1 zk_k_xxh64 (a wave per frame), 2 zk_k_xxh64_wide (sixteen frames per wave), 3 zk_k_xxh64_lean (the same in 64
                                   * registers), 5 zk_k_xxh64_fed<4> (four frames per workgroup: sixteen chains in one wave, their products
                                   * brought by another; large batches take it by themselves) -- behind the executor;
                                   * 4 zk_k_xxh64_follow: BESIDE the executor, behind its progress words, on the decode's second queue
                                   * (zk_engine_checksums_followed says how many frames it verified; what it leaves is checked behind the
                                   * executor as with 5).  By batch shape: 4 for a synchronous decode of >= 512 frames */
    ZK_CHOICE_SMALL_PATH = 6,     /* host-pointer decode of <= 64 frames: 1 = through the general pipeline, 2 = the small path with its
                                   * entropy roles as two kernels */
    ZK_CHOICE_PIPE_CONTEXTS = 7,  /* host pipeline: decode contexts it rotates through (1..6; 0 = 2) */
    ZK_CHOICE_PIPE_CHUNK_MIB = 8, /* host pipeline: output MiB per chunk (0 = by total size) */
    ZK_CHOICE_EXEC_RESIDENT = 9,  /* zk_k_exec with 256-lane tiles: at most this many workgroups per CU (4 or 5; the launch asks for LDS it does not use) */
    ZK_CHOICE_EXEC_SEG = 10,      /* the executor in segments, several workgroups per frame (zk_k_seg_prep / zk_k_exec_seg / zk_k_exec_fill): 1 never, 2 always
                                     (decodes without a prefix); 0 = by batch shape */
    ZK_CHOICE_SEG_KIB = 11,       /* ... output KiB per segment (1..128; 0 = 128, or 4 for short frames on the host-pointer small path) */
    ZK_CHOICE_SEG_FILL = 12,      /* ... its fill pass: 1 zk_k_exec_fill<1024> (rounds through memory), 2 zk_k_exec_fill<256>, 3 zk_k_exec_fill_lds (holes in LDS); 0 by batch size */
    ZK_CHOICE_ENTROPY = 13,       /* literals and sequences of a device-pointer batch: 1 = zk_k_huf beside the sequence kernels on two queues, 2 = one kernel
                                   * (zk_k_entropy_frame) for every batch that qualifies -- no frame with more than one set of own tables -- whatever its
                                   * size; 0 = by batch shape.  zk_engine_entropy_fused says which one ran */
    ZK_CHOICE_RANGE_PASS_MIB = 14, /* zk_read_ranges*, zk_read_view_ranges_dev: decoded MiB of scratch per pass (1..2^20; 0 = 1024).  A pass is never less than one frame */
    ZK_CHOICE_ENC_DENSE_SLICE_KIB = 15, /* encodes with dense far history (level 0 / >= 3, frames beyond the matcher's ring): input KiB whose candidate scratch
                                        * (8 bytes per input byte) is reserved at a time (1..2^22; 0 = 2^22, 4 GiB).  A longer input is matched slice after
                                        * slice of whole frames over that scratch, never less than one frame; the bytes produced do not depend on it */
    ZK_CHOICE_ENC_DICT_SLICE_KIB = 16, /* zk_encode_frames_dict*: KiB of [dictionary content | frame] records staged for the matcher at a time (1..2^22;
                                        * 0 = 2^20, 1 GiB).  A longer input is staged and matched slice after slice of whole frames over that buffer, never
                                        * less than one frame; the bytes produced do not depend on it */
    ZK_CHOICE_ENC_PLAN = 17,           /* zk_encode_frame_list_dev: where the frame / block / segment records are made: 0 = by the number of frames,
                                        * 1 = on the host (written and uploaded, 160 bytes per frame), 2 = on the device from the offsets.  The same
                                        * records, so the same bytes */
    ZK_CHOICE_TRAIN_TRIAL_KIB = 18,    /* zk_train_dictionary*: KiB of samples above which the candidates are tried, and the tables measured, on every j-th
                                        * sample (1..2^22; 0 = 2^16, 64 MiB).  Unlike the keys above it is part of the function: it decides which samples
                                        * the choice of k and the tables see.  The tests reach the rule with small inputs through it */
    ZK_CHOICE_CDC_SLICE_KIB = 19,      /* zk_chunk_boundaries*: input KiB whose candidates the engine holds at a time (1..2^22; 0 = 2^16, 64 MiB).  A longer
                                        * input is marked and selected slice after slice, the chain's cut carried across.  The offsets do not depend on it;
                                        * the scratch (up to 4 1/4 bytes per byte of a slice) does */
    ZK_CHOICE_DEDUP_KEY_BITS = 20,     /* zk_dedup_frames* / zk_encode_dedup*: only the low k bits of a frame's key (a 64-bit hash and the length) group the frames that
                                        * are then compared byte for byte (1..64; 0 = all 64).  The outputs do not depend on it: with 1-4 bits nearly every
                                        * frame meets a wrong leader and the rounds that settle one content per key run many times, which no real input
                                        * provokes.  Like ZK_CHOICE_TRAIN_TRIAL_KIB it lets small inputs reach the rule's rare path */
    ZK_CHOICE_DEDUP_SLICE_KIB = 21,    /* zk_encode_dedup*: KiB of unique frames gathered into engine scratch and encoded at a time, whole frames, one at
                                        * least (1..2^22; 0 = 2^20, 1 GiB).  The bytes do not depend on it; the scratch does */
    ZK_CHOICE_DEDUP_PASS_KIB = 22,     /* zk_dedup_against_dev / zk_encode_dedup_against_dev / zk_dedup_index_add_archive_dev: KiB of archive frames decoded
                                        * into engine scratch at a time, whole frames, one at least (1..2^22; 0 = 2^20, 1 GiB).  The results do not
                                        * depend on it; the scratch does */
    ZK_CHOICE_COMPACT_SLICE_KIB = 23   /* zk_compact_archive_dev in place: KiB of the destination moved per step, in whole tiles of 64 KiB, one at least
                                        * (1..2^22; 0 = 2^18, 256 MiB).  The bytes do not depend on it; the scratch (a staged step's bytes) and the
                                        * number of steps do.  It lets small inputs take many steps */
};
int zk_engine_set_kernel_choice(zk_engine *e, int what, int value);
/* Frames of the last finished device-pointer decode (zk_decode_frames_dev and its siblings, zk_decode_wait) whose Content_Checksum was
 * verified by zk_k_xxh64_follow, beside the executor; the others were verified behind it.  A diagnostic: results do not depend on it. */
uint64_t zk_engine_checksums_followed(const zk_engine *e);
/* 1 if the last finished device-pointer decode ran literals and sequences in one kernel (zk_k_entropy_frame), 0 if as two kernels side by
 * side.  A diagnostic: results do not depend on it. */
int zk_engine_entropy_fused(const zk_engine *e);
int zk_engine_kernel_count(void);
const char *zk_engine_kernel_name(int k);
int zk_engine_kernel_times(const zk_engine *e, float *ms_out, int n);

/*
 * Decode frames [first, first+count) of a seekable payload.
 *   comp      compressed payload; frame i occupies comp[c_off[i], c_off[i+1])
 *   c_off     n+1 prefix sums of compressed sizes   (SeekTable entries, seek_table.rs:97-131)
 *   d_off     n+1 prefix sums of decompressed sizes
 *   dst       receives the decompressed bytes of the range, frame `first` at dst[0];
 *             dst_cap >= d_off[first+count] - d_off[first]
 *   verify    != 0: verify Content_Checksum (XXH64 low 32 bits) of frames that carry one
 *   frame_status  optional, count entries: 0 or the ZSTD_ErrorCode of that frame
 * Replaces the ZSTD_decompressStream loop of decode.rs:242-256 for whole frames.
 * Returns 0, or -(code) of the first failing frame.
 */
int zk_decode_frames(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off,
                     const uint64_t *d_off, uint32_t first, uint32_t count, uint8_t *dst, uint64_t dst_cap,
                     int verify, int32_t *frame_status);
/* Same with every buffer resident in HBM (c_off/d_off/frame_status are device pointers too).
 * stream: hipStream_t (NULL = the engine's own stream).  Synchronises the stream before returning. */
#define ZK_COMP_PADDING 8 /* device-resident compressed buffers must be readable this many bytes past comp_size */
int zk_decode_frames_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off,
                         const void *d_d_off, uint32_t first, uint32_t count, void *d_dst, uint64_t dst_cap,
                         int verify, void *d_frame_status, void *stream);

/* Random-access batch (many seeks per submission; engine-specific, no reference counterpart -- the reference serves one
 * seek at a time, lib/src/decode.rs:402-437): decode archive frames d_ids[0..count) (uint32, any order, repeats allowed) of a
 * device-resident archive; frame d_ids[i] lands at d_dst + d_out_off[i], d_out_off being the count + 1 prefix sums of the
 * selected frames' decompressed sizes (uint64).  d_c_off / d_d_off are the archive's full n+1 prefix arrays. */
int zk_decode_frame_list_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                             const void *d_ids, const void *d_out_off, uint32_t count, void *d_dst, uint64_t dst_cap,
                             int verify, void *d_frame_status, void *stream);

/* Batched reads (the bulk form of set_offset / set_offset_limit / read, lib/src/decode.rs:402-437, which serves one seek at a time):
 * range i is bytes [d_offs[i], d_offs[i] + d_lens[i]) of the DECOMPRESSED stream (uint64 arrays of count entries) and lands at
 * d_dst + d_dst_off[i]; d_dst_off == NULL packs the ranges back to back in list order (prefix sums of the lengths, made on the
 * device; a range outside the stream takes no room).  d_c_off / d_d_off are the archive's full n_frames + 1 prefix arrays.  Ranges
 * may come in any order, overlap, repeat, be empty, cross any number of frames and exceed 4 GiB.  An offset on a frame boundary
 * belongs to the frame that starts there and empty frames are skipped (seek_table.rs:579-596).
 *   - exactly the bytes of the ranges are written: what lies between or behind the destinations stays untouched (destinations may
 *     be padded and aligned at will).  Destinations that overlap each other are the caller's error and are not detected.
 *   - every frame some range touches is decoded once, into scratch of the engine, whatever number of ranges touch it; the others,
 *     and frames of decompressed size 0, are not decoded.  The scratch holds at most ZK_CHOICE_RANGE_PASS_MIB of decoded frames (1 GiB
 *     by default, one frame at least): a call that touches more runs in passes.  zk_engine_ranges_frames_decoded counts the frames.
 *   - verify != 0: the Content_Checksum of every touched frame that carries one is verified, over the whole frame.
 *   - d_range_status (optional, int32, count entries): 0; ZK_ERR_OFFSET_OUT_OF_RANGE for a range that leaves the stream, -70
 *     (dstSize_tooSmall) for one whose destination leaves dst_cap -- such a range writes nothing, the others are served --; or
 *     -(ZSTD_ErrorCode) of the first frame it touches that failed to decode or verify -- its bytes are then unspecified within its own
 *     destination, ranges that touch good frames only are delivered all the same.
 * Returns 0, or the status of the first failing range in list order; engine errors as everywhere.  There is no prefix mode.
 * zk_read_ranges: host pointers; only the compressed bytes of touched frames are uploaded. */
int zk_read_ranges_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                       const void *d_offs, const void *d_lens, const void *d_dst_off, uint32_t count,
                       void *d_dst, uint64_t dst_cap, int verify, void *d_range_status, void *stream);
int zk_read_ranges(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, const uint64_t *d_off, uint32_t n_frames,
                   const uint64_t *offs, const uint64_t *lens, const uint64_t *dst_off, uint32_t count,
                   uint8_t *dst, uint64_t dst_cap, int verify, int32_t *range_status);
/* Frames the last zk_read_ranges* / zk_read_view_ranges_dev call decoded (every touched frame once).  A diagnostic. */
uint64_t zk_engine_ranges_frames_decoded(const zk_engine *e);

/* Batched reads of a VIEW of a device-resident archive: what a chunk store keeps of a snapshot.  A view is d_view_ids[view_count] (uint32
 * archive frames, any order, repeats allowed) and d_view_off[view_count + 1] (uint64, non-decreasing; d_view_off[0] need not be 0) -- the
 * ids / off pair zk_dedup_frames, zk_encode_dedup[_against]_dev and DedupStore.append return.
 * THE RULE, a pure function of the decoded archive frames, the view and the ranges:
 *   - the view's stream is the decoded bytes of frame view_ids[0], then view_ids[1], ...: the byte at coordinate view_off[j] + p is byte p
 *     of the decoded archive frame view_ids[j].
 *   - range i is [d_offs[i], d_offs[i] + d_lens[i]) in the coordinates of view_off and lands at d_dst + d_dst_off[i]; d_dst_off == NULL packs
 *     the ranges in list order (a range outside the stream takes no room).  Ranges may overlap, repeat, be empty, come in any order, cross
 *     any number of entries and exceed 4 GiB, as the stream may.  An offset on an entry boundary belongs to the entry that starts there and
 *     empty entries are skipped (zk_read_ranges_dev's edge rule, over view_off).
 *   - the view is checked WHOLE before anything is decoded or written, whether a range touches an entry or not: every view_ids[j] < n_frames,
 *     view_off non-decreasing, view_off[j + 1] - view_off[j] == d_off[view_ids[j] + 1] - d_off[view_ids[j]].  Anything else: ZK_ERR_ARGUMENT,
 *     d_dst and d_range_status untouched.
 *   - d_range_status (optional, int32, count entries): 0; ZK_ERR_OFFSET_OUT_OF_RANGE for a range that leaves [view_off[0],
 *     view_off[view_count]] or whose off + len overflows; -70 (dstSize_tooSmall) for one whose destination leaves dst_cap -- such a range
 *     writes nothing, its neighbours are served --; or -(ZSTD_ErrorCode) of the first entry, in VIEW order, that it touches and whose frame
 *     failed to decode or verify -- its bytes are then unspecified within its own destination, the other ranges are delivered all the same.
 *   - exactly the bytes of the good ranges are written: nothing between or behind the destinations.
 *   - every archive frame is decoded AT MOST ONCE per call, however many entries name it and however many ranges touch those entries, into
 *     scratch of the engine bounded by ZK_CHOICE_RANGE_PASS_MIB (passes are slices of the sorted list of distinct frames, one frame at least);
 *     frames that no touched, non-empty entry names are not decoded.  zk_engine_ranges_frames_decoded: the distinct frames decoded.
 *   - verify, an engine dictionary, ZK_COMP_PADDING and `stream` as for zk_read_ranges_dev.  There is no prefix mode.  count == 0 returns 0.
 * Returns 0, or the status of the first failing range in list order; engine errors as everywhere.  With the identity view (view_ids = 0 ..
 * n_frames - 1, view_off = d_off) the call is zk_read_ranges_dev: same bytes, statuses, return value and frame count. */
int zk_read_view_ranges_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                            const void *d_view_ids, const void *d_view_off, uint32_t view_count,
                            const void *d_offs, const void *d_lens, const void *d_dst_off, uint32_t count,
                            void *d_dst, uint64_t dst_cap, int verify, void *d_range_status, void *stream);

/* Decode with a raw-content prefix (patch mode): what the reference does with ZSTD_DCtx_refPrefix before the first
 * frame and again after every frame end (lib/src/decode.rs:212-214, 248-255) -- every frame of the batch sees the
 * same prefix right before its first byte and a match may start up to prefix_len bytes before the frame.  With a
 * prefix an offset is bounded by availability only (libzstd's ZSTD_execSequence), not by the frame's window.
 * prefix_len may not exceed 2^30 - 2^27 bytes (-16 window_too_large otherwise); prefix_len == 0 is the plain call. */
int zk_decode_frames_prefix_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off,
                                const void *d_d_off, uint32_t first, uint32_t count, const void *d_prefix, uint64_t prefix_len,
                                void *d_dst, uint64_t dst_cap, int verify, void *d_frame_status, void *stream);
int zk_decode_frames_prefix(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off,
                            const uint64_t *d_off, uint32_t first, uint32_t count, const uint8_t *prefix, uint64_t prefix_len,
                            uint8_t *dst, uint64_t dst_cap, int verify, int32_t *frame_status);

/* Decode frames that were compressed with a zstd dictionary (what the reference reaches through DecodeOptions::with_dctx, decode.rs:43,
 * with a context the caller has loaded a dictionary into; ZSTD_DCtx_loadDictionary).
 * zk_dict_create parses and validates the bytes on the host (no GPU needed) and copies them.  Bytes that begin with 0xEC30A437 are a
 * formatted dictionary (RFC 8878 section 5: magic, Dictionary_ID, Huffman tree description, FSE descriptions of offsets, match lengths and
 * literal lengths, three repeat offsets, content); -30 (dictionary_corrupted) when its entropy section is truncated or invalid or a
 * repeat offset is 0 or larger than the content.  Anything else is a raw-content dictionary: ID 0, no tables, repeat offsets 1 / 4 / 8, every
 * byte content.  Content beyond 2^30 - 2^27 bytes: -16, as for a prefix.
 * zk_engine_set_dictionary uploads the dictionary once (the engine keeps its own device copy: the zk_dict may be freed right away);
 * NULL = none.  ZK_ERR_ARGUMENT while a submitted batch is outstanding (zk_decode_wait first).  With a dictionary set, every frame of
 * zk_decode_frames[_dev], zk_decode_frame_list_dev, zk_decode_submit_dev, zk_read_ranges[_dev], zk_frame_content_sizes[_dev],
 * zk_refine_entries[_dev], zk_decode_shard and of the zk_decoder_* handles opened on the engine is decoded as libzstd decodes it after loadDictionary:
 *   - a Dictionary_ID field that is absent, 0 or the dictionary's is accepted, any other value is -32 for that frame alone;
 *   - the dictionary's content lies right before the frame's first byte (offsets are bounded by availability, as with a prefix) and
 *     the repeat-offset history starts from the dictionary's three offsets;
 *   - formatted dictionaries: the Huffman tree and the three sequence tables in force at the frame's first block are the dictionary's
 *     (Treeless literals / Repeat_Mode there are valid); with a raw-content dictionary, or none, they stay corruption (-20).
 * An explicit non-empty prefix (zk_decode_frames_prefix*, zk_decoder_decompress_with_prefix) overrides the dictionary for that call, as
 * ZSTD_DCtx_refPrefix does.  As in libzstd, EVERY frame of the call starts from the dictionary's repeat offsets and has its content below it: a frame that was made without
 * a dictionary decodes to the same bytes unless it uses a repeat offset before it has set one (libzstd's encoder emits no such frame) and the
 * dictionary's offsets are not 1 / 4 / 8, or it is damaged.  The encode
 * half is zk_cdict / zk_encode_frames_dict* below. */
typedef struct zk_dict zk_dict;
int zk_dict_create(const uint8_t *bytes, size_t len, zk_dict **out);
void zk_dict_free(zk_dict *d);
uint32_t zk_dict_id(const zk_dict *d);             /* 0 for a raw-content dictionary */
size_t zk_dict_content_offset(const zk_dict *d);   /* 0 for raw content, else the first byte of Content */
int zk_engine_set_dictionary(zk_engine *e, const zk_dict *d);

/* The decompressed sizes of frames whose seek entries the caller does not hold: header walk + sequence walks on the device, no output
 * (a frame that carries Frame_Content_Size is walked all the same and held to it: corruption_detected when its blocks make another
 * size).  What libzstd's streaming decoder needs no table for
 * (lib/src/decode.rs:243-245: ZSTD_decompressStream is handed bytes, not entries); the Level-C shim asks here before
 * it decodes.  sizes[count] (uint64), frame_status[count] (0 or -ZSTD_ErrorCode).  _dev: device pointers, c_off relative to d_comp. */
int zk_frame_content_sizes(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, uint32_t first, uint32_t count,
                           uint64_t *sizes, int32_t *frame_status);
int zk_frame_content_sizes_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, uint32_t first, uint32_t count,
                               void *d_sizes, void *d_frame_status, void *stream);

/* A seek table refined to ONE ENTRY PER FRAME, on the device.  An entry of a seek table may be any chain of Zstandard frames and skippable
 * frames (seekable_format.md:41: an archive consists of "Zstandard compressed frames and skippable frames"; the reference seeks to the
 * entry's first byte and libzstd's streaming decoder walks through whatever frames follow, lib/src/decode.rs:206-267), while every decode
 * call here takes entries of exactly one frame.  The refined table is an ordinary seek table of the same bytes -- same totals, same entry
 * boundaries, finer entries -- that every decode call, zk_read_ranges* and the handles serve; a seek under it decodes less.
 *   c_off     n_entries + 1 prefix sums of compressed sizes
 *   d_off     the same for decompressed sizes, or NULL = nobody knows them (a plain multi-frame .zst: n_entries = 1, c_off = {0, size})
 *   c_out, d_out   out_cap + 1 prefix sums each (uint64); entry_of (optional, uint32, out_cap): the input entry refined entry j came from
 *   entry_status   n_entries (int32): 0 or -(ZSTD_ErrorCode)
 * - A good entry of k frames becomes k refined entries in order, skippable frames among them with size 0; each holds exactly one frame and
 *   its decompressed size is what its blocks regenerate (obtained as zk_frame_content_sizes_dev obtains it, and held against
 *   Frame_Content_Size where the frame carries one).  A dictionary set on the engine applies as it does there.
 * - With d_off, the sizes of an entry's frames must sum to the entry's size (-20 otherwise) and d_out continues d_off: d_out[0] = d_off[0],
 *   every entry boundary of d_off is one of d_out.  With d_off == NULL, d_out starts at 0.
 * - A bad entry stays ONE refined entry: its own compressed range, its size from d_off (0 without one) and its code in entry_status, so the
 *   refined table is always a total table of the archive and decoding it reports that entry as it is reported today.  The code is that of
 *   the first frame of the entry that fails, as zk_decode_frames* and zk_frame_content_sizes* report a frame; -72 (srcSize_wrong: the entry's size does
 *   not match its frames) where fewer than 4 bytes are left behind a complete frame or the bytes left begin with neither magic; -14 where a
 *   frame decodes to more than SEEKABLE_MAX_FRAME_SIZE.
 * - *n_out (the refined entries) is always set and entry_status always written.  If *n_out > out_cap nothing else is written and -70 comes
 *   back: out_cap = 0 with NULL c_out / d_out / entry_of asks for the size.  n_entries == 0: *n_out = 0, nothing written, 0.
 * Returns 0, or the status of the first failing entry with the arrays still valid; engine errors as everywhere.  It runs on decode context 0
 * (the table above zk_decode_submit_dev); per-kernel profiling is off inside it.  The work is parallel over ENTRIES: a stream without a table
 * is one serial chain (frame i + 1 begins where frame i's last block ends) walked by one lane.
 * _dev: device pointers, c_off relative to d_comp, which must be readable ZK_COMP_PADDING bytes past comp_size.  zk_refine_entries: host
 * pointers; comp[c_off[0], c_off[n_entries]) is uploaded. */
int zk_refine_entries_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_entries,
                          void *d_c_out, void *d_d_out, void *d_entry_of, uint32_t out_cap, uint32_t *n_out, void *d_entry_status, void *stream);
int zk_refine_entries(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, const uint64_t *d_off, uint32_t n_entries,
                      uint64_t *c_out, uint64_t *d_out, uint32_t *entry_of, uint32_t out_cap, uint32_t *n_out, int32_t *entry_status);

/* Two batches in flight.  zk_decode_submit_dev enqueues exactly what zk_decode_frames_dev runs, on one of the
 * engine's two decode contexts (own HIP queues and scratch), and returns while the kernels are still running;
 * *slot_out names the context.  zk_decode_wait(slot) blocks until that batch is complete and returns its status (0,
 * or the first failing frame's code like zk_decode_frames_dev); d_frame_status is valid after the wait.  At most
 * two batches may be outstanding (a third submit returns ZK_ERR_ARGUMENT until the older one was waited for) and
 * all buffers of a batch must stay untouched until its wait.  The gain: the last stage of a batch (per-frame XXH64,
 * a serial chain that leaves the GPU mostly idle) overlaps the first stages of the next.  No reference counterpart:
 * zeekstd's Decoder is synchronous (lib/src/decode.rs:201-270); this is the batch engine's pipelining.
 *
 * Slots ALTERNATE: the first submit of an engine gets context 0, every successful submit hands the turn to the other context, nothing else
 * moves it.  A submit whose turn is a context that still holds a batch is refused -- also when the other context is free (submit A,
 * submit B, wait B, submit: refused until A was waited for); DESIGN.md 5e says why.  Waits may come in any order.  zk_decode_wait on a
 * context that holds no batch, or on a slot other than 0 and 1, is ZK_ERR_ARGUMENT.  count == 0: ZK_ERR_ARGUMENT from a submit (there
 * would be no batch to wait for; *slot_out is not written), while zk_decode_frames_dev returns 0.  A refused or failed submit leaves the
 * turn, *slot_out and the buffers as they were.
 *
 * What every other entry point does while (a) context 0, (b) context 1, (c) both hold a submitted batch:
 *   refused   ZK_ERR_ARGUMENT at once: nothing enqueued, nothing reserved or uploaded, no wait for the batch, output buffers and the
 *             engine's diagnostics as they were
 *   served    the result the call has with nothing in flight, and the batches unaffected.  (It may take longer: a call that runs on
 *             context 0's queue runs behind context 0's batch, and one that has to grow a buffer of the engine waits for the device.)
 *
 *                                                                                   (a)       (b)       (c)
 *   zk_decode_frames_dev, zk_decode_frames_prefix_dev, zk_decode_frame_list_dev     refused   served    refused    (they run on context 0,
 *   zk_frame_content_sizes_dev, zk_read_ranges_dev, zk_read_view_ranges_dev         refused   served    refused     also on the caller's stream)
 *   zk_frame_content_sizes, zk_read_ranges (host pointers)                          refused   served    refused
 *   zk_refine_entries_dev, zk_refine_entries                                        refused   served    refused    (context 0; *n_out and the arrays stay)
 *   zk_decode_frames, zk_decode_frames_prefix, zk_decode_shard (host pipeline)      refused   refused   refused    (it rotates through both contexts)
 *   zk_decoder_decompress[_with_prefix], zk_decoder_time_seeks: a read that needs   refused   refused   refused    (as ZK_ERR_IO "invalid argument", like every
 *     a submission                                                                                                  engine failure through a handle; offset, limits,
 *                                                                                                                   cache, read-ahead and counters stay)
 *     ... a read the handle's cache serves, or the part of one that it serves        served    served    served
 *     zk_decoder_set_* / _seek / _reset / the getters (the handle's own state)      served    served    served
 *   zk_engine_set_dictionary                                                        refused   refused   refused    (a batch decodes against the dictionary it was
 *                                                                                                                   submitted with)
 *   zk_gather_seekable                                                              refused   refused   refused    (a collective waits for its peers)
 *   zk_encode_frames[_prefix][_dev], zk_raw_encoder_*, zk_encoder_*                 served    served    served     (scratch of their own)
 *   zk_cdict_create / _free / _id, zk_encode_frames_dict[_dev],                     served    served    served     (the same; a zk_cdict is no decode state)
 *     zk_raw_encoder_set_dictionary, zk_encoder_set_dictionary
 *   zk_encode_frame_list[_dev]                                                      served    served    served     (the encoder's scratch, as the rows above)
 *   zk_train_dictionary[_dev]                                                       served    served    served     (the encoder's scratch and its frame-list route)
 *   zk_chunk_boundaries[_dev], zk_encode_chunked[_dev]                              served    served    served     (the encoder's scratch and its frame-list route)
 *   zk_dedup_frames[_dev], zk_encode_dedup[_dev]                                    served    served    served     (the encoder's scratch and its frame-list route)
 *   zk_dedup_against_dev, zk_encode_dedup_against_dev,                              refused   served    refused    (the candidates are decoded on context 0;
 *     zk_dedup_index_add_archive_dev                                                                                *n_fresh, the arrays and the index stay)
 *   zk_dedup_index_create / _free / _count / _add[_dev] / _export / _truncate,      served    served    served     (memory of the index's own, the encoder's scratch)
 *   zk_mark_frames_dev, zk_compact_archive_dev, zk_remap_ids_dev,                   served    served    served     (the encoder's scratch and the index's own memory, no decode
 *     zk_dedup_index_compact_dev                                                                                    context.  Compacting an archive that a submitted batch is reading
 *                                                                                                                   breaks that batch's "buffers stay untouched" rule: the caller's business)
 *     zk_frame_keys[_dev]
 *   zk_frame_digests[_dev]                                                          served    served    served     (the encoder's scratch)
 *   zk_archive_digests_dev                                                          refused   served    refused    (the frames are decoded on context 0; d_digests stays)
 *   zk_xxh64_frames[_dev]                                                           served    served    served
 *   zk_engine_set_kernel_choice / _set_fse_kernel / _set_profiling /                served    served    served     (for the calls that follow: a submitted batch keeps
 *     _set_host_threads                                                                                             the plan it was enqueued with, and is never timed)
 *   zk_engine_checksums_followed / _entropy_fused / _ranges_frames_decoded /        served    served    served     ("the last finished decode" is the batch waited for
 *     _kernel_times / _kernel_name / _last_hip_error / _device_name                                                 last, or a synchronous call after it)
 *   zk_engine_destroy                                                               served    served    served     (completes the batches first; their buffers hold the
 *                                                                                                                   results, their return codes are lost)
 * Functions that take no engine and no handle opened on one (zk_dict_*, zk_seek_table_*, zk_serializer_*, zk_host_alloc / _free,
 * zk_compress_bound, zk_compress_bound_dict, zk_compress_bound_list, zk_compress_bound_chunked, zk_shard_range, zk_set_collective_library) do not
 * depend on any of this. */
int zk_decode_submit_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off,
                         const void *d_d_off, uint32_t first, uint32_t count, void *d_dst, uint64_t dst_cap,
                         int verify, void *d_frame_status, int *slot_out);
int zk_decode_wait(zk_engine *e, int slot);

/*
 * Encode src[0, n) as ceil(n / frame_size) independent zstd frames (FrameSizePolicy::Uncompressed(frame_size),
 * lib/src/encode.rs:21-39, 528-544; n == 0 yields one empty frame like Encoder::finish, encode.rs:755-757),
 * concatenated in dst, and report the seek-table entries: c_sizes[i] / d_sizes[i] are what
 * SeekTable::log_frame receives (seek_table.rs:513-525).  checksum != 0 appends the XXH64 Content_Checksum
 * (ZSTD_c_checksumFlag, encode.rs:283-284).  level is ZSTD_c_compressionLevel (encode.rs:281-282): one strategy
 * (hash matching in a 57 280-byte window -- from level 2 on plus sampled far matches anywhere behind it in the frame, the frame
 * then declares a window over its size --, Huffman literals, FSE tables measured per frame) with five settings
 * (zk_enc_device.h: zke_fast / zke_minmatch / zke_hash_log / zke_lazy / zke_step / zke_dense_in_frame / zke_dense_log) --
 * level <= 1 (negative levels included): table matches of 6+ bytes, 2^14 table entries, greedy parse; level 2: 5+ bytes,
 * 2^15 entries, lazy parse; levels 3..5 and 0 (= libzstd's default 3, the reference CLI's default): the same plus DENSE far
 * history (round 6: every position of the frame looked up in two tables per 256 KiB, 2^17 slots -- the short far matches
 * libzstd's level 3 finds in its 2 MiB window; 8 bytes of device scratch per input byte, at most 32 GiB); level 6..8: the same with the table
 * refreshed every 1024 instead of 4096 positions; level >= 9: 2^18 slots.  Ratio on the survey's text 2.485 / 2.655 / 2.732 /
 * 2.736 / 2.743 (libzstd 1.5.7: 2.50 at level 1, 2.79 at 3, 2.88 at 9), encode 100 / 47 / 24 / 20 / 20 GiB/s HBM to HBM.
 * Replaces the ZSTD_compressStream2 loops of encode.rs:340-346, 442-464.
 * dst_cap >= zk_compress_bound(n, frame_size) always suffices; otherwise -70 (dstSize_tooSmall) may come back, and then nothing has been
 * written to dst by the device entry points (the host ones may have delivered pieces below dst_cap).
 * zk_compress_bound(n, frame_size) = n + frames * (6 + 4 + 3 * (ceil(frame_size / 1024) + 8)) + 16, frames = max(1, ceil(n / frame_size)); 0 for
 * frame_size 0.  Per frame that is the header, the checksum and a 3-byte header for more blocks than the frame can have (one block up to
 * 4 KiB, blocks of at least 4 KiB above): at least 24 bytes spare.  Blocks are stored raw unless their compressed form is smaller; only the
 * one block that carries a frame's table descriptions (frames with >= 256 sequences) can outgrow its input, by at most 149 bytes, which the
 * spare headers cover from 37 889 bytes of frame size on and the sequences' savings below (tests/test_encode_bound.py).
 */
uint64_t zk_compress_bound(uint64_t n, uint32_t frame_size);
int zk_encode_frames(zk_engine *e, const uint8_t *src, uint64_t n, uint32_t frame_size, int level, int checksum,
                     uint8_t *dst, uint64_t dst_cap, uint32_t *c_sizes, uint32_t *d_sizes, uint32_t frames_cap,
                     uint32_t *n_frames, uint64_t *written);
/* Device-resident variant: d_src / d_dst / d_c_sizes / d_d_sizes (uint32 arrays, may be NULL) live in HBM.  Once the call has
 * returned -- with 0, with -70 or with any other error -- no kernel of it reads d_src any more, on either of the engine's queues.
 * With dst_cap below the bound the total decides before anything is written: -70 leaves d_dst untouched; what d_c_sizes /
 * d_d_sizes hold after an error is unspecified. */
int zk_encode_frames_dev(zk_engine *e, const void *d_src, uint64_t n, uint32_t frame_size, int level, int checksum,
                         void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint32_t *n_frames,
                         uint64_t *written, void *stream);

/* Encode against a raw-content prefix: ZSTD_CCtx_refPrefix at the start of every frame (lib/src/encode.rs:334-338).
 * The matcher's ring reaches the last 57280 bytes of the prefix; a longer prefix is also reached through a long-distance
 * table over its last 2^27 - 1 bytes (what the reference CLI asks of libzstd for --patch-from, cli/src/compress.rs:31-37:
 * long-distance matching + a window over the old file).  Frames made this way declare a window that covers prefix + frame
 * (128 KiB .. 128 MiB) and need the same prefix to decode (zk_decode_frames_prefix, or libzstd with ZSTD_DCtx_refPrefix).
 * prefix_len == 0 is the plain call. */
int zk_encode_frames_prefix_dev(zk_engine *e, const void *d_src, uint64_t n, uint32_t frame_size, int level, int checksum,
                                const void *d_prefix, uint64_t prefix_len, void *d_dst, uint64_t dst_cap, void *d_c_sizes,
                                void *d_d_sizes, uint32_t *n_frames_out, uint64_t *written_out, void *stream);
int zk_encode_frames_prefix(zk_engine *e, const uint8_t *src, uint64_t n, uint32_t frame_size, int level, int checksum,
                            const uint8_t *prefix, uint64_t prefix_len, uint8_t *dst, uint64_t dst_cap, uint32_t *c_sizes,
                            uint32_t *d_sizes, uint32_t frames_cap, uint32_t *n_frames_out, uint64_t *written_out);

/* Encode against a zstd dictionary (what the reference reaches through EncodeOptions::with_cctx / .cctx(), encode.rs:142-155, with a context the
 * caller has loaded a dictionary into; ZSTD_CCtx_loadDictionary / ZSTD_CDict).  The frames decode with the same dictionary: here with
 * zk_engine_set_dictionary, in libzstd with ZSTD_DCtx_loadDictionary / ZSTD_decompress_usingDict.
 * zk_cdict is the compiled dictionary on the device, the counterpart of ZSTD_CDict: made once from a zk_dict (which may be freed right away), used by
 * any number of calls; several may exist on one engine, and each belongs to the engine it was made on (ZK_ERR_ARGUMENT on another).  Creation uploads
 * the content the matcher can reach (its last 2^27 - 1 bytes) and, for a formatted dictionary, builds and uploads the compression side of its four
 * tables: the Huffman code from the tree description's weights, the three FSE tables from the normalised counts, with a cost per symbol.  Free it
 * before the engine is destroyed and after the last call that uses it has returned.  There is no engine-wide "current encode dictionary":
 * zk_encode_frames* and zk_encode_frames_prefix* behave the same whatever objects exist.
 * Every frame of zk_encode_frames_dict[_dev] (cdict == NULL: ZK_ERR_ARGUMENT):
 *   - header: what zk_encode_frames_prefix* writes for the same input with the dictionary's content as the prefix -- the window covers content +
 *     frame -- plus a Dictionary_ID field of the smallest width (1 / 2 / 4 bytes) that holds the ID; no field for a raw-content dictionary (ID 0).
 *     n == 0 makes one empty frame that carries the field.
 *   - sequences and literals: exactly those of the prefix route (same records, same match kernels at every level, the same long-distance table for
 *     content beyond the matcher's ring).  The matcher emits a repeat code only after a sequence of the same block, so the dictionary's three repeat
 *     offsets never enter.
 *   - sequence tables, per frame and per table (LL / OF / ML), the cheapest by estimate of: predefined; the frame's own under the conditions of the
 *     other routes; the dictionary's -- Repeat_Mode in every block of the frame that has sequences, the first included -- which is legal only if it
 *     gives every code the frame uses a probability.  Ties keep what the other routes would take.
 *   - literals, first block of a frame only: a Treeless_Literals_Block under the dictionary's tree where that is smaller, in bytes produced, than
 *     the block's own tree, raw and RLE; legal only if every literal has a weight.  Later blocks are coded as on the other routes, and a
 *     first block that was stored as a Raw_Block or RLE_Block stays one.
 * A raw-content dictionary offers neither choice: its frames are byte-identical to zk_encode_frames_prefix* with the dictionary's bytes as the prefix.
 * dst_cap >= zk_compress_bound_dict(n, frame_size) = zk_compress_bound(n, frame_size) + 4 per frame always suffices: the largest Dictionary_ID field
 * is the one thing a frame gains.  Nothing else grows: a block is stored raw unless its compressed form is smaller, a dictionary table replaces table
 * descriptions (the one thing that lets a block outgrow its input) and adds none, and a Treeless section is taken only where it is smaller than the
 * section it replaces.  -70 and "destination untouched" are as for zk_encode_frames_dev.
 * The [content | frame] records are staged for the matcher in slices of whole frames over a bounded buffer (ZK_CHOICE_ENC_DICT_SLICE_KIB, 1 GiB by
 * default), not in one piece as the prefix route stages them. */
typedef struct zk_cdict zk_cdict;
int zk_cdict_create(zk_engine *e, const zk_dict *d, zk_cdict **out);
void zk_cdict_free(zk_cdict *c);
uint32_t zk_cdict_id(const zk_cdict *c);            /* 0 for a raw-content dictionary */
uint64_t zk_compress_bound_dict(uint64_t n, uint32_t frame_size);
int zk_encode_frames_dict_dev(zk_engine *e, const void *d_src, uint64_t n, uint32_t frame_size, int level, int checksum, const zk_cdict *cdict,
                              void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint32_t *n_frames, uint64_t *written, void *stream);
int zk_encode_frames_dict(zk_engine *e, const uint8_t *src, uint64_t n, uint32_t frame_size, int level, int checksum, const zk_cdict *cdict,
                          uint8_t *dst, uint64_t dst_cap, uint32_t *c_sizes, uint32_t *d_sizes, uint32_t frames_cap, uint32_t *n_frames,
                          uint64_t *written);

/* ---- Frames of caller-given sizes: one frame per record, log line, row or tensor, or an archive re-encoded on its own frame boundaries.
 * off[count + 1]: non-decreasing uint64 prefix sums -- the array the decode calls later take as d_off.  Frame i is src[off[i], off[i + 1]); off[0]
 * need not be 0.  A size of 0 makes the empty frame that n == 0 makes on the other routes.  count == 0 returns 0, sets *written = 0 and writes
 * nothing.  cdict == NULL and prefix_len == 0: the plain route; a non-empty prefix: the prefix route (zk_encode_frames_prefix*); cdict: the
 * dictionary route (zk_encode_frames_dict*); a cdict together with a non-empty prefix is ZK_ERR_ARGUMENT.  So is a decreasing list and a frame above
 * ZK_SEEKABLE_MAX_FRAME_SIZE; count > ZK_SEEKABLE_MAX_FRAMES is ZK_ERR_FRAME_INDEX_TOO_LARGE, decided before the list is read.  A refused call
 * writes nothing.
 * Frame i is byte for byte the frame zk_encode_frames[_prefix|_dict]_dev makes of those bytes alone -- n = size_i, frame_size = max(size_i, 1), the
 * same level, checksum flag, prefix and cdict -- at every level: window, block cut, in-frame far history, dense history, long-distance table into a
 * long prefix, dictionary tables, Treeless first block.  A list of equal sizes gives exactly the output of zk_encode_frames*.
 * c_sizes / d_sizes (may be NULL): count entries each.  *written: the sum of the c_sizes.
 * dst_cap >= zk_compress_bound_list(n, count, with_dictionary) = n + 3 * (n / 1024) + (53 + (with_dictionary ? 4 : 0)) * count, n = off[count] -
 * off[0], always suffices: it is an upper bound of the sum of the frames' own bounds.  Below it, -70 and "destination untouched" are as for
 * zk_encode_frames_dev.
 * The device entry point synchronises its stream ONCE AT THE START: the offsets (8 bytes per frame) come to the host, which checks them, and
 * with them the totals of the plan when the device makes it (ZK_CHOICE_ENC_PLAN: from 1000 frames on unless pinned).  d_off is device memory.  The host-pointer call runs through the host pipeline in groups of whole frames. */
uint64_t zk_compress_bound_list(uint64_t n, uint32_t count, int with_dictionary);
int zk_encode_frame_list_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, int checksum,
                             const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict,
                             void *d_dst, uint64_t dst_cap, void *d_c_sizes, void *d_d_sizes, uint64_t *written, void *stream);
int zk_encode_frame_list(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count, int level, int checksum,
                         const uint8_t *prefix, uint64_t prefix_len, const zk_cdict *cdict,
                         uint8_t *dst, uint64_t dst_cap, uint32_t *c_sizes, uint32_t *d_sizes, uint64_t *written);

/* ---- A dictionary trained on the device from the caller's samples (what ZDICT_trainFromBuffer does on the host; the reference has no
 * counterpart: it is handed contexts that already hold a dictionary).  off[count + 1]: the prefix sums of zk_encode_frame_list, sample i is
 * samples[off[i], off[i + 1]); off[0] need not be 0, empty samples are allowed.  p == NULL: every default.
 * The content is chosen as fastCover chooses it, without its per-segment duplicate map: every d-mer that lies inside one
 * sample is hashed to f bits and counted; the samples' N bytes are cut into E = max(1, min(content_cap / k, N / (10 k))) epochs of N / E
 * positions; epoch after epoch the segment of k bytes inside the epoch whose k - d + 1 d-mers have the largest sum of counts joins the content
 * (the lowest position on ties; nothing when the sum is 0) and the counts of its d-mers are cleared; rounds over the epochs until no further
 * segment fits or a round adds nothing.  The first segment taken lies last, nearest the data.  content_cap = min(cap - 512, 2^27 - 1): 512
 * bytes of the capacity are kept for a formatted dictionary's header whatever is written, and the matcher reaches no further back.  When no
 * segment is taken (fewer bytes than k in an epoch) the content is the last min(N, content_cap) bytes of the samples.
 * k == 0: the candidates {64, 128, 256, 512} that are <= cap / 4 are each selected (a workgroup each), the samples are encoded against every
 * candidate content with zk_encode_frame_list_dev's own route at `level` (the content as a raw-content dictionary), and the candidate with the
 * smallest total is kept, the smaller k on a tie.  Samples of at most 64 MiB in all are all encoded; above that every j-th sample is (0, j,
 * 2 j, ...), for the smallest j whose samples total at most 64 MiB (the first sample alone when no j does) -- these TRIAL SAMPLES are also what
 * the tables are measured on and what the report's two compressed totals count.  The content is always selected from all samples.
 * The result is a pure function of the arguments (integer atomics and sums only); both entry points give identical bytes.
 * What is written (RFC 8878 section 5): magic, Dictionary_ID, Huffman tree description, FSE descriptions of offsets, match lengths and literal
 * lengths, the repeat offsets 1 / 4 / 8, the content (moved up to the header: the header takes less than its 512 bytes).  The tables are the
 * statistics of the engine's own matcher: the encode stages up to and including the match stage run once more over the samples with the
 * chosen content as the prefix, and every literal byte and every sequence's three codes are counted (zk_k_train_stats).  The matcher emits a
 * repeat code only after a sequence of the same block, so the dictionary's repeat offsets never enter: they are 1 / 4 / 8.  Every literal value
 * and every code (LL 0..35, ML 0..52, OF 0..30) gets a count of at least 1, so that zk_encode_frames_dict*'s rules always allow the Treeless
 * first block and Repeat_Mode; Huffman code lengths are at most 11 and their 255 weights are written FSE-compressed; the FSE tables are
 * normalised at accuracy logs 9 / 9 / 8 (LL / ML / OF).  dict_id == 0: 32768 + XXH64(content) mod (2^31 - 65536), inside libzstd's private range.
 * The result is a dictionary zk_dict_create accepts and libzstd loads.  flags: ZK_TRAIN_RAW_CONTENT writes the content alone, a raw-content
 * dictionary (ID 0): exactly the formatted result's content.
 * ZK_ERR_ARGUMENT, and nothing written, for: count == 0; cap < 1024; NULL dict_out / written / off; d other than 0 / 6 / 8; f other than 0 or
 * 10 ... 24; k other than 0 or 16 ... 4096, or k > cap / 4; an unknown flag; a decreasing list; 2^32 or more sample bytes; fewer than
 * 8 samples of at least d bytes; a sample above ZK_SEEKABLE_MAX_FRAME_SIZE.  count > ZK_SEEKABLE_MAX_FRAMES: ZK_ERR_FRAME_INDEX_TOO_LARGE, decided
 * before the list is read.
 * report (optional): the segment length kept, the segments taken, the content's and the header's bytes (0 for raw content), and the samples'
 * bytes: as given (all of them) / the trial samples encoded at `level` against the result's CONTENT as a raw-content dictionary / the trial
 * samples encoded without a dictionary.
 * The device entry point synchronises its stream; dict_out, written and report are host memory in both. */
#define ZK_TRAIN_RAW_CONTENT 1u
typedef struct zk_train_params {
    uint32_t k;        /* segment length, 16 ... 4096; 0 = try the built-in set {64, 128, 256, 512} (those <= cap / 4) and keep the best */
    uint32_t d;        /* d-mer length, 6 or 8; 0 = 8 */
    uint32_t f;        /* log2 of the frequency table, 10 ... 24; 0 = 20 */
    int level;         /* encoder level the statistics, the choice between candidates and the report are taken at; 0 = 1 */
    uint32_t dict_id;  /* 0 = derived from the content's XXH64 into [32768, 2^31 - 32768) */
    uint32_t flags;    /* ZK_TRAIN_RAW_CONTENT: write the content alone (a raw-content dictionary) */
} zk_train_params;
typedef struct zk_train_report {
    uint32_t k_chosen, segments, content_bytes, header_bytes;
    uint64_t sample_bytes, compressed_with, compressed_without;
} zk_train_report;
int zk_train_dictionary_dev(zk_engine *e, const void *d_samples, const void *d_off, uint32_t count, const zk_train_params *p,
                            uint8_t *dict_out, size_t cap, size_t *written, zk_train_report *report, void *stream);
int zk_train_dictionary(zk_engine *e, const uint8_t *samples, const uint64_t *off, uint32_t count, const zk_train_params *p,
                        uint8_t *dict_out, size_t cap, size_t *written, zk_train_report *report);

/* ---- Content-defined frame boundaries: where the frames end when the caller has no records to point at and a fixed grid will not do (one
 * inserted byte shifts every later frame of a grid; cuts that follow the content fall back onto the old ones within a frame or two, and every
 * untouched frame compresses to the same bytes as before -- what zchunk, casync and `zstd --rsyncable` cut by content for).  The reference has
 * no counterpart.  off[count + 1] is the array zk_encode_frame_list[_dev] and later the decode calls take.
 * THE RULE, a pure function of (src[0, n), min_size, avg_size, max_size):
 *   - gear table G[b], b = 0..255, in 32-bit wrap-around arithmetic: x = (b + 1) * 0x9E3779B1; x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13;
 *     x *= 0xC2B2AE35; x ^= x >> 16; G[b] = x
 *   - hash of position p: h(p) = sum over j = 0..31 of G[src[p - j]] << j (mod 2^32), terms with p - j < 0 absent.  It is the gear recurrence
 *     h = (h << 1) + G[byte], which forgets a byte after 32 steps: h(p) depends on src[p - 31 .. p] only
 *   - candidate: with bits = log2(avg_size), p is a candidate iff h(p) >> (32 - bits) == 0 (the top bits: the low bits of a gear hash see only the
 *     last few bytes).  A candidate at p offers the cut offset q = p + 1
 *   - selection: off[0] = 0.  From a cut c < n, with lo = c + min_size and hi = min(c + max_size, n), the next cut is the smallest candidate offset
 *     q with lo <= q <= hi, or hi if there is none.  Selection ends with the cut at n.  The last frame may be shorter than min_size, no other is;
 *     no frame is longer than max_size.  n == 0: count = 1 and off = {0, 0}, the empty frame the other routes make.
 * zk_chunk_params (p == NULL: every default): avg_size a power of two in [2^8, 2^24], 0 = 2^21 (zeekstd's default frame size); min_size in
 * [64, avg_size], 0 = avg_size / 4; max_size in [min_size, ZK_SEEKABLE_MAX_FRAME_SIZE], 0 = min(4 * avg_size, 2^30); flags must be 0.  Anything
 * else is ZK_ERR_ARGUMENT, decided before any work.
 * What follows from the rule:
 *   - a frame's end depends on its own bytes: min_size >= 64, so a candidate's 32-byte window lies inside the current frame, past its 32nd byte.
 *     Where a frame ends depends only on where it starts and on its own bytes: two chains of cuts that share one cut share all later ones
 *   - on incompressible data the mean frame is about min_size + avg_size when max_size is far away (316, 1306 and 5243 bytes measured on random
 *     bytes for min / avg = 64 / 256, 256 / 1024 and 1024 / 4096)
 *   - min_size == max_size == S gives exactly the cuts of frame_size = S, and therefore the bytes of zk_encode_frames*
 * zk_chunk_boundaries_dev: d_src (any alignment) and d_off_out (uint64, off_cap + 1 entries) are device memory.  *count is always set; if count >
 * off_cap nothing else is written and -70 comes back, so off_cap = 0 with a NULL array asks for the size.  (With off_cap >= n / min_size + 1,
 * which no chain exceeds, the array is written in the one pass that finds the cuts; with less room the engine counts first and runs once more
 * when the count fits.)  count > ZK_SEEKABLE_MAX_FRAMES is ZK_ERR_FRAME_INDEX_TOO_LARGE.  The call synchronises its stream.
 * zk_chunk_boundaries (host pointers) uploads the source slice by slice; only the offsets come back.
 * zk_encode_chunked[_dev] is zk_chunk_boundaries[_dev] followed by zk_encode_frame_list[_dev] on the plain, prefix or dictionary route: the frames
 * are byte for byte what that call makes of the offsets.  The offsets array holds off_cap + 1 entries, c_sizes / d_sizes (may be NULL) off_cap
 * each; *n_frames = count.  An off_cap that is too small is -70 before anything is encoded, with the destination untouched.
 * dst_cap >= zk_compress_bound_chunked(n, p, with_dictionary) = zk_compress_bound_list(n, n / min_size + 1, with_dictionary) always suffices (0
 * for parameters that would be refused); below it, -70 and "destination untouched" are as for zk_encode_frame_list_dev.
 * The input is marked and selected in slices (ZK_CHOICE_CDC_SLICE_KIB), the chain's current cut carried from slice to slice and the 31-byte
 * window read across the seam: the offsets do not depend on the slice, and the scratch is bounded by it, not by n. */
typedef struct zk_chunk_params { uint32_t min_size, avg_size, max_size, flags; } zk_chunk_params;
int zk_chunk_boundaries_dev(zk_engine *e, const void *d_src, uint64_t n, const zk_chunk_params *p, void *d_off_out, uint32_t off_cap,
                            uint32_t *count, void *stream);
int zk_chunk_boundaries(zk_engine *e, const uint8_t *src, uint64_t n, const zk_chunk_params *p, uint64_t *off_out, uint32_t off_cap,
                        uint32_t *count);
uint64_t zk_compress_bound_chunked(uint64_t n, const zk_chunk_params *p, int with_dictionary);
int zk_encode_chunked_dev(zk_engine *e, const void *d_src, uint64_t n, const zk_chunk_params *p, int level, int checksum,
                          const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict, void *d_dst, uint64_t dst_cap,
                          void *d_off_out, uint32_t off_cap, void *d_c_sizes, void *d_d_sizes, uint32_t *n_frames,
                          uint64_t *written, void *stream);
int zk_encode_chunked(zk_engine *e, const uint8_t *src, uint64_t n, const zk_chunk_params *p, int level, int checksum,
                      const uint8_t *prefix, uint64_t prefix_len, const zk_cdict *cdict, uint8_t *dst, uint64_t dst_cap,
                      uint64_t *off_out, uint32_t off_cap, uint32_t *c_sizes, uint32_t *d_sizes, uint32_t *n_frames, uint64_t *written);

/* ---- Duplicate frames found on the device, and each distinct frame encoded once: what content-defined cuts are for (a VM image with repeated
 * blocks, backups of several versions of a tree, logs with repeated records).  The reference has no counterpart.  off[count + 1] is the array
 * zk_encode_frame_list[_dev] takes: non-decreasing, off[0] need not be 0, frame i is src[off[i], off[i + 1]).
 * THE RULE, a pure function of the frames' bytes:
 *   - ref[i] is the smallest j <= i whose frame has the same length and the same bytes as frame i.  ref[i] == i exactly for the first frame of
 *     each distinct content; all empty frames are equal to each other
 *   - uniq[0 .. n_unique) is the ascending list of the i with ref[i] == i
 *   - ids[i] is the position of ref[i] in uniq: the array zk_decode_frame_list_dev takes as d_ids when the archive holds the uniq frames in
 *     that order
 * ref, ids (count entries) and uniq (n_unique entries; size it for count) are uint32, and each may be NULL; *n_unique is always set.
 * The result is EXACT: it does not depend on the quality of any hash.  Frames are grouped by a 64-bit key (a hash of the bytes made for this purpose, and the length)
 * and a frame is merged into a group's first frame only after all its bytes have been compared with that frame's; a frame that differs is
 * grouped again among the frames still open, round after round, until every frame is settled.  ZK_CHOICE_DEDUP_KEY_BITS
 * shortens the key so that tests reach those rounds; the outputs do not depend on it.
 * ZK_ERR_ARGUMENT for a decreasing list or a frame above ZK_SEEKABLE_MAX_FRAME_SIZE; count > ZK_SEEKABLE_MAX_FRAMES is
 * ZK_ERR_FRAME_INDEX_TOO_LARGE, decided before the list is read; count == 0 returns 0 with *n_unique = 0.  A refused call writes nothing to
 * the arrays (*n_unique = 0).
 * zk_dedup_frames_dev: d_src (any alignment, no padding needed: no load leaves [off[0], off[count])), d_off and the three arrays are device
 * memory, n_unique is host memory.  The call SYNCHRONISES ITS STREAM: once at the start, when the offsets come to the host to be checked;
 * once or twice per round (one round unless two different frames share a key) for the count of frames still open; and at the end.
 * zk_dedup_frames (host pointers) uploads the source whole into engine scratch, off[count] - off[0] bytes; only the three arrays come back.
 * zk_encode_dedup[_dev] is zk_dedup_frames[_dev] followed by zk_encode_frame_list[_dev] over the uniq frames only, on the plain, prefix or
 * dictionary route: frame k of the output is byte for byte the frame that call makes of source frame uniq[k] alone, with the same level,
 * checksum flag, prefix and cdict.  c_sizes / d_sizes (may be NULL) receive n_unique entries; size them for count.  *written is the sum of
 * the c_sizes.  The unique frames are gathered back to back into engine scratch in slices of whole frames (ZK_CHOICE_DEDUP_SLICE_KIB) and
 * encoded slice after slice into consecutive destinations; a list without duplicates is encoded where it lies.  The bytes do not depend on
 * the slice.  dst_cap >= zk_compress_bound_list(n, count, with_dictionary), the bound of the list without any duplicate, always suffices;
 * below it, -70 and "destination untouched" are as for zk_encode_frame_list_dev (with more than one slice the frames are then encoded
 * twice, the first time into scratch).  The host-pointer call uploads the source whole and stages the prefix as zk_encode_frame_list does.
 * READING BACK needs nothing new.  With c_off / d_off the prefix sums of the n_unique c_sizes / d_sizes,
 *     zk_decode_frame_list_dev(e, d_comp, written, d_c_off, d_d_off, d_ids = ids, d_out_off = off - off[0], count, d_dst, off[count] - off[0], ...)
 * reproduces src[off[0], off[count]): ids may repeat and come in any order.  zk_read_view_ranges_dev(..., d_view_ids = ids, d_view_off = off,
 * view_count = count, ...) reads any byte ranges of src[off[0], off[count]) instead, and decodes a frame that ids names several times once.  Where ids is kept is the caller's business (a skippable frame
 * is the obvious place); nothing is remembered from call to call -- that is what zk_dedup_index and zk_encode_dedup_against_dev, below, are for. */
int zk_dedup_frames_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count,
                        void *d_ref, void *d_ids, void *d_uniq, uint32_t *n_unique, void *stream);
int zk_dedup_frames(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count,
                    uint32_t *ref, uint32_t *ids, uint32_t *uniq, uint32_t *n_unique);
int zk_encode_dedup_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, int checksum,
                        const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict,
                        void *d_dst, uint64_t dst_cap, void *d_ids, void *d_uniq,
                        void *d_c_sizes, void *d_d_sizes, uint32_t *n_unique, uint64_t *written, void *stream);
int zk_encode_dedup(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count, int level, int checksum,
                    const uint8_t *prefix, uint64_t prefix_len, const zk_cdict *cdict,
                    uint8_t *dst, uint64_t dst_cap, uint32_t *ids, uint32_t *uniq,
                    uint32_t *c_sizes, uint32_t *d_sizes, uint32_t *n_unique, uint64_t *written);

/* ---- A frame list deduplicated against an archive that already exists: tonight's backup against last night's, version N + 1 of an image
 * against version N, a chunk store that grows.  The reference has no counterpart.  An ARCHIVE is what zk_decode_frame_list_dev reads: d_comp,
 * d_c_off, d_d_off, n_frames, all in device memory.  A zk_dedup_index knows its first m frames (m = zk_dedup_index_count).
 * THE RULE, a pure function of the decoded archive frames 0 .. m-1 and the list's bytes (off[count + 1] as everywhere else):
 *   - ids[i] is the smallest archive frame s < m whose decoded bytes and length equal frame i's, where one exists
 *   - otherwise let j be the smallest list index <= i with frame i's bytes: j is FRESH, and ids[i] = m + (the position of j in fresh)
 *   - fresh[0 .. n_fresh) is the ascending list of such j
 *   - all empty frames are equal, to each other and to an empty archive frame
 *   - with m == 0, ids and fresh are exactly ids and uniq of zk_dedup_frames
 *   - after the fresh frames are appended to the archive in that order, zk_decode_frame_list_dev over the grown archive with d_ids = ids and
 *     d_out_off = off - off[0] reproduces src[off[0], off[count])
 * ids (count entries) and fresh (n_fresh entries; size it for count) are uint32 and may be NULL; *n_fresh is always set.
 * The result is EXACT: a frame is mapped to an archive frame only after every one of its bytes has been compared with that frame's DECODED
 * bytes.  The key decides the time, never the result.
 * THE FRAME KEY, a stored format from here on (an exported index holds it): the frame is read as little-endian 8-byte words counted from its
 * own first byte, zero-padded to a multiple of 16 bytes; word w of value v gives the term
 *     x = v + (w + 1) * 0x9E3779B97F4A7C15;  x ^= x >> 33;  x *= 0xFF51AFD7ED558CCD;  x ^= x >> 33;  x *= 0xC4CEB9FE1A85EC53;  x ^= x >> 33
 * (all mod 2^64), and the key is (the sum of the terms' low 32 bits mod 2^32) | (the sum of their high 32 bits mod 2^32) << 32.  The empty
 * frame's key is 0.  The length is not part of it: the index keeps it beside the key.  zk_frame_keys[_dev] writes count keys (uint64; the
 * device array 8-byte aligned); list errors as for zk_dedup_frames.
 * THE INDEX lives on the device: the full 64-bit keys and the lengths of its m frames, and an open-addressing table of 32-bit archive ids that
 * persists between calls.  Every frame has a slot of its own (equal keys are not merged: the archive may hold duplicates), taken by
 * compare-and-swap, linear probing from the home of its key cut to ZK_CHOICE_DEDUP_KEY_BITS as in force when the index was created.  The table
 * keeps at least twice as many slots as frames and is rebuilt at twice the size from the keys when an add would cross that.
 *   zk_dedup_index_create       an empty index (NULL when the device gives no memory); zk_dedup_index_free(NULL) is allowed
 *   zk_dedup_index_add[_dev]    frames m .. m + count - 1 from their keys (uint64) and decoded sizes (uint32).  An index made by add from
 *                               exported arrays behaves exactly like the one they were exported from
 *   zk_dedup_index_add_archive_dev   decodes archive frames m .. n_frames - 1 (checksums verified, against the engine's dictionary if one is
 *                               set) in passes of ZK_CHOICE_DEDUP_PASS_KIB, keys them and adds them; a frame that fails returns its -(code) and
 *                               leaves the index as it was.  n_frames < m is ZK_ERR_ARGUMENT
 *   zk_dedup_index_export       keys and sizes of frames [first, first + count) to host arrays (either may be NULL)
 *   zk_dedup_index_truncate     forgets frames >= count (an append the caller could not keep); the table is rebuilt
 * m + count above ZK_SEEKABLE_MAX_FRAMES is ZK_ERR_FRAME_INDEX_TOO_LARGE.  Every call that changes the index synchronises its stream.  An index
 * belongs to the engine it was made on and must be freed before it.
 * zk_dedup_against_dev: the in-call map of zk_dedup_frames_dev first; then, in rounds, every unique frame still open looks up the smallest
 * index entry of its key and length above the one it tried last; the round's candidates are decoded on context 0 -- the route of
 * zk_decode_frame_list_dev, checksums verified, against the engine's dictionary if one is set -- into engine scratch in passes of at most
 * ZK_CHOICE_DEDUP_PASS_KIB (one whole frame at least), and each is compared with its source frame byte for byte.  Equal settles the frame on
 * that archive frame; different opens it again.  Candidates ascend, so the first match is the smallest s.  One round unless an
 * archive frame shares key and length with a different frame.  The call SYNCHRONISES ITS STREAM as zk_dedup_frames_dev does, and then once per
 * round for the candidates, once per pass, once per round for the verdicts, and at the end.
 *   - n_frames < m is ZK_ERR_ARGUMENT; frames at or beyond m are not looked at.  An index entry whose length is not the archive's is never a match
 *   - a candidate that fails to decode or verify returns its -(code): the arrays are not written, *n_fresh = 0, the index is unchanged
 *   - list errors, count == 0 and NULL outputs as for zk_dedup_frames_dev; a refused call writes nothing to the arrays (*n_fresh = 0)
 * zk_encode_dedup_against_dev runs that map and then encodes the fresh frames exactly as zk_encode_dedup_dev encodes its uniq frames (gathered
 * in slices of ZK_CHOICE_DEDUP_SLICE_KIB, through zk_encode_frame_list_dev, the same bound, -70 with the destination and the arrays
 * untouched): output frame k is byte for byte what the list call makes of source frame fresh[k] alone.  c_sizes / d_sizes (may be NULL) receive
 * n_fresh entries; size them for count.  On success, and only then, the fresh frames' keys and lengths are added to the index -- they are known
 * from the map, nothing is decoded -- so that m grows by n_fresh.  The caller appends the payload to the archive and extends c_off / d_off
 * from c_sizes / d_sizes (or calls zk_dedup_index_truncate when it cannot).  There is no prefix route: the verifying decode takes no prefix, so
 * the call has no prefix parameters.  cdict is allowed; the verification of later calls then needs the matching dictionary set on the engine
 * (zk_engine_set_dictionary), which is the caller's business.
 * Not here: Level-B handles, host-pointer forms of the two `against` calls, an on-disk container for ids or for an exported index. */
typedef struct zk_dedup_index zk_dedup_index;
zk_dedup_index *zk_dedup_index_create(zk_engine *e);
void zk_dedup_index_free(zk_dedup_index *x);
uint32_t zk_dedup_index_count(const zk_dedup_index *x);
int zk_dedup_index_add(zk_dedup_index *x, const uint64_t *keys, const uint32_t *d_sizes, uint32_t count);
int zk_dedup_index_add_dev(zk_dedup_index *x, const void *d_keys, const void *d_d_sizes, uint32_t count, void *stream);
int zk_dedup_index_add_archive_dev(zk_dedup_index *x, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                                   uint32_t n_frames, void *stream);
int zk_dedup_index_export(const zk_dedup_index *x, uint32_t first, uint32_t count, uint64_t *keys_out, uint32_t *d_sizes_out);
int zk_dedup_index_truncate(zk_dedup_index *x, uint32_t count);
int zk_frame_keys_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, void *d_keys, void *stream);
int zk_frame_keys(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count, uint64_t *keys);
int zk_dedup_against_dev(zk_engine *e, const zk_dedup_index *x,
                         const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                         const void *d_src, const void *d_off, uint32_t count,
                         void *d_ids, void *d_fresh, uint32_t *n_fresh, void *stream);
int zk_encode_dedup_against_dev(zk_engine *e, zk_dedup_index *x,
                                const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                                const void *d_src, const void *d_off, uint32_t count, int level, int checksum, const zk_cdict *cdict,
                                void *d_dst, uint64_t dst_cap, void *d_ids, void *d_fresh, void *d_c_sizes, void *d_d_sizes,
                                uint32_t *n_fresh, uint64_t *written, void *stream);

/* ---- Frames removed from a device-resident archive: a backup whose oldest snapshot is dropped, a chunk store with retention.  The reference
 * has no counterpart.  The ARCHIVE is what zk_decode_frame_list_dev reads: d_comp, comp_size, d_c_off[n_frames + 1], d_d_off[n_frames + 1]
 * (uint64, non-decreasing).  live[n_frames] is uint8, nonzero = keep.  THE RULE, a pure function of these:
 *   - kept[0 .. n_kept) is the ascending list of s with live[s] != 0
 *   - remap[s] is the position of s in kept, or ZK_FRAME_REMOVED for a removed frame
 *   - c_off_out[0] = c_off[0], d_off_out[0] = d_off[0]; c_off_out[k + 1] - c_off_out[k] is the compressed size of frame kept[k], and the same
 *     holds for d_off_out
 *   - dst[c_off_out[k], c_off_out[k + 1]) is, byte for byte, comp[c_off[kept[k]], c_off[kept[k] + 1])
 *   - *written = c_off_out[n_kept]: one past the last byte of the compacted archive, counted from d_dst, like comp_size
 * Kept frames keep their order, so the "smallest archive frame" of zk_dedup_against_dev over the compacted archive is what the rule gives over
 * the kept frames.  No frame is decoded: the call moves bytes and never looks inside them.  Entries of compressed size 0 are legal, kept or
 * removed.
 * zk_mark_frames_dev sets live[ids[i]] = 1 for count uint32 ids.  It only sets: the caller zeroes live once and marks every snapshot it keeps,
 * call after call.  An id at or above n_frames returns ZK_ERR_ARGUMENT and leaves live as it was (the ids are checked first, then written;
 * one wait between).  count == 0 returns 0.
 * zk_compact_archive_dev writes remap (uint32, n_frames entries), c_off_out and d_off_out (uint64, n_kept + 1 entries; size them for n_frames
 * + 1); each may be NULL.  *n_kept and *written are always set.  d_dst may be d_comp itself: IN PLACE, the form a store uses; otherwise
 * d_dst[0, dst_cap) must not overlap d_comp[0, comp_size + ZK_COMP_PADDING): any other overlap is ZK_ERR_ARGUMENT.  The offsets may be updated
 * in place too (d_c_off_out == d_c_off, d_d_off_out == d_d_off).  Nothing is stored outside dst[c_off[0], written); in place nothing before
 * the first removed frame is stored at all, and nothing at or beyond written.  Nothing is loaded outside comp[c_off[0], c_off[n_frames]).
 *   - dst_cap < written (out of place; in place dst_cap is not looked at) returns -70 with the destination and the arrays untouched,
 *     *n_kept = 0 and *written = the size that is needed
 *   - a decreasing offset list, c_off[n_frames] > comp_size, NULL d_live or d_dst return ZK_ERR_ARGUMENT
 *   - n_frames > ZK_SEEKABLE_MAX_FRAMES returns ZK_ERR_FRAME_INDEX_TOO_LARGE before anything is read
 *   - n_frames == 0 returns 0 with *n_kept = 0 and *written = c_off[0] if d_c_off is given, else 0
 *   - a refused call writes nothing
 * It SYNCHRONISES ITS STREAM once for the checks and the totals, and at the end.  In place the bytes move in steps of
 * ZK_CHOICE_COMPACT_SLICE_KIB destination bytes from the first removed frame on; a step that cannot read and write side by side goes through
 * engine scratch of one step's size.
 * zk_remap_ids_dev: ids_out[i] = remap[ids[i]] (uint32; d_ids_out may be d_ids).  An id at or above n_frames, or one of a removed frame,
 * returns ZK_ERR_ARGUMENT and leaves ids_out untouched.
 * zk_dedup_index_compact_dev: the index after the same removal.  n_frames must equal zk_dedup_index_count(x) and remap must be what
 * zk_compact_archive_dev writes (kept frames numbered 0, 1, ... in order), else ZK_ERR_ARGUMENT.  The keys and lengths of the kept frames move
 * to their new places on the device and the table is rebuilt from them as zk_dedup_index_truncate rebuilds it; m becomes n_kept.  The index
 * then behaves exactly like one built by zk_dedup_index_add from the kept frames' exported keys and sizes.  Nothing is decoded.  On any
 * refusal the index is unchanged.
 * Not here: merging duplicate frames an archive already holds, host-pointer forms, Level-B handles, re-encoding kept frames, compaction
 * across several archives. */
#define ZK_FRAME_REMOVED 0xFFFFFFFFu
int zk_mark_frames_dev(zk_engine *e, const void *d_ids, uint32_t count, uint32_t n_frames, void *d_live, void *stream);
int zk_compact_archive_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                           const void *d_live, void *d_dst, uint64_t dst_cap, void *d_c_off_out, void *d_d_off_out, void *d_remap,
                           uint32_t *n_kept, uint64_t *written, void *stream);
int zk_remap_ids_dev(zk_engine *e, const void *d_remap, uint32_t n_frames, const void *d_ids, uint32_t count, void *d_ids_out, void *stream);
int zk_dedup_index_compact_dev(zk_dedup_index *x, const void *d_remap, uint32_t n_frames, void *stream);

/* ---- Content digests of frames: what names a chunk between two parties -- a client that asks a remote store which chunks it lacks, a manifest, a
 * restore that proves a chunk is the one that was stored, tools that address chunks by hash.  The frame key above is fast and order-free but not
 * collision-resistant; it is trusted only because every match is followed by a byte-for-byte compare.  The reference has no counterpart.
 * Frame i is src[off[i], off[i + 1]) (off[count + 1], non-decreasing).  digests receives count * ZK_DIGEST_BYTES bytes, digest i at byte
 * 32 i, in the order hexdigest() prints them; the device array must be 4-byte aligned.  THE DIGEST, a stored format from here on:
 *   ZK_DIGEST_SHA256        FIPS 180-4 SHA-256 of the frame's bytes.  The empty frame gives e3b0c442 98fc1c14 9afbf4c8 996fb924 27ae41e4 649b934c
 *                           a495991b 7852b855.
 *   ZK_DIGEST_BLAKE2S_TREE  BLAKE2s (RFC 7693) with the tree parameters of the BLAKE2 specification: digest length 32, no key, no salt, no
 *                           personalisation, fanout 0 (unlimited), maximal depth 2, leaf length ZK_DIGEST_LEAF = 4096, inner length 32.  The
 *                           frame is cut into n = max(1, ceil(len / 4096)) leaves; leaf k is hashed with node offset k and node depth 0, the
 *                           last leaf carries the last-node flag, an empty frame has one empty leaf; the digest is the root: BLAKE2s over the
 *                           n concatenated 32-byte leaf digests with node offset 0, node depth 1 and the last-node flag.  In Python:
 *                               def tree(m, L=4096):
 *                                   n = max(1, -(-len(m) // L))
 *                                   inner = b"".join(hashlib.blake2s(m[k*L:(k+1)*L], digest_size=32, fanout=0, depth=2, leaf_size=L, node_offset=k,
 *                                                    node_depth=0, inner_size=32, last_node=(k == n-1)).digest() for k in range(n))
 *                                   return hashlib.blake2s(inner, digest_size=32, fanout=0, depth=2, leaf_size=L, node_offset=0, node_depth=1,
 *                                                          inner_size=32, last_node=True).digest()
 *                           The empty frame gives f516be67ca647aaa6b225e5844e35af8e4a7073cd445f0a41b3ba2a5d0584aa4, the 4097 bytes i & 255 give
 *                           66d4770bed3555ad5838c35af7753df322a55172a6309c3a949d06919122f201.
 * SHA-256 is the interoperable one (borg, restic, casync and OCI address chunks by it): a frame is ONE chain in one lane, fast for lists of
 * short chunks and bound by that chain for long frames (2 MiB are 32 768 compressions one after the other).  The tree runs a lane per leaf, at
 * device speed for any frame length; only the root of a very long frame is a chain again (a 1 GiB frame has 262 144 leaves, its root hashes
 * 8 MiB in one lane).  Measured on 1 GiB of text cut at avg_size 4 KiB / 64 KiB / 2 MiB (tools/digest_probe.py, profiles/digest_probe.txt): the
 * tree 1.58 / 0.89 / 4.06 ms -- at 2 MiB 3.6 ms of it the roots, the longest frame's 2 048 leaf digests in one lane --, SHA-256 3.92 / 20.8 /
 * 729 ms: the 411 chains of the 2 MiB list run at 1.5 GB/s, below one host core.
 * zk_frame_digests[_dev]:
 *   - an unknown algo is ZK_ERR_ARGUMENT, returned before anything is read
 *   - list errors, count == 0, count > ZK_SEEKABLE_MAX_FRAMES and NULL pointers as for zk_frame_keys[_dev]; a misaligned d_digests is
 *     ZK_ERR_ARGUMENT; a refused call writes nothing
 *   - nothing is stored outside d_digests[0, 32 count), nothing is loaded outside src[off[0], off[count])
 *   - the device form SYNCHRONISES ITS STREAM once for the offsets and once at the end, as zk_frame_keys_dev does
 * zk_archive_digests_dev: the digests of the DECODED content of archive frames [first, first + count) (d_comp, comp_size, d_c_off, d_d_off: what
 * zk_decode_frame_list_dev reads).  The frames are decoded on context 0 exactly as zk_dedup_index_add_archive_dev decodes them -- checksums
 * verified, against the engine's dictionary if one is set, in passes of at most ZK_CHOICE_DEDUP_PASS_KIB and at least one whole frame -- into
 * engine scratch, and each pass is digested there by the same kernels behind the decode.  An entry of decoded size 0 gets the empty digest.  A
 * frame that fails returns its -(code); the contents of d_digests[0, 32 count) are unspecified then, and nothing outside that range is written.
 * The call does not know how many entries the tables hold: first + count above ZK_SEEKABLE_MAX_FRAMES, a decreasing d_d_off and frames that
 * reach beyond comp_size are ZK_ERR_ARGUMENT.  It is refused while context 0 holds a submitted batch (the table above zk_decode_submit_dev).
 * Not here: a digest-keyed index or a missing(digests) lookup, digests stored in a skippable frame or any on-disk container, keyed or salted
 * hashing, SHA-512, BLAKE3, Level-B handles, a host-pointer form of the archive call. */
#define ZK_DIGEST_SHA256        1
#define ZK_DIGEST_BLAKE2S_TREE  2
#define ZK_DIGEST_BYTES         32
#define ZK_DIGEST_LEAF          4096
int zk_frame_digests_dev(zk_engine *e, int algo, const void *d_src, const void *d_off, uint32_t count, void *d_digests, void *stream);
int zk_frame_digests(zk_engine *e, int algo, const uint8_t *src, const uint64_t *off, uint32_t count, uint8_t *digests);
int zk_archive_digests_dev(zk_engine *e, int algo, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                           uint32_t first, uint32_t count, void *d_digests, void *stream);

/* Host memory the host-pointer entry points above move by DMA directly (pinned; hipHostMalloc underneath).  Buffers from
 * anywhere else work too: they are staged through the engine's own pinned rings by worker threads, chunk by chunk, beside
 * the kernels (the reference streams through 128 KiB buffers at no copy cost, lib/src/encode.rs:779-787,
 * decode.rs:222-225; on a GPU the PCIe legs are part of the path and are overlapped instead). */
void *zk_host_alloc(size_t bytes);
void zk_host_free(void *p);
/* worker threads of the host pipeline (parallel staging copies); 0 = default (hardware threads / 8, clamped to 2..16) */
int zk_engine_set_host_threads(zk_engine *e, int n);

/* Sharded encode, the one exchange step (BASELINE.json configs[4]): frames are independent, so rank r of `world`
 * encodes its contiguous frame range on its own GPU (zk_encode_frames_dev) and this call concatenates the ranks' compressed
 * streams in rank order into d_out on `root` and appends the seek table -- an archive zeekstd's Decoder reads
 * (seek_table.rs:379-436).  nccl_comm: the caller's RCCL communicator (ncclComm_t, one per rank); RCCL is resolved at run time.
 * Steps: all-gather of (bytes, frames), all-gather of the padded (c_size, d_size) entries, grouped ncclSend / ncclRecv of the
 * payloads straight into d_out + offset_r over xGMI, table serialised by the root.  d_payload / d_out: device memory;
 * c_sizes / d_sizes: this rank's n_frames entries on the host (what zk_encode_frames_dev reported).  On the root *out_bytes
 * receives stream + table bytes and *table_out (optional) the gathered SeekTable; the other ranks pass d_out = NULL. */
typedef struct zk_seek_table zk_seek_table;
/* The shared library that provides ncclAllGather / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd for zk_gather_seekable; NULL or ""
 * = RCCL (symbols already in the process, else librccl.so.1).  Process-wide; call it before the first gather.  (The library reads no
 * environment variable.)  The tests name a shared-memory transport between processes that share one GPU here. */
int zk_set_collective_library(const char *path);
int zk_gather_seekable(zk_engine *e, void *nccl_comm, int rank, int world, int root, const void *d_payload, uint64_t payload_bytes,
                       const uint32_t *c_sizes, const uint32_t *d_sizes, uint32_t n_frames, int format, void *d_out, uint64_t out_cap,
                       uint64_t *out_bytes, zk_seek_table **table_out, void *stream);

/* Sharded decode (the decode side): rank r of `world` owns the contiguous frame range zk_shard_range gives it,
 * reads / receives the compressed bytes [c_off[first], c_off[first + count]) of the archive -- nothing else -- and decodes
 * them into its own buffer; the output stays sharded, there is no collective.  zk_decode_shard does the arithmetic:
 * comp_shard points at exactly those bytes (frame `first` at comp_shard[0]), table is the archive's seek table
 * (zk_seek_table_from_bytes / _from_reader on the tail every rank can read: 8 n + 17 bytes), dst receives the frames'
 * decompressed bytes, *first / *count / *written report the range and its size.  Returns 0 or -(code) of the first
 * failing frame, like zk_decode_frames. */
int zk_shard_range(uint32_t n_frames, int rank, int world, uint32_t *first, uint32_t *count);
int zk_decode_shard(zk_engine *e, const uint8_t *comp_shard, uint64_t shard_bytes, const zk_seek_table *table, int rank, int world,
                    uint8_t *dst, uint64_t dst_cap, int verify, uint32_t *first, uint32_t *count, uint64_t *written);

/* XXH64(seed 0) of count byte ranges data[off[i], off[i+1]) -> out[i].  (The checksum libzstd
 * computes when ZSTD_c_checksumFlag is set: encode.rs:163-167, 283-284.) */
int zk_xxh64_frames(zk_engine *e, const uint8_t *data, const uint64_t *off, uint32_t count, uint64_t *out);
int zk_xxh64_frames_dev(zk_engine *e, const void *d_data, const void *d_off, uint32_t count, void *d_out, void *stream);

/* ================================================================ Level B: the zeekstd API as C handles
 * One-to-one with the crate's public items; C++ callers can use the classes in
 * zeekstd_amd/csrc/host/zeekstd.hpp directly.  Functions that can fail return 0 / a negative code and
 * deliver values through out-pointers; zk_last_error_message() holds the Display text of the last error
 * on this thread (lib/src/error.rs:60-71). */
const char *zk_last_error_message(void);

#define ZK_FORMAT_HEAD 0 /* seek_table::Format (lib/src/seek_table.rs:228-241) */
#define ZK_FORMAT_FOOT 1

/* ---- SeekTable (lib/src/seek_table.rs:243-935) */
typedef struct zk_serializer zk_serializer;
zk_seek_table *zk_seek_table_new(void);                                                        /* SeekTable::new :287 */
zk_seek_table *zk_seek_table_clone(const zk_seek_table *t);
void zk_seek_table_free(zk_seek_table *t);
/* from_seekable_format over a BytesWrapper (seek_table.rs:379-436, seekable.rs:55-97) */
int zk_seek_table_from_bytes(const uint8_t *src, size_t len, int format, zk_seek_table **out);
/* from_reader (Head format, :461-493); max_read > 0 makes the reader return at most that many bytes per read */
int zk_seek_table_from_reader_bytes(const uint8_t *p, size_t len, size_t max_read, zk_seek_table **out);
int zk_seek_table_log_frame(zk_seek_table *t, uint32_t c_size, uint32_t d_size);               /* :513-525 */
/* the same for n frames in one call (the entries zk_encode_frames* returns, or a whole gathered shard: one call instead of one per
 * frame from a host language).  Stops at the first frame that cannot be logged (:513-525's errors); the frames before it stay. */
int zk_seek_table_log_frames(zk_seek_table *t, uint32_t n, const uint32_t *c_sizes, const uint32_t *d_sizes);
uint32_t zk_seek_table_num_frames(const zk_seek_table *t);                                     /* :540 */
uint32_t zk_seek_table_frame_index_comp(const zk_seek_table *t, uint64_t offset);              /* :560 */
uint32_t zk_seek_table_frame_index_decomp(const zk_seek_table *t, uint64_t offset);            /* :579 */
int zk_seek_table_frame_start_comp(const zk_seek_table *t, uint32_t index, uint64_t *out);     /* :604 */
int zk_seek_table_frame_start_decomp(const zk_seek_table *t, uint32_t index, uint64_t *out);   /* :633 */
int zk_seek_table_frame_end_comp(const zk_seek_table *t, uint32_t index, uint64_t *out);       /* :662 */
int zk_seek_table_frame_end_decomp(const zk_seek_table *t, uint32_t index, uint64_t *out);     /* :691 */
int zk_seek_table_frame_size_comp(const zk_seek_table *t, uint32_t index, uint64_t *out);      /* :720 */
int zk_seek_table_frame_size_decomp(const zk_seek_table *t, uint32_t index, uint64_t *out);    /* :750 */
uint64_t zk_seek_table_max_frame_size_comp(const zk_seek_table *t);                            /* :774 */
uint64_t zk_seek_table_max_frame_size_decomp(const zk_seek_table *t);                          /* :799 */
uint64_t zk_seek_table_size_comp(const zk_seek_table *t);                                      /* :827 */
uint64_t zk_seek_table_size_decomp(const zk_seek_table *t);                                    /* :853 */
int zk_seek_table_equal(const zk_seek_table *a, const zk_seek_table *b);                       /* PartialEq :266 */
/* the n+1 prefix sums (what zk_decode_frames takes); returns n+1 */
size_t zk_seek_table_entries(const zk_seek_table *t, uint64_t *c_off, uint64_t *d_off, size_t cap);
/* engine-specific (zk_refine_entries above): table t of the compressed stream src[0, len) -- the frames only -- refined to one entry per frame.
 * t == NULL: one entry over all of it, sizes unknown: the way to give a plain multi-frame .zst (pzstd output, `cat a.zst b.zst`) a seek
 * table.  The result is built with log_frame, so its errors apply (:513-525).  On a bad entry its code comes back, *out stays NULL and
 * zk_last_error_message says which error it was. */
int zk_seek_table_refine(zk_engine *e, const uint8_t *src, size_t len, const zk_seek_table *t, zk_seek_table **out);
/* ---- Serializer (seek_table.rs:937-1059): resumable at byte granularity, 0 == done */
zk_serializer *zk_seek_table_serializer(const zk_seek_table *t, int format);                   /* into_format_serializer :907 */
size_t zk_serializer_write_into(zk_serializer *s, uint8_t *buf, size_t len);                   /* :967-1005 */
void zk_serializer_reset(zk_serializer *s);                                                    /* :1034 */
size_t zk_serializer_encoded_len(const zk_serializer *s);                                      /* :1042 */
void zk_serializer_free(zk_serializer *s);

/* ---- DecodeOptions / Decoder (lib/src/decode.rs) */
typedef struct zk_decoder zk_decoder;
#define ZK_DEC_HAS_OFFSET 1u
#define ZK_DEC_HAS_OFFSET_LIMIT 2u
#define ZK_DEC_HAS_LOWER_FRAME 4u
#define ZK_DEC_HAS_UPPER_FRAME 8u
#define ZK_DEC_NO_VERIFY 16u
/* engine-specific: every zk_decoder_open_* refines the table it was given or parsed against the source before the first read
 * (zk_refine_entries; the source is read in groups of whole entries of at most 256 MiB compressed, a larger entry alone), and
 * zk_decoder_seek_table returns the refined table.  lower_frame / upper_frame index the table as given.  For archives whose entries hold several
 * frames or skippable frames, which fail with -72 / -10 otherwise.  A bad entry does not fail the open: it stays as it is and fails
 * when it is read.  The open itself runs zk_refine_entries: it fails (ZK_ERR_IO) while decode context 0 holds a submitted batch.  Without
 * the flag nothing changes. */
#define ZK_DEC_REFINE_ENTRIES 32u
typedef struct zk_decode_opts {          /* DecodeOptions builder fields, decode.rs:13-114 */
    uint32_t flags;
    uint32_t lower_frame, upper_frame;   /* :73, :81 (upper is inclusive) */
    uint64_t offset, offset_limit;       /* :90, :99 */
    const zk_seek_table *seek_table;     /* :65; NULL = parse it from the source's tail */
    uint64_t batch_bytes;                /* engine-specific: decode-ahead per GPU submission (0 = default 64 MiB) */
} zk_decode_opts;
#define ZK_SEEK_START 0
#define ZK_SEEK_END 1
#define ZK_SEEK_CURRENT 2
/* e == NULL: the decoder creates (and owns) an engine on device 0, like DecodeOptions::new creating a DCtx (:30).
 * The byte source is borrowed and must outlive the decoder (BytesWrapper<'a>). */
int zk_decoder_open_bytes(zk_engine *e, const uint8_t *src, size_t len, const zk_decode_opts *o, zk_decoder **out);
int zk_decoder_open_file(zk_engine *e, const char *path, const zk_decode_opts *o, zk_decoder **out);   /* Read+Seek source, seekable.rs:112-138 */
/* Any `impl Seekable` of the host (lib/src/seekable.rs:16-39).  set_offset: whence 0 = OffsetFrom::Start(value), 1 =
 * OffsetFrom::End(value); returns the new position counted from the start, or a negative value on failure.  read: bytes
 * delivered (0 = end of source), or negative on failure.  Failures surface as ZK_ERR_IO.  The engine pulls compressed bytes
 * through `read` straight into its pinned staging buffers; calls come from the thread that calls the decoder.
 * seek_table_integrity is a REQUIRED method of the trait (seekable.rs:33-38; each impl supplies it, :84-96, :126-137):
 * zk_decoder_open_seekable takes it as a third callback -- format 0 = Format::Head, 1 = Format::Foot; it fills the 9-byte
 * integrity field and returns 0, or a negative value on failure -- so a source that keeps the field elsewhere plugs in.
 * zk_decoder_open_callbacks is the two-callback form: the field is then read the way both of the reference's own impls
 * read it (seek to SKIPPABLE_HEADER_SIZE, or to End(-9), and read 9 bytes). */
typedef int64_t (*zk_seek_fn)(void *user, int whence, int64_t value);
typedef int64_t (*zk_read_fn)(void *user, uint8_t *buf, size_t len);
typedef int (*zk_integrity_fn)(void *user, int format, uint8_t out[9]);
int zk_decoder_open_callbacks(zk_engine *e, zk_seek_fn set_offset, zk_read_fn read, void *user, const zk_decode_opts *o, zk_decoder **out);
int zk_decoder_open_seekable(zk_engine *e, zk_seek_fn set_offset, zk_read_fn read, zk_integrity_fn seek_table_integrity, void *user,
                             const zk_decode_opts *o, zk_decoder **out);
void zk_decoder_free(zk_decoder *d);
int64_t zk_decoder_decompress(zk_decoder *d, uint8_t *buf, size_t len);                        /* :314; bytes written or <0 */
int zk_decoder_decompress_with_prefix(zk_decoder *d, uint8_t *buf, size_t len, const uint8_t *prefix, size_t plen, size_t *out); /* :201 */
void zk_decoder_reset(zk_decoder *d);                                                          /* :346 */
int zk_decoder_set_lower_frame(zk_decoder *d, uint32_t index, uint64_t *out);                  /* :367 */
int zk_decoder_set_upper_frame(zk_decoder *d, uint32_t index, uint64_t *out);                  /* :383 */
int zk_decoder_set_offset(zk_decoder *d, uint64_t offset);                                     /* :402 */
int zk_decoder_set_offset_limit(zk_decoder *d, uint64_t limit);                                /* :432 */
uint64_t zk_decoder_read_compressed(const zk_decoder *d);                                      /* :448 */
uint64_t zk_decoder_offset(const zk_decoder *d);                                               /* :458 */
uint64_t zk_decoder_offset_limit(const zk_decoder *d);                                         /* :463 */
zk_seek_table *zk_decoder_seek_table(const zk_decoder *d);                                     /* :453 (a copy; free it) */
int zk_decoder_seek(zk_decoder *d, int whence, int64_t n, uint64_t *out);                      /* io::Seek :545-579 */
uint64_t zk_decoder_gpu_submissions(const zk_decoder *d);                                      /* engine-specific counter */
/* Measurement helper (BASELINE.json configs[3]): n seeks one at a time -- set_offset(offs[i]);
 * set_offset_limit(offs[i] + lens[i]); decompress to exhaustion (decode.rs:402-437, 201-270) -- each timed on its own with
 * the monotonic clock, microseconds into us_out[i].  expect (optional): the archive's uncompressed bytes; every read is
 * compared with expect + offs[i] outside the timed span.  Returns 0, a decoder error, or ZK_ERR_ARGUMENT on a mismatch: the
 * loop stops there, us_out[i] of that seek is negated and buf holds what it delivered. */
int zk_decoder_time_seeks(zk_decoder *d, const uint64_t *offs, const uint32_t *lens, uint32_t n, uint8_t *buf, size_t buf_len,
                          const uint8_t *expect, double *us_out);

/* ---- EncodeOptions / RawEncoder / Encoder (lib/src/encode.rs) */
typedef struct zk_raw_encoder zk_raw_encoder;
typedef struct zk_encoder zk_encoder;
#define ZK_POLICY_UNCOMPRESSED 0 /* FrameSizePolicy::Uncompressed(n), encode.rs:21-39 (default, n = 0x200000) */
#define ZK_POLICY_COMPRESSED 1   /* FrameSizePolicy::Compressed(n): frame closes once its encoding reaches n bytes (probed speculatively) */
typedef struct zk_encode_opts {  /* EncodeOptions builder fields, encode.rs:110-207 */
    uint32_t policy, frame_size; /* frame_size 0 = default policy */
    int32_t level;               /* compression_level :170 (default 0) */
    int32_t checksum;            /* checksum_flag :164 (default false) */
    uint32_t batch_frames;       /* engine-specific: frames per GPU submission gathered by Encoder (0 = 64) */
} zk_encode_opts;
/* e == NULL: the encoder creates (and owns) an engine on device 0, like EncodeOptions::new creating a CCtx (:129) */
int zk_raw_encoder_new(zk_engine *e, const zk_encode_opts *o, zk_raw_encoder **out);                 /* with_opts :280 */
void zk_raw_encoder_free(zk_raw_encoder *r);
int zk_raw_encoder_compress(zk_raw_encoder *r, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len,
                            size_t *in_progress, size_t *out_progress);                                /* :398 */
int zk_raw_encoder_compress_with_prefix(zk_raw_encoder *r, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len,
                                        const uint8_t *prefix, size_t plen, size_t *in_progress, size_t *out_progress); /* :311 */
int zk_raw_encoder_end_frame(zk_raw_encoder *r, uint8_t *out, size_t out_len, size_t *out_progress, size_t *data_left); /* :438 */
zk_seek_table *zk_raw_encoder_seek_table(const zk_raw_encoder *r);                                    /* :487 (a copy) */
void zk_raw_encoder_reset_frame(zk_raw_encoder *r);                                                   /* :501 */
void zk_raw_encoder_reset_seek_table(zk_raw_encoder *r);                                              /* :524 */
/* engine-specific (ZSTD_CCtx_loadDictionary on the context the reference is handed with with_cctx, :142-155): the frames this handle writes are
 * encoded against the compiled dictionary (zk_encode_frames_dict above), under every policy; NULL = none.  There is no field for it in
 * zk_encode_opts, whose layout is ABI.  Allowed while no frame is open and nothing is buffered; otherwise -60 (stage_wrong, as
 * ZSTD_CCtx_loadDictionary) and nothing changes.  A non-empty explicit prefix on a call overrides the dictionary for the frames begun under
 * it, as in libzstd.  The zk_cdict must belong to the handle's engine and outlive the handle's use of it. */
int zk_raw_encoder_set_dictionary(zk_raw_encoder *r, const zk_cdict *cdict);
/* Encoder<W>: W is a write callback (return 0 on success) = io::Write::write_all */
typedef int (*zk_write_fn)(void *user, const uint8_t *data, size_t len);
int zk_encoder_new(zk_engine *e, const zk_encode_opts *o, zk_write_fn write, void *user, zk_encoder **out);   /* with_opts :596 */
/* A ready-made W for Encoder<W>: appends into caller memory like `Vec<u8>` does for the reference's benches
 * (lib/benches/compress.rs:47-51).  zk_buffer_writer_write is a zk_write_fn, `user` = the zk_buffer_writer.  With
 * `engine` set, large pieces are copied by the engine's worker threads.  A write past cap fails (-> ZK_ERR_IO). */
typedef struct zk_buffer_writer { uint8_t *data; uint64_t cap, len; zk_engine *engine; } zk_buffer_writer;
int zk_buffer_writer_write(void *user, const uint8_t *data, size_t len);
void zk_encoder_free(zk_encoder *e);
int64_t zk_encoder_compress(zk_encoder *e, const uint8_t *buf, size_t len);                           /* :692 / io::Write::write :791 */
int64_t zk_encoder_compress_with_prefix(zk_encoder *e, const uint8_t *buf, size_t len, const uint8_t *prefix, size_t plen); /* :641; the prefix buffer must stay valid and unchanged until the frames begun under it are out (end_frame / flush / finish) */
int64_t zk_encoder_end_frame(zk_encoder *e);                                                          /* :704 */
int zk_encoder_flush(zk_encoder *e);                                                                  /* io::Write::flush :796 */
int zk_encoder_set_dictionary(zk_encoder *e, const zk_cdict *cdict);                                  /* as zk_raw_encoder_set_dictionary */
int zk_encoder_finish(zk_encoder *e, int format, uint64_t *total);                                    /* finish_format :755 */
uint64_t zk_encoder_written_compressed(const zk_encoder *e);                                          /* :615 */
zk_seek_table *zk_encoder_seek_table(const zk_encoder *e);                                            /* :610 (a copy) */

#ifdef __cplusplus
}
#endif
#endif /* ZEEKSTD_AMD_H */

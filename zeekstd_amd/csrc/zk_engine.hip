// zk_engine.hip -- the batch engine behind the C ABI of include/zeekstd_amd.h (Level A).
// Owns the device scratch (frame infos, block list, sequence records, literal scratch) and
// sequences the kernel pipeline of zk_decode.hip / zk_encode.hip on one HIP stream.
// No CPU fallback: every entry point needs a live gfx950 device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_kernels.h"
#include "zk_dict.h"

int zk_devbuf_reserve(zk_engine *e, zk_devbuf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) ZK_HIP(hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    ZK_HIP(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

int zk_pin_reserve(zk_engine *e, uint8_t *&p, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return 0;
    if (p) ZK_HIP(hipHostFree(p));
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    ZK_HIP(hipHostMalloc((void **)&p, want, hipHostMallocDefault));
    cap = want;
    return 0;
}

void zk_profile_begin(zk_engine *e)
{
    if (!e->profiling) return;
    for (int k = 0; k < ZK_NKERNELS; k++) { e->ev_used[k] = false; e->kernel_ms[k] = 0.f; }
}
void zk_profile_collect(zk_engine *e)       // call after the stream has been synchronised
{
    if (!e->profiling) return;
    for (int k = 0; k < ZK_NKERNELS; k++)
        if (e->ev_used[k]) { float ms = 0.f; if (hipEventElapsedTime(&ms, e->ev_start[k], e->ev_stop[k]) == hipSuccess) e->kernel_ms[k] = ms; }
}

extern "C" int zk_engine_set_profiling(zk_engine *e, int on)
{
    if (!e) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    if (on && !e->ev_start[0])
        for (int k = 0; k < ZK_NKERNELS; k++) { ZK_HIP(hipEventCreate(&e->ev_start[k])); ZK_HIP(hipEventCreate(&e->ev_stop[k])); }
    e->profiling = on != 0;
    return 0;
}
extern "C" int zk_engine_set_kernel_choice(zk_engine *e, int what, int value)
{
    if (!e) return ZK_ERR_ARGUMENT;
    ZkKernelChoice &k = e->choice;
    switch (what) {
    case ZK_CHOICE_RESET: k = ZkKernelChoice(); e->pipe_contexts = 0; e->pipe_chunk_bytes = 0; e->range_pass_bytes = 0; e->enc.dense_slice_bytes = 0; e->enc.dict_slice_bytes = 0; e->enc.plan_choice = 0; e->enc.train_trial_bytes = 0; e->enc.cdc_slice_bytes = 0; e->enc.dedup_key_bits = 0; e->enc.dedup_slice_bytes = 0; e->enc.dedup_pass_bytes = 0; e->enc.compact_slice_bytes = 0; zk_hostpipe_tune(e); return 0;   // every key, the host pipeline's two included
    case ZK_CHOICE_FSE_OWN: if (value < 0 || value > 2) return ZK_ERR_ARGUMENT; k.fse_own = value; return 0;
    case ZK_CHOICE_FSE_SHARED: if (value < 0 || value > 3) return ZK_ERR_ARGUMENT; k.fse_shared = value; return 0;
    case ZK_CHOICE_EXEC_LANES: if (value != 0 && value != 128 && value != 256 && value != 512 && value != 1024) return ZK_ERR_ARGUMENT; k.exec_lanes = value; return 0;
    case ZK_CHOICE_EXEC_RING: if (value < 0 || value > 2) return ZK_ERR_ARGUMENT; k.exec_ring = value; return 0;
    case ZK_CHOICE_XXH64: if (value < 0 || value > 5) return ZK_ERR_ARGUMENT; k.xxh = value; return 0;
    case ZK_CHOICE_EXEC_RESIDENT: if (value != 0 && value != 4 && value != 5) return ZK_ERR_ARGUMENT; k.exec_resident = value; return 0;
    case ZK_CHOICE_SMALL_PATH: if (value < 0 || value > 2) return ZK_ERR_ARGUMENT; k.small_path = value; return 0;
    case ZK_CHOICE_EXEC_SEG: if (value < 0 || value > 2) return ZK_ERR_ARGUMENT; k.exec_seg = value; return 0;
    case ZK_CHOICE_SEG_KIB: if (value < 0 || value > 128) return ZK_ERR_ARGUMENT; k.seg_kib = value; return 0;
    case ZK_CHOICE_ENTROPY: if (value < 0 || value > 2) return ZK_ERR_ARGUMENT; k.entropy = value; return 0;
    case ZK_CHOICE_SEG_FILL: if (value < 0 || value > 3) return ZK_ERR_ARGUMENT; k.seg_fill = value; return 0;
    case ZK_CHOICE_PIPE_CONTEXTS: if (value < 0 || value > ZK_MAX_CTX) return ZK_ERR_ARGUMENT; e->pipe_contexts = value; zk_hostpipe_tune(e); return 0;
    case ZK_CHOICE_PIPE_CHUNK_MIB: if (value < 0 || value > 4096) return ZK_ERR_ARGUMENT; e->pipe_chunk_bytes = (uint64_t)value << 20; zk_hostpipe_tune(e); return 0;
    case ZK_CHOICE_RANGE_PASS_MIB: if (value < 0 || value > (1 << 20)) return ZK_ERR_ARGUMENT; e->range_pass_bytes = (uint64_t)value << 20; return 0;
    case ZK_CHOICE_ENC_DENSE_SLICE_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.dense_slice_bytes = (uint64_t)value << 10; return 0;
    case ZK_CHOICE_ENC_DICT_SLICE_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.dict_slice_bytes = (uint64_t)value << 10; return 0;
    case ZK_CHOICE_ENC_PLAN: if (value < 0 || value > 2) return ZK_ERR_ARGUMENT; e->enc.plan_choice = value; return 0;
    case ZK_CHOICE_TRAIN_TRIAL_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.train_trial_bytes = (uint64_t)value << 10; return 0;
    case ZK_CHOICE_CDC_SLICE_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.cdc_slice_bytes = (uint64_t)value << 10; return 0;
    case ZK_CHOICE_DEDUP_KEY_BITS: if (value < 0 || value > 64) return ZK_ERR_ARGUMENT; e->enc.dedup_key_bits = (uint32_t)value; return 0;
    case ZK_CHOICE_DEDUP_SLICE_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.dedup_slice_bytes = (uint64_t)value << 10; return 0;
    case ZK_CHOICE_DEDUP_PASS_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.dedup_pass_bytes = (uint64_t)value << 10; return 0;
    case ZK_CHOICE_COMPACT_SLICE_KIB: if (value < 0 || value > (1 << 22)) return ZK_ERR_ARGUMENT; e->enc.compact_slice_bytes = (uint64_t)value << 10; return 0;
    default: return ZK_ERR_ARGUMENT;
    }
}
extern "C" int zk_engine_set_fse_kernel(zk_engine *e, int mode) { return zk_engine_set_kernel_choice(e, ZK_CHOICE_FSE_OWN, mode); }
extern "C" uint64_t zk_engine_checksums_followed(const zk_engine *e) { return e ? e->followed : 0; }
extern "C" int zk_engine_entropy_fused(const zk_engine *e) { return e && e->entropy_fused ? 1 : 0; }
extern "C" int zk_engine_kernel_count(void) { return ZK_NKERNELS; }
extern "C" const char *zk_engine_kernel_name(int k)
{
    static const char *names[ZK_NKERNELS] = {"zk_k_walk(count)", "zk_k_scan", "zk_k_walk(fill)", "zk_k_huf", "zk_k_fse", "zk_k_exec",
                                             "zk_k_xxh64", "zk_k_status", "zk_k_enc_match", "zk_k_enc_entropy", "zk_k_enc_compact", "zk_k_enc_xxh64", "zk_k_enc_fse_build", "zk_k_enc_dense_cand",
                                             "zk_k_range_plan", "zk_k_range_pieces", "zk_k_range_gather", "zk_k_range_status",
                                             "zk_k_train_count", "zk_k_train_select", "zk_k_train_stats",
                                             "zk_k_cdc_mark", "zk_k_cdc_select",
                                             "zk_k_dedup_hash", "zk_k_dedup_insert", "zk_k_dedup_verify", "zk_k_dedup_verify_long", "zk_k_dedup_compact", "zk_k_dedup_gather",
                                             "zk_k_dxi_insert", "zk_k_dxi_lookup", "zk_k_dxi_compare", "zk_k_dxi_emit",
                                             "zk_k_cmp_mark", "zk_k_cmp_emit", "zk_k_cmp_move", "zk_k_cmp_remap_ids", "zk_k_cmp_take",
                                             "zk_k_view_plan", "zk_k_view_mark", "zk_k_view_gather", "zk_k_view_status",
                                             "zk_k_digest_plan", "zk_k_digest_leaves", "zk_k_digest_roots"};
    return k >= 0 && k < ZK_NKERNELS ? names[k] : "";
}
extern "C" int zk_engine_kernel_times(const zk_engine *e, float *ms_out, int n)
{
    if (!e || !ms_out) return ZK_ERR_ARGUMENT;
    for (int k = 0; k < n && k < ZK_NKERNELS; k++) ms_out[k] = e->kernel_ms[k];
    return 0;
}

extern "C" int zk_abi_version(void) { return ZK_ABI_VERSION; }

extern "C" const char *zk_error_name(int code)
{
    switch (code) {
    case 0: return "No error detected";
    case -1: return "Error (generic)";
    case -10: return "Unknown frame descriptor";
    case -12: return "Version not supported";
    case -14: return "Unsupported frame parameter";
    case -16: return "Frame requires too much memory for decoding";
    case -20: return "Data corruption detected";
    case -22: return "Restored data doesn't match checksum";
    case -30: return "Dictionary is corrupted";
    case -32: return "Dictionary mismatch";
    case -40: return "Unsupported parameter";
    case -42: return "Parameter is out of bound";
    case -64: return "Allocation error : not enough memory";
    case -70: return "Destination buffer is too small";
    case -72: return "Src size is incorrect";
    case -74: return "Operation on NULL destination buffer";
    case ZK_ERR_OFFSET_OUT_OF_RANGE: return "offset out of range";
    case ZK_ERR_FRAME_INDEX_TOO_LARGE: return "frame index too large";
    case ZK_ERR_NUMBER_CONVERSION: return "number conversion failed";
    case ZK_ERR_IO: return "io error";
    case ZK_ERR_HIP: return "HIP runtime error";
    case ZK_ERR_NO_DEVICE: return "no usable gfx950 device";
    case ZK_ERR_ARGUMENT: return "invalid argument";
    default: return "Unspecified error code";
    }
}

// The runtime multiplexes HIP streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and a copy queue that lands
// on the hardware queue of a compute queue serialises behind its kernels (the host pipeline then runs at 29 instead of
// 46 GiB/s).  The engine owns up to six queues, so it asks for eight -- effective when this library is loaded before the
// process initialises HIP; an explicit setting of the user wins.
__attribute__((constructor)) static void zk_ask_for_hw_queues(void) { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

extern "C" int zk_engine_create(int device, zk_engine **out)
{
    if (!out) return ZK_ERR_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return ZK_ERR_NO_DEVICE;
    zk_engine *e = new zk_engine();
    e->device = device;
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) { delete e; return ZK_ERR_NO_DEVICE; }
    snprintf(e->devname, sizeof e->devname, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { delete e; return ZK_ERR_NO_DEVICE; }   // kernels are built for gfx950 only
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return ZK_ERR_NO_DEVICE; }
    if (hipHostMalloc((void **)&e->h_words, 16 * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) { (void)hipStreamDestroy(e->stream); delete e; return ZK_ERR_HIP; }
    if (zk_dec_ctx_ready(e, 0) != 0 || zk_dec_ctx_ready(e, 1) != 0) { zk_engine_destroy(e); return ZK_ERR_HIP; }
    // the host pipeline's two copy queues are created right behind the two compute queues, before any second queue of a
    // context: streams are dealt onto the hardware queues in creation order
    if (zk_hostpipe_create(e) != 0) { zk_engine_destroy(e); return ZK_ERR_HIP; }
    *out = e;
    return 0;
}

extern "C" void zk_engine_destroy(zk_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    zk_hostpipe_destroy(e);
    if (e->enc.pin) (void)hipHostFree(e->enc.pin);
    if (e->enc.pin_lf) (void)hipHostFree(e->enc.pin_lf);
    if (e->enc.pin_off) (void)hipHostFree(e->enc.pin_off);
    if (e->enc.pin_dd) (void)hipHostFree(e->enc.pin_dd);
    for (auto &c : e->dctx) if (c.st) (void)hipStreamSynchronize(c.st);
    zk_devbuf *bufs[] = {&e->dict.buf, &e->st_prefix, &e->st_comp, &e->st_off, &e->st_dst, &e->st_misc, &e->rf_entries, &e->rf_frames,
                         &e->enc.lists, &e->enc.seqs, &e->enc.lits, &e->enc.scratch, &e->enc.words, &e->enc.ftab, &e->enc.hist, &e->enc.seg, &e->enc.ldm, &e->enc.dense, &e->enc.plan, &e->enc.train, &e->enc.train_src, &e->enc.cdc, &e->enc.cdc_src, &e->enc.cdc_off,
                         &e->enc.dd, &e->enc.dd_src, &e->enc.dd_off, &e->enc.dd_dry, &e->enc.dd_up, &e->enc.dd_out, &e->enc.dx, &e->enc.cmp, &e->enc.cmp_gaps, &e->enc.cmp_stage, &e->enc.dg, &e->enc.dg_up};
    for (zk_devbuf *b : bufs) if (b->p) (void)hipFree(b->p);
    if (e->h_words) (void)hipHostFree(e->h_words);
    for (int k = 0; k < ZK_NKERNELS; k++) { if (e->ev_start[k]) (void)hipEventDestroy(e->ev_start[k]); if (e->ev_stop[k]) (void)hipEventDestroy(e->ev_stop[k]); }
    for (int i = 0; i < ZK_MAX_CTX; i++) {
        zk_engine::DecCtx &c = e->dctx[i];
        for (zk_devbuf *b : {&c.infos, &c.bases, &c.words, &c.blocks, &c.seqs, &c.lit, &c.prog, &c.seg_tab, &c.seg_cnt, &c.seg_holes, &c.seg_tiles, &c.rng, &c.rng_meta}) if (b->p) (void)hipFree(b->p);
        if (c.h_words) (void)hipHostFree(c.h_words);
        for (hipEvent_t ev : {c.ev_fork, c.ev_join, c.ev_exec}) if (ev) (void)hipEventDestroy(ev);
        if (c.aux) (void)hipStreamDestroy(c.aux);
        if (c.st && i != 0) (void)hipStreamDestroy(c.st);     // context 0 runs on the engine's own stream
    }
    if (e->enc.aux) { (void)hipStreamSynchronize(e->enc.aux); (void)hipStreamDestroy(e->enc.aux); }
    for (hipEvent_t ev : {e->enc.ev_fork, e->enc.ev_join}) if (ev) (void)hipEventDestroy(ev);
    (void)hipStreamDestroy(e->stream);
    delete e;
}

extern "C" const char *zk_engine_last_hip_error(const zk_engine *e) { return e ? e->last_err.c_str() : ""; }
extern "C" const char *zk_engine_device_name(const zk_engine *e) { return e ? e->devname : ""; }

// ---------------------------------------------------------------------------------------------- decode
// ids / out_off (device arrays, both or neither): frame f of the batch is archive frame ids[f]; its bytes go to dst + out_off[f]
// One decode in flight per context: queues, scratch and pinned read-back words.  Context 0 is the engine's own (synchronous
// entry points, optionally on the caller's stream), context 1 exists for zk_decode_submit_dev; the host-pointer pipeline
// (zk_engine_host.hip) alternates between the two.
int zk_dec_ctx_ready(zk_engine *e, int slot)
{
    if (slot < 0 || slot >= ZK_MAX_CTX) return ZK_ERR_ARGUMENT;
    zk_engine::DecCtx &c = e->dctx[slot];
    if (c.ready) return 0;
    if (slot == 0) c.st = e->stream;
    else ZK_HIP(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
    ZK_HIP(hipEventCreateWithFlags(&c.ev_exec, hipEventDisableTiming));
    ZK_HIP(hipHostMalloc((void **)&c.h_words, 16 * sizeof(uint64_t), hipHostMallocDefault));
    c.ready = true;
    return 0;
}
// the second queue of a context (huf || fse of one batch) exists only once a batch asked for it: the host pipeline overlaps
// whole chunks on one queue per context, and every stream the process owns competes for the runtime's few hardware queues
int zk_dec_ctx_aux(zk_engine *e, zk_engine::DecCtx &c)
{
    if (c.aux) return 0;
    ZK_HIP(hipStreamCreateWithFlags(&c.aux, hipStreamNonBlocking));
    ZK_HIP(hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming));
    ZK_HIP(hipEventCreateWithFlags(&c.ev_join, hipEventDisableTiming));
    return 0;
}

// what the frame walk needs of the dictionary; nblocks: the batch's block count (0 for the counting pass, which writes no block entry)
static ZkWalkDict zk_dict_walk_args(const zk_engine *e, bool applies, uint64_t nblocks, bool fill)
{
    ZkWalkDict wd;
    if (!applies) return wd;
    wd.on = 1; wd.id = e->dict.id;
    if (e->dict.tables) {
        wd.def = (uint32_t)nblocks;                         // (the counting pass only asks "is a table in force": any index will do)
        if (fill) { wd.tmpl = e->dict.d_tmpl; wd.img = e->dict.d_img; }
    }
    return wd;
}

// ---- the stages (zk_engine.h)
int zk_dec_frame_tables(zk_engine *e, zk_engine::DecCtx &c, uint32_t count)
{
    int rc;
    if ((rc = zk_devbuf_reserve(e, c.infos, (size_t)count * sizeof(ZkFrameInfo)))) return rc;
    if ((rc = zk_devbuf_reserve(e, c.bases, (size_t)count * sizeof(ZkFrameBase)))) return rc;
    return zk_devbuf_reserve(e, c.words, 16 * sizeof(uint64_t));       // [0..2] totals, [3] first error (zk_dec_plan.h)
}
void zk_dec_walk(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a, bool with_dict, uint64_t nblocks, bool fill)
{
    zk_kernel_timer t(e, fill ? ZK_K_WALK_FILL : ZK_K_WALK_COUNT, st);
    zk_launch_walk(st, (const uint8_t *)a.d_comp, a.comp_size, (const uint64_t *)a.d_c_off, (const uint64_t *)a.d_d_off, a.first, a.count, a.ids, a.out_off, a.dst_cap,
                   fill ? (const ZkFrameBase *)c.bases.p : nullptr, fill ? (ZkBlock *)c.blocks.p : nullptr, (ZkFrameInfo *)c.infos.p, zk_dict_walk_args(e, with_dict, nblocks, fill));
}
int zk_dec_count_pass(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a, bool with_dict, uint32_t nwords)
{
    zk_dec_walk(e, c, st, a, with_dict, 0, false);
    { zk_kernel_timer t(e, ZK_K_SCAN, st); zk_launch_scan(st, (const ZkFrameInfo *)c.infos.p, a.count, (ZkFrameBase *)c.bases.p, (uint64_t *)c.words.p, (const uint64_t *)a.d_d_off, a.first, a.out_off); }
    ZK_HIP(hipMemcpyAsync(c.h_words, c.words.p, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return 0;
}
int zk_dec_block_scratch(zk_engine *e, zk_engine::DecCtx &c, uint64_t nblocks, uint64_t nseq)
{
    if (nblocks > 0xFFFFFFF0ull) return -(int)ZK_E_GENERIC;
    int rc;
    if ((rc = zk_devbuf_reserve(e, c.blocks, (size_t)(nblocks + 1) * sizeof(ZkBlock)))) return rc;
    return zk_devbuf_reserve(e, c.seqs, (size_t)(nseq + 1) * sizeof(ZkSeqP));
}
int zk_dec_seg_scratch(zk_engine *e, zk_engine::DecCtx &c, uint32_t count, const ZkSegPlan &sp, uint64_t out_bytes, uint64_t nblocks, ZkSegScratch &sgs)
{
    int rc;
    const uint64_t nsg = (uint64_t)count * sp.max_segs;
    if ((rc = zk_devbuf_reserve(e, c.seg_tab, (size_t)nsg * sizeof(ZkSeg)))) return rc;
    if ((rc = zk_devbuf_reserve(e, c.seg_cnt, (size_t)(nsg + count) * sizeof(uint32_t)))) return rc;
    if ((rc = zk_devbuf_reserve(e, c.seg_holes, (size_t)((out_bytes >> 2) + 16 * nsg + 16) * sizeof(ZkHole)))) return rc;
    if ((rc = zk_devbuf_reserve(e, c.seg_tiles, (size_t)((out_bytes >> 10) + 2 * nblocks + 8 * nsg + 16) * sizeof(uint32_t)))) return rc;
    sgs.seg_bytes = sp.seg_bytes; sgs.max_segs = sp.max_segs;
    sgs.segs = (ZkSeg *)c.seg_tab.p; sgs.nsegs = (uint32_t *)c.seg_cnt.p; sgs.segn = sgs.nsegs + count;
    sgs.holes = (ZkHole *)c.seg_holes.p; sgs.tilecnt = (uint32_t *)c.seg_tiles.p;
    return 0;
}
// checksums WHILE the executor writes (zk_k_xxh64_follow, zk_decode.hip): the executor publishes a progress word per frame, the
// checksum waves run on the context's second queue beside it, the ordinary pass behind the executor takes what they left
int zk_dec_follow_prepare(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, uint32_t count, uint64_t **prog)
{
    int rc;
    if ((rc = zk_devbuf_reserve(e, c.prog, (size_t)count * sizeof(uint64_t)))) return rc;
    if ((rc = zk_dec_ctx_aux(e, c))) return rc;
    *prog = (uint64_t *)c.prog.p;
    ZK_HIP(hipMemsetAsync(*prog, 0, (size_t)count * sizeof(uint64_t), st));
    return 0;
}
int zk_dec_fork(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st)
{
    ZK_HIP(hipEventRecord(c.ev_fork, st));
    ZK_HIP(hipStreamWaitEvent(c.aux, c.ev_fork, 0));
    return 0;
}
int zk_dec_exec_checksums(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a, const ZkSegScratch *sgs, const ZkDecShape &shape,
                          uint64_t nseq, uint64_t *prog, const uint32_t *rep_init)
{
    const uint8_t *comp = (const uint8_t *)a.d_comp, *lit = (const uint8_t *)c.lit.p;
    uint8_t *dst = (uint8_t *)a.d_dst;
    const uint64_t *d_off = (const uint64_t *)a.d_d_off;
    const ZkBlock *blocks = (const ZkBlock *)c.blocks.p;
    const ZkFrameBase *bases = (const ZkFrameBase *)c.bases.p;
    const ZkSeqP *seqs = (const ZkSeqP *)c.seqs.p;
    ZkFrameInfo *infos = (ZkFrameInfo *)c.infos.p;
    const uint64_t *x_off = a.out_off ? a.out_off : d_off;   // packed indexed output: out_off (count + 1 prefix sums) doubles as the d_off of the checksum kernels
    const uint32_t x_first = a.out_off ? 0 : a.first;
    const uint64_t plen = a.d_prefix ? a.prefix_len : 0;
    if (sgs) { zk_kernel_timer t(e, ZK_K_EXEC, st); zk_launch_exec_seg(st, comp, d_off, a.first, a.count, a.ids, a.out_off, blocks, bases, infos, seqs, lit, dst, *sgs, zk_exec_seg_plan(a.count, sgs->max_segs, nseq, shape.out_bytes, shape.k), prog); }
    else { zk_kernel_timer t(e, ZK_K_EXEC, st); zk_launch_exec(st, comp, d_off, a.first, a.count, a.ids, a.out_off, blocks, bases, infos, seqs, lit, dst, (const uint8_t *)a.d_prefix, plen, zk_exec_plan(a.count, nseq, shape.out_bytes, plen != 0, shape.follow, shape.k, a.neighbour && c.fused), prog, rep_init); }
    if (a.mark_exec) ZK_HIP(hipEventRecord(c.ev_exec, st));
    if (prog) {
        // enqueued BEHIND the executor's launch: were the two queues ever served one after the other, the checksum waves would find
        // finished frames, not wait (ZK_FOLLOW_PATIENCE) for an executor that cannot start
        zk_launch_xxh64_follow(c.aux, dst, x_off, x_first, a.count, infos, prog, zk_xxh_follow_plan(a.count));
        ZK_HIP(hipEventRecord(c.ev_join, c.aux));
        ZK_HIP(hipStreamWaitEvent(st, c.ev_join, 0));
        zk_launch_xxh64(st, dst, x_off, x_first, a.count, infos, nullptr, zk_xxh_plan(a.count, shape.k, true), prog);
    } else if (a.verify) { zk_kernel_timer t(e, ZK_K_XXH64, st); zk_launch_xxh64(st, dst, x_off, x_first, a.count, infos, nullptr, zk_xxh_plan(a.count, shape.k, false)); }
    return 0;
}

// Enqueue the whole decode on the context's queues.  Blocks the host once, for the block / sequence / literal totals
// that size the scratch (72 bytes, after the two cheapest kernels); returns with the rest still running.
int zk_decode_enqueue(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st, const zk_dec_args &a_in)
{
    // the engine's dictionary: its content is the prefix of every frame, its repeat offsets their first history, its tables the
    // ones in force at their first block (ZSTD_DCtx_loadDictionary)
    const bool with_dict = zk_dict_applies(e, a_in.d_prefix);
    zk_dec_args a = a_in;
    if (with_dict && e->dict.content_len) { a.d_prefix = e->dict.d_content; a.prefix_len = e->dict.content_len; }
    // history positions are 32-bit words biased by 2^30 (zk_device.h): a frame plus its prefix must fit below that
    if (a.d_prefix && a.prefix_len > ZK_MAX_PREFIX) return -(int)ZK_E_WINDOW_TOO_LARGE;
    const uint32_t count = a.count;
    int rc;
    if ((rc = zk_dec_frame_tables(e, c, count))) return rc;
    uint64_t *words = (uint64_t *)c.words.p;
    zk_profile_begin(e);
    if ((rc = zk_dec_count_pass(e, c, st, a, with_dict, ZK_SCAN_WORDS))) return rc;
    const uint64_t nblocks = c.h_words[ZK_SCAN_BLOCKS], nseq = c.h_words[ZK_SCAN_SEQS], nlit = c.h_words[ZK_SCAN_LITS], out_bytes = c.h_words[ZK_SCAN_OUT_BYTES];
    const uint32_t n_own = (uint32_t)c.h_words[ZK_SCAN_OWN_TABLES];
    a.verify = a.verify && c.h_words[ZK_SCAN_CHECKSUMMED] != 0;    // (a batch without a Content_Checksum: zeekstd's library default, encode.rs:163-167 -- no checksum kernel is launched)
    // the pass behind the shared-table kernels has to run whenever a dictionary lends tables (rest_always, zk_entropy_plan); no fused
    // kernel with per-kernel timing on, nor on one queue
    const ZkEntropyPlan ep = zk_entropy_plan((uint32_t)nblocks, n_own, count, e->choice, with_dict && e->dict.tables, e->profiling || a.single_queue);
    ZkDecShape shape = zk_dec_shape(e, count, out_bytes, c.h_words[ZK_SCAN_MAX_FRAME], nblocks, a.d_prefix != nullptr, a.alone);
    if ((rc = zk_dec_block_scratch(e, c, nblocks, nseq))) return rc;
    if ((rc = zk_devbuf_reserve(e, c.lit, (size_t)nlit + 64))) return rc;
    ZkBlock *blocks = (ZkBlock *)c.blocks.p;
    ZkSeqP *seqs = (ZkSeqP *)c.seqs.p;
    uint8_t *lit = (uint8_t *)c.lit.p;
    const uint8_t *comp = (const uint8_t *)a.d_comp;
    c.h_words[3] = ~0ull;
    ZK_HIP(hipMemcpyAsync(words + 3, c.h_words + 3, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // the checksums beside the executor (zk_dec_follow_prepare)?  (not in the host pipeline's chunks: they overlap whole chunks on one queue per context, PCIe bounds them, and the extra queues
    //  cost the copy queues 1-2 %: 46.4 -> 45.3 GiB/s end to end)
    const bool follow = shape.follow = a.verify && !a.single_queue && zk_follow_wanted(shape);      // (in segments: behind the fill pass's progress words)
    // The executor in segments (several workgroups per frame; zk_device.h): where a frame is long and the frames alone do not fill the device.
    const ZkSegPlan sp = zk_seg_plan_dev(shape);
    ZkSegScratch sgs{};
    if (sp.on && (rc = zk_dec_seg_scratch(e, c, count, sp, out_bytes, nblocks, sgs))) return rc;
    uint64_t *prog = nullptr;
    if (follow && (rc = zk_dec_follow_prepare(e, c, st, count, &prog))) return rc;
    ZK_HIP(hipMemsetAsync(words + 6, 0, sizeof(uint64_t), st));
    zk_dec_walk(e, c, st, a, with_dict, nblocks, true);
    // literals (huf) and sequences (fse) of a block are independent: the two kernels run side by side on two queues;
    // with per-kernel timing on they are serialised instead
    // ... or, where the sequences would get zk_k_fse_predef_fed, both in one kernel whose workgroups each bring a Huffman half and a
    // sequence half (zk_k_entropy_frame: no second queue, no events)
    c.fused = ep.fused;
    if (ep.fused) zk_launch_entropy(st, comp, blocks, (uint32_t)nblocks, seqs, lit, ep);
    else if (e->profiling || a.single_queue) {
        { zk_kernel_timer t(e, ZK_K_HUF, st); zk_launch_huf(st, comp, blocks, (uint32_t)nblocks, lit); }
        { zk_kernel_timer t(e, ZK_K_FSE, st); zk_launch_fse(st, comp, blocks, (uint32_t)nblocks, seqs, ep); }
    } else {
        if ((rc = zk_dec_ctx_aux(e, c)) || (rc = zk_dec_fork(e, c, st))) return rc;
        zk_launch_huf(c.aux, comp, blocks, (uint32_t)nblocks, lit);
        ZK_HIP(hipEventRecord(c.ev_join, c.aux));
        zk_launch_fse(st, comp, blocks, (uint32_t)nblocks, seqs, ep);
        ZK_HIP(hipStreamWaitEvent(st, c.ev_join, 0));
    }
    if (follow && (rc = zk_dec_fork(e, c, st))) return rc;  // (in front of the executor: the checksum waves start with it)
    if ((rc = zk_dec_exec_checksums(e, c, st, a, sp.on ? &sgs : nullptr, shape, nseq, prog, with_dict ? e->dict.rep : nullptr))) return rc;
    { zk_kernel_timer t(e, ZK_K_STATUS, st); zk_launch_status(st, (const ZkFrameInfo *)c.infos.p, count, (int32_t *)a.d_frame_status, words + 3, prog, words + 6); }
    ZK_HIP(hipMemcpyAsync(c.h_words + 3, words + 3, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return 0;
}
int zk_decode_finish(zk_engine *e, zk_engine::DecCtx &c, hipStream_t st)
{
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    e->entropy_fused = c.fused;
    e->followed = c.h_words[6] & 0xFFFFFFFFull;          // (the high half counts frames the checksum waves hashed and found different)
    if (c.h_words[3] != ~0ull) return -(int)(uint32_t)(c.h_words[3] & 0xFFFFFFFFu);
    return 0;
}

static int zk_decode_impl(zk_engine *e, const zk_dec_args &a, void *stream)
{
    if (!e || (a.count && (!a.d_comp || !a.d_c_off || !a.d_d_off || !a.d_dst))) return ZK_ERR_ARGUMENT;
    if (a.count == 0) return 0;
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;            // a submitted batch still owns context 0: zk_decode_wait first
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &c = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, c, stream);
    zk_dec_args b = a;
    b.alone = !e->slot_busy[1];                             // (a batch submitted on the other context would be its neighbour)
    b.neighbour = e->slot_busy[1];
    int rc = zk_decode_enqueue(e, c, st, b);
    if (rc) return rc;
    return zk_decode_finish(e, c, st);
}

extern "C" int zk_decode_submit_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off,
                                    const void *d_d_off, uint32_t first, uint32_t count, void *d_dst, uint64_t dst_cap,
                                    int verify, void *d_frame_status, int *slot_out)
{
    if (!e || !slot_out || count == 0 || !d_comp || !d_c_off || !d_d_off || !d_dst) return ZK_ERR_ARGUMENT;
    const int slot = e->next_slot;
    if (e->slot_busy[slot]) return ZK_ERR_ARGUMENT;         // both contexts in flight: zk_decode_wait the older one first
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &c = e->dctx[slot];
    zk_profiling_off quiet(e);                              // per-kernel events belong to the synchronous path
    zk_dec_args a{d_comp, comp_size, d_c_off, d_d_off, first, count, nullptr, nullptr, d_dst, dst_cap, verify, d_frame_status, nullptr, 0};
    a.neighbour = e->slot_busy[slot ^ 1];                   // (the first batch of a pipeline, or one submitted and waited for alone, has none)
    int rc = zk_decode_enqueue(e, c, c.st, a);
    if (rc) { (void)hipStreamSynchronize(c.st); return rc; }
    e->slot_busy[slot] = true;
    e->next_slot = slot ^ 1;
    *slot_out = slot;
    return 0;
}

extern "C" int zk_decode_wait(zk_engine *e, int slot)
{
    if (!e || slot < 0 || slot > 1 || !e->slot_busy[slot]) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    zk_profiling_off quiet(e);
    const int rc = zk_decode_finish(e, e->dctx[slot], e->dctx[slot].st);
    e->slot_busy[slot] = false;
    return rc;
}

extern "C" int zk_decode_frames_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off,
                                    const void *d_d_off, uint32_t first, uint32_t count, void *d_dst, uint64_t dst_cap,
                                    int verify, void *d_frame_status, void *stream)
{
    zk_dec_args a{d_comp, comp_size, d_c_off, d_d_off, first, count, nullptr, nullptr, d_dst, dst_cap, verify, d_frame_status, nullptr, 0};
    return zk_decode_impl(e, a, stream);
}

extern "C" int zk_decode_frames_prefix_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off,
                                           const void *d_d_off, uint32_t first, uint32_t count, const void *d_prefix, uint64_t prefix_len,
                                           void *d_dst, uint64_t dst_cap, int verify, void *d_frame_status, void *stream)
{
    zk_dec_args a{d_comp, comp_size, d_c_off, d_d_off, first, count, nullptr, nullptr, d_dst, dst_cap, verify, d_frame_status,
                  prefix_len ? d_prefix : nullptr, prefix_len};
    return zk_decode_impl(e, a, stream);
}

extern "C" int zk_decode_frame_list_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                                        const void *d_ids, const void *d_out_off, uint32_t count, void *d_dst, uint64_t dst_cap,
                                        int verify, void *d_frame_status, void *stream)
{
    if (count && (!d_ids || !d_out_off)) return ZK_ERR_ARGUMENT;
    zk_dec_args a{d_comp, comp_size, d_c_off, d_d_off, 0, count, (const uint32_t *)d_ids, (const uint64_t *)d_out_off, d_dst, dst_cap, verify,
                  d_frame_status, nullptr, 0};
    return zk_decode_impl(e, a, stream);
}

// ---------------------------------------------------------------------------------------------- dictionaries
// zk_dict: a dictionary parsed and validated on the host (zk_dict.h; no GPU involved).  zk_engine_set_dictionary uploads it once; every
// decode call of the engine then follows ZSTD_DCtx_loadDictionary (zk_decode_enqueue, zk_frame_content_sizes_dev).
extern "C" int zk_dict_create(const uint8_t *bytes, size_t len, zk_dict **out)
{
    if (!out || (len && !bytes)) return ZK_ERR_ARGUMENT;
    *out = nullptr;
    ZkDictLayout L;
    const uint32_t st = zk_dict_parse(bytes, len, L);
    if (st != ZK_OK) return -(int)st;
    if (len - L.content_off > ZK_MAX_PREFIX) return -(int)ZK_E_WINDOW_TOO_LARGE;     // the content is a prefix (zk_decode_frames_prefix)
    zk_dict *d = new zk_dict();
    d->bytes.assign(bytes, bytes + len);
    d->L = L;
    *out = d;
    return 0;
}
extern "C" void zk_dict_free(zk_dict *d) { delete d; }
extern "C" uint32_t zk_dict_id(const zk_dict *d) { return d ? d->L.id : 0; }
extern "C" size_t zk_dict_content_offset(const zk_dict *d) { return d ? d->L.content_off : 0; }

extern "C" int zk_engine_set_dictionary(zk_engine *e, const zk_dict *d)
{
    if (!e) return ZK_ERR_ARGUMENT;
    if (e->slot_busy[0] || e->slot_busy[1]) return ZK_ERR_ARGUMENT;     // a submitted batch decodes against the dictionary it was submitted with
    ZK_HIP(hipSetDevice(e->device));
    for (auto &c : e->dctx) if (c.st) ZK_HIP(hipStreamSynchronize(c.st));
    e->dict.on = false;
    if (!d || d->bytes.empty()) return 0;
    std::vector<uint8_t> img;
    ZkBlock blk;
    memset(&blk, 0, sizeof blk);
    if (d->L.formatted) zk_dict_block(d->bytes.data(), d->L, img, blk);
    // [block entry | its content, padded to 64 bytes | the dictionary's content | 64 readable bytes]
    const size_t img_at = 128, img_room = (img.size() + 63) & ~(size_t)63, content_at = img_at + img_room;
    const size_t content_len = d->bytes.size() - d->L.content_off;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->dict.buf, content_at + content_len + 64))) return rc;
    std::vector<uint8_t> h(content_at + content_len + 64, 0);
    memcpy(h.data(), &blk, sizeof blk);
    if (!img.empty()) memcpy(h.data() + img_at, img.data(), img.size());
    if (content_len) memcpy(h.data() + content_at, d->bytes.data() + d->L.content_off, content_len);
    ZK_HIP(hipMemcpy(e->dict.buf.p, h.data(), h.size(), hipMemcpyHostToDevice));
    const uint8_t *base = (const uint8_t *)e->dict.buf.p;
    e->dict.d_tmpl = (const ZkBlock *)base; e->dict.d_img = base + img_at; e->dict.d_content = base + content_at;
    e->dict.content_len = content_len;
    e->dict.tables = d->L.formatted; e->dict.id = d->L.id;
    e->dict.rep[0] = d->L.rep[0]; e->dict.rep[1] = d->L.rep[1]; e->dict.rep[2] = d->L.rep[2];
    e->dict.on = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------- frame sizes nobody knows yet
// What libzstd's streaming decoder needs no table for -- how many bytes a frame decodes to -- this engine is told by the seek table
// (lib/src/seek_table.rs:750).  A host that holds frames WITHOUT their entries (the Level-C shim under an unmodified zeekstd hands
// over what ZSTD_decompressStream receives, lib/src/decode.rs:243-245) asks first: header walk + sequence walks, no literals, no
// output.  A frame that carries Frame_Content_Size is walked like any other and its blocks' sum is held against the header's field
// (zk_k_frame_sizes: corruption_detected when they differ) -- the sizes reported are always what the blocks regenerate.
// (The host-pointer variant below relies on context 0's queue being the engine's own stream: its uploads and this call's kernels are
//  one queue, in order.)
extern "C" int zk_frame_content_sizes_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, uint32_t first, uint32_t count,
                                          void *d_sizes, void *d_frame_status, void *stream)
{
    if (!e || (count && (!d_comp || !d_c_off || !d_sizes || !d_frame_status))) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &c = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, c, stream);
    zk_profiling_off quiet(e);                              // (no per-kernel events here)
    const zk_dec_args a{d_comp, comp_size, d_c_off, nullptr, first, count, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0};
    const bool with_dict = zk_dict_applies(e, nullptr);
    int rc;
    if ((rc = zk_dec_frame_tables(e, c, count))) return rc;
    if ((rc = zk_dec_count_pass(e, c, st, a, with_dict, 6))) return rc;
    const uint64_t nblocks = c.h_words[ZK_SCAN_BLOCKS];
    if ((rc = zk_dec_block_scratch(e, c, nblocks, c.h_words[ZK_SCAN_SEQS]))) return rc;
    zk_dec_walk(e, c, st, a, with_dict, nblocks, true);
    ZkBlock *blocks = (ZkBlock *)c.blocks.p;
    zk_launch_fse(st, (const uint8_t *)d_comp, blocks, (uint32_t)nblocks, (ZkSeqP *)c.seqs.p, zk_entropy_plan((uint32_t)nblocks, (uint32_t)c.h_words[ZK_SCAN_OWN_TABLES], count, e->choice, with_dict && e->dict.tables, true));   // (true: no literals here, no fused kernel)
    zk_launch_frame_sizes(st, (const ZkFrameInfo *)c.infos.p, (const ZkFrameBase *)c.bases.p, blocks, count, (uint64_t *)d_sizes, (int32_t *)d_frame_status);
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return 0;
}
// host pointers: comp[c_off[first] .. c_off[first + count]) is uploaded, sizes[count] and frame_status[count] come back
extern "C" int zk_frame_content_sizes(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, uint32_t first, uint32_t count,
                                      uint64_t *sizes, int32_t *frame_status)
{
    if (!e || (count && (!comp || !c_off || !sizes || !frame_status))) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    const uint64_t lo = c_off[first], hi = c_off[first + count];
    if (hi < lo || hi > comp_size) return -(int)ZK_E_SRC_SIZE_WRONG;
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;            // refused before the staging: its uploads ride on context 0's queue, behind the batch
    ZK_HIP(hipSetDevice(e->device));
    int rc;
    std::vector<uint64_t> rel(count + 1);
    for (uint32_t i = 0; i <= count; i++) rel[i] = c_off[first + i] - lo;
    if ((rc = zk_devbuf_reserve(e, e->st_comp, (size_t)(hi - lo) + 64))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->st_off, (size_t)(count + 1) * 8))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->st_misc, (size_t)count * 12))) return rc;
    hipStream_t st = e->stream;
    ZK_HIP(hipMemsetAsync((uint8_t *)e->st_comp.p + (hi - lo), 0, 64, st));                  // readable padding behind the last frame
    ZK_HIP(hipMemcpyAsync(e->st_comp.p, comp + lo, hi - lo, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(e->st_off.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
    uint64_t *d_sizes = (uint64_t *)e->st_misc.p;
    int32_t *d_stat = (int32_t *)(d_sizes + count);
    if ((rc = zk_frame_content_sizes_dev(e, e->st_comp.p, hi - lo, e->st_off.p, 0, count, d_sizes, d_stat, nullptr))) return rc;
    ZK_HIP(hipMemcpy(sizes, d_sizes, (size_t)count * 8, hipMemcpyDeviceToHost));
    ZK_HIP(hipMemcpy(frame_status, d_stat, (size_t)count * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------- XXH64
extern "C" int zk_xxh64_frames_dev(zk_engine *e, const void *d_data, const void *d_off, uint32_t count, void *d_out, void *stream)
{
    if (!e || (count && (!d_off || !d_out))) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    // the kernels address frame i at data + (off[i] - off[0]) (the decoder hands them its output, which begins with the batch's first
    // frame); this entry point hashes data[off[i], off[i+1]) as documented, so they get the data pointer moved by off[0]
    // (found by tests/test_gpu_past_4gib.py: a table that did not start at 0 hashed the wrong bytes)
    uint64_t off0 = 0;
    ZK_HIP(hipMemcpyAsync(&off0, d_off, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    zk_launch_xxh64(st, (const uint8_t *)d_data + off0, (const uint64_t *)d_off, 0, count, nullptr, (uint64_t *)d_out, zk_xxh_plan(count, e->choice, false));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return 0;
}


// zk_compact.hip -- zk_mark_frames_dev, zk_compact_archive_dev, zk_remap_ids_dev, zk_dedup_index_compact_dev: frames removed from a
// device-resident archive (include/zeekstd_amd.h; the kernels, the rule and the plan functions: zk_compact.h).
//   the compaction   zk_k_cmp_flags, zk_k_scan64 three times, zk_k_cmp_emit -- remap, the new offsets and the run table go to scratch, the
//                    totals to words the host reads -- and, in place, zk_k_cmp_step_gaps; ONE wait for the words, behind which every refusal
//                    is decided.  Then the outputs are copied out of the scratch and the bytes move: out of place in one launch of
//                    zk_k_cmp_move over [c_off[0], written); in place in the steps of zkc_nsteps from the first removed frame on, each
//                    direct or staged as zkc_step_direct says.  A wait at the end.
//   the index        remap checked on the device (flags, zk_k_scan64, zk_k_cmp_remap_check; a wait), zk_k_cmp_take into scratch, the kept
//                    keys and lengths copied to the front of the index's arrays, the table rebuilt as zk_dedup_index_truncate rebuilds it.
// All scratch is the encoder's (zk_engine::Enc::cmp*) and the index's own memory: no decode context is touched, so the calls are served
// while batches of zk_decode_submit_dev are in flight.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_compact.h"

static_assert(ZKC_REMOVED == ZK_FRAME_REMOVED, "zk_compact.h restates ZK_FRAME_REMOVED");

namespace {
constexpr uint32_t ZKC_STEPS_MAX = 1u << 22;                // steps whose gap is asked for; a step beyond them is staged
inline bool zkc_overlap(const void *a, uint64_t an, const void *b, uint64_t bn)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return an && bn && a0 < b0 + bn && b0 < a0 + an;
}
inline void zkc_launch_move(hipStream_t st, const uint8_t *src, uint8_t *out, uint64_t obase, const uint64_t *rsrc, const uint64_t *rdst, uint32_t nruns, uint64_t lo,
                            uint64_t hi)
{
    hipLaunchKernelGGL(zk_k_cmp_move, dim3(zkc_move_grid(hi - lo)), dim3(ZKC_THREADS), 0, st, src, out, obase, rsrc, rdst, nruns, lo, hi);
}
}  // namespace

extern "C" int zk_mark_frames_dev(zk_engine *e, const void *d_ids, uint32_t count, uint32_t n_frames, void *d_live, void *stream)
{
    if (!e) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    if (!d_ids || !d_live) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.cmp, 64))) return rc;
    uint32_t *err = (uint32_t *)e->enc.cmp.p, bad = 0;
    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(err, 0, 4, st));
    zk_kernel_timer t(e, ZK_K_CMP_MARK, st);
    // check first, then write: a refused call leaves live as it was
    hipLaunchKernelGGL(zk_k_cmp_check_ids, dim3(zkc_blocks(count)), dim3(ZKC_THREADS), 0, st, (const uint32_t *)d_ids, count, n_frames, err);
    ZK_HIP(hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    if (bad) return ZK_ERR_ARGUMENT;
    hipLaunchKernelGGL(zk_k_cmp_mark, dim3(zkc_blocks(count)), dim3(ZKC_THREADS), 0, st, (const uint32_t *)d_ids, count, (uint8_t *)d_live);
    if (t.on) { (void)hipEventRecord(e->ev_stop[ZK_K_CMP_MARK], st); t.on = false; }
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    return 0;
}

extern "C" int zk_compact_archive_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                                      const void *d_live, void *d_dst, uint64_t dst_cap, void *d_c_off_out, void *d_d_off_out, void *d_remap,
                                      uint32_t *n_kept, uint64_t *written, void *stream)
{
    uint32_t nk_dummy;
    uint64_t wr_dummy;
    if (!n_kept) n_kept = &nk_dummy;
    if (!written) written = &wr_dummy;
    *n_kept = 0; *written = 0;
    if (!e) return ZK_ERR_ARGUMENT;
    if (n_frames > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    if (n_frames == 0) {
        if (d_c_off) { ZK_HIP(hipMemcpyAsync(written, d_c_off, 8, hipMemcpyDeviceToHost, st)); ZK_HIP(hipStreamSynchronize(st)); }
        return 0;
    }
    if (!d_comp || !d_c_off || !d_d_off || !d_live || !d_dst) return ZK_ERR_ARGUMENT;
    const bool in_place = d_dst == d_comp;
    if (!in_place && zkc_overlap(d_dst, dst_cap, d_comp, comp_size + ZK_COMP_PADDING)) return ZK_ERR_ARGUMENT;
    const uint32_t n = n_frames;
    const ZkCmpLayout L = zkc_layout(n);
    const uint64_t step = zkc_step_bytes(e->enc.compact_slice_bytes);
    const uint32_t max_steps = !in_place ? 0 : comp_size / step + 2 < ZKC_STEPS_MAX ? (uint32_t)(comp_size / step + 2) : ZKC_STEPS_MAX;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.cmp, L.end + 64))) return rc;
    if (in_place && (rc = zk_devbuf_reserve(e, e->enc.cmp_gaps, (size_t)max_steps * 8))) return rc;
    uint8_t *b = (uint8_t *)e->enc.cmp.p;
    uint64_t *fk = (uint64_t *)(b + L.fk), *pk = (uint64_t *)(b + L.pk), *fc = (uint64_t *)(b + L.fc), *pc = (uint64_t *)(b + L.pc), *fd = (uint64_t *)(b + L.fd),
             *pd = (uint64_t *)(b + L.pd), *co = (uint64_t *)(b + L.co), *dof = (uint64_t *)(b + L.dof), *rsrc = (uint64_t *)(b + L.rsrc), *rdst = (uint64_t *)(b + L.rdst),
             *words = (uint64_t *)(b + L.words), *gaps = (uint64_t *)e->enc.cmp_gaps.p;
    uint32_t *remap = (uint32_t *)(b + L.remap);
    const uint64_t *c_off = (const uint64_t *)d_c_off, *d_off = (const uint64_t *)d_d_off;
    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(words, 0, 8 * ZKC_W_WORDS, st));
    {
        zk_kernel_timer t(e, ZK_K_CMP_EMIT, st);
        const dim3 grid(zkc_blocks((uint64_t)n + 1)), block(ZKC_THREADS);
        hipLaunchKernelGGL(zk_k_cmp_flags, grid, block, 0, st, c_off, d_off, (const uint8_t *)d_live, n, fk, fc, fd, (uint32_t *)words);
        zk_launch_scan64(st, fk, n + 1, pk);
        zk_launch_scan64(st, fc, n + 1, pc);
        zk_launch_scan64(st, fd, n + 1, pd);
        hipLaunchKernelGGL(zk_k_cmp_emit, grid, block, 0, st, c_off, d_off, n, fk, pk, pc, pd, remap, co, dof, rsrc, rdst, words);
        if (in_place) hipLaunchKernelGGL(zk_k_cmp_step_gaps, dim3(zkc_blocks(max_steps)), block, 0, st, rsrc, rdst, words, step, max_steps, gaps);
    }
    uint64_t w[ZKC_W_WORDS] = {};
    std::vector<uint64_t> h_gaps(max_steps);
    ZK_HIP(hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, st));
    if (in_place) ZK_HIP(hipMemcpyAsync(h_gaps.data(), gaps, (size_t)max_steps * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));                       // the checks and the totals
    ZK_HIP(hipGetLastError());
    if ((uint32_t)w[ZKC_W_ERR] || w[ZKC_W_END] > comp_size) return ZK_ERR_ARGUMENT;
    const uint32_t nk = (uint32_t)w[ZKC_W_KEPT], nruns = (uint32_t)w[ZKC_W_RUNS];
    const uint64_t wr = w[ZKC_W_WRITTEN];
    if (!in_place && wr > dst_cap) { *written = wr; return -(int)ZK_E_DST_TOO_SMALL; }
    // nothing refuses the call from here on.  (In place the offsets may be the caller's own arrays: the kernels have read them.)
    uint64_t staged_max = 0;
    const uint64_t lo = in_place ? w[ZKC_W_FIRST_REMOVED] : w[ZKC_W_BEGIN], moved = wr > lo ? wr - lo : 0, nsteps = in_place ? zkc_nsteps(moved, step) : 0;
    const auto direct = [&](uint64_t k) { return zkc_step_direct(k < max_steps ? h_gaps[k] : 0, zkc_step_end(k, step, moved) - zkc_step_begin(k, step)); };
    for (uint64_t k = 0; k < nsteps; k++) if (!direct(k)) { staged_max = zkc_stage_bytes(moved, step); break; }
    if (staged_max && (rc = zk_devbuf_reserve(e, e->enc.cmp_stage, (size_t)staged_max + 64))) return rc;
    if (d_remap) ZK_HIP(hipMemcpyAsync(d_remap, remap, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    if (d_c_off_out) ZK_HIP(hipMemcpyAsync(d_c_off_out, co, ((size_t)nk + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (d_d_off_out) ZK_HIP(hipMemcpyAsync(d_d_off_out, dof, ((size_t)nk + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (nruns && moved) {
        // (one pair of events round every step: the copies of the staged ones are part of the move)
        zk_kernel_timer t(e, ZK_K_CMP_MOVE, st);
        const uint8_t *src = (const uint8_t *)d_comp;
        uint8_t *dst = (uint8_t *)d_dst, *stage = (uint8_t *)e->enc.cmp_stage.p;
        if (!in_place) zkc_launch_move(st, src, dst, 0, rsrc, rdst, nruns, lo, wr);
        for (uint64_t k = 0; k < nsteps; k++) {
            const uint64_t a = lo + zkc_step_begin(k, step), z = lo + zkc_step_end(k, step, moved);
            if (direct(k)) zkc_launch_move(st, src, dst, 0, rsrc, rdst, nruns, a, z);
            else {
                zkc_launch_move(st, src, stage, a, rsrc, rdst, nruns, a, z);
                ZK_HIP(hipMemcpyAsync(dst + a, stage, (size_t)(z - a), hipMemcpyDeviceToDevice, st));
            }
        }
    }
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    *n_kept = nk;
    *written = wr;
    return 0;
}

extern "C" int zk_remap_ids_dev(zk_engine *e, const void *d_remap, uint32_t n_frames, const void *d_ids, uint32_t count, void *d_ids_out, void *stream)
{
    if (!e) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    if (!d_remap || !d_ids || !d_ids_out) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.cmp, 16 + (size_t)count * 4 + 64))) return rc;
    uint32_t *err = (uint32_t *)e->enc.cmp.p, *out = err + 4, bad = 0;
    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(err, 0, 4, st));
    {
        zk_kernel_timer t(e, ZK_K_CMP_REMAP, st);
        hipLaunchKernelGGL(zk_k_cmp_remap_ids, dim3(zkc_blocks(count)), dim3(ZKC_THREADS), 0, st, (const uint32_t *)d_remap, n_frames, (const uint32_t *)d_ids, count, out, err);
    }
    ZK_HIP(hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    if (bad) return ZK_ERR_ARGUMENT;                        // (the new ids are in scratch: ids_out is as it was)
    ZK_HIP(hipMemcpyAsync(d_ids_out, out, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int zk_dedup_index_compact_dev(zk_dedup_index *x, const void *d_remap, uint32_t n_frames, void *stream)
{
    if (!x) return ZK_ERR_ARGUMENT;
    const ZkDxArrays A = zk_dedup_index_arrays(x);
    if (n_frames != A.m) return ZK_ERR_ARGUMENT;
    if (n_frames == 0) return 0;
    if (!d_remap) return ZK_ERR_ARGUMENT;
    zk_engine *e = A.e;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    const uint32_t n = n_frames;
    // flags[n + 1] | pos[n + 2] | keys_out[n] | lens_out[n] | err
    const size_t pos_at = 8 * ((size_t)n + 1), keys_at = pos_at + 8 * ((size_t)n + 2), lens_at = keys_at + 8 * (size_t)n, err_at = (lens_at + 4 * (size_t)n + 15) & ~(size_t)15;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.cmp, err_at + 64))) return rc;
    uint8_t *b = (uint8_t *)e->enc.cmp.p;
    uint64_t *flags = (uint64_t *)b, *pos = (uint64_t *)(b + pos_at), *keys_out = (uint64_t *)(b + keys_at), kept = 0;
    uint32_t *lens_out = (uint32_t *)(b + lens_at), *err = (uint32_t *)(b + err_at), bad = 0;
    const uint32_t *remap = (const uint32_t *)d_remap;
    const dim3 block(ZKC_THREADS);
    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(err, 0, 4, st));
    hipLaunchKernelGGL(zk_k_cmp_remap_flags, dim3(zkc_blocks((uint64_t)n + 1)), block, 0, st, remap, n, flags);
    zk_launch_scan64(st, flags, n + 1, pos);
    hipLaunchKernelGGL(zk_k_cmp_remap_check, dim3(zkc_blocks(n)), block, 0, st, remap, n, pos, err);
    ZK_HIP(hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(&kept, pos + n, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    if (bad) return ZK_ERR_ARGUMENT;                        // not a compaction's remap: the index is as it was
    const uint32_t nk = (uint32_t)kept;
    {
        zk_kernel_timer t(e, ZK_K_CMP_TAKE, st);
        hipLaunchKernelGGL(zk_k_cmp_take, dim3(zkc_blocks(n)), block, 0, st, remap, n, (const uint64_t *)A.keys, (const uint32_t *)A.lens, keys_out, lens_out);
    }
    if (nk) {
        ZK_HIP(hipMemcpyAsync(A.keys, keys_out, (size_t)nk * 8, hipMemcpyDeviceToDevice, st));
        ZK_HIP(hipMemcpyAsync(A.lens, lens_out, (size_t)nk * 4, hipMemcpyDeviceToDevice, st));
    }
    return zk_dedup_index_rebuilt(x, st, nk);
}

// zk_view.hip -- zk_read_view_ranges_dev (include/zeekstd_amd.h): byte ranges of a VIEW of a device-resident archive -- the ids / off pair
// the dedup calls return -- many per call.  The view is checked whole and the plan made on the device (zk_view.h), the distinct frames that
// touched entries name decoded ONCE each through zk_decode_enqueue into engine-owned scratch -- pass after pass over slices of the sorted
// frame list when they exceed the pass size, as zk_read_ranges_dev does --, the wanted bytes copied out by zk_k_view_gather, a status per range.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_kernels.h"
#include "zk_view.h"

static_assert(ZKV_SMALL == ZK_RANGE_SMALL && ZKV_CHUNK == ZK_RANGE_CHUNK, "a view's ranges are dealt as an archive's are");

namespace {
// the plan's arrays (zkv_sizes), carved out of one allocation (every piece 16-byte aligned)
struct Carver {
    uint8_t *base; size_t at = 0;
    template <typename T> T *take(size_t n) { T *p = base ? (T *)(base + at) : nullptr; at += (n * sizeof(T) + 15) & ~(size_t)15; return p; }
};
struct ViewMeta {
    uint64_t *eff, *cnt, *packed, *coff, *uoff, *poff, *words;
    uint32_t *efirst, *elast, *ecover, *seg, *super, *fcover, *ebase, *slot, *uids;
    int32_t *status, *fstat;
    size_t zero_bytes, bytes;       // ecover | seg | super | fcover: cleared together
    ViewMeta(void *p, uint32_t count, uint32_t vcount, uint32_t n_frames)
    {
        Carver c{(uint8_t *)p};
        const ZkViewSizes s = zkv_sizes(count, vcount, n_frames);
        eff = c.take<uint64_t>(s.eff); cnt = c.take<uint64_t>(s.cnt); packed = c.take<uint64_t>(s.packed); coff = c.take<uint64_t>(s.coff);
        uoff = c.take<uint64_t>(s.uoff); poff = c.take<uint64_t>(s.poff); words = c.take<uint64_t>(ZKV_W_WORDS);
        efirst = c.take<uint32_t>(s.efirst); elast = c.take<uint32_t>(s.elast);
        const size_t z0 = c.at;
        ecover = c.take<uint32_t>(s.ecover); seg = c.take<uint32_t>(s.seg); super = c.take<uint32_t>(s.super); fcover = c.take<uint32_t>(s.fcover);
        zero_bytes = c.at - z0;
        ebase = c.take<uint32_t>(s.ebase); slot = c.take<uint32_t>(s.slot); uids = c.take<uint32_t>(s.uids);
        status = c.take<int32_t>(s.status); fstat = c.take<int32_t>(s.fstat);
        bytes = c.at;
    }
};
struct ViewArgs {
    const uint64_t *d_off; uint32_t n_frames;
    const uint32_t *ids; const uint64_t *voff; uint32_t vcount;
    const uint64_t *offs, *lens, *dst_off; uint32_t count; uint8_t *dst; uint64_t dst_cap;
};

// check, destinations, plan, the touched entries' frames, the sorted distinct frame list (words[ZKV_W_FRAMES], [ZKV_W_BYTES]) and the chunk sums
void launch_view_plan(zk_engine *e, hipStream_t st, const ViewArgs &v, const ViewMeta &m)
{
    const dim3 tb(ZKV_THREADS);
    uint32_t *err = (uint32_t *)(m.words + ZKV_W_VIEW_ERR);
    {
        zk_kernel_timer t(e, ZK_K_VIEW_PLAN, st);
        if (v.vcount) hipLaunchKernelGGL(zk_k_view_check, dim3(zkv_blocks(v.vcount)), tb, 0, st, v.d_off, v.n_frames, v.ids, v.voff, v.vcount, err);
        if (!v.dst_off) {
            hipLaunchKernelGGL(zk_k_view_lens, dim3(zkv_blocks(v.count)), tb, 0, st, v.voff, v.vcount, v.offs, v.lens, v.count, m.eff);
            zk_launch_scan64(st, m.eff, v.count, m.packed);
        }
        hipLaunchKernelGGL(zk_k_view_plan, dim3(zkv_blocks(v.count)), tb, 0, st, v.voff, v.vcount, v.offs, v.lens, v.dst_off ? v.dst_off : m.packed, v.count, v.dst_cap,
                           (uintptr_t)v.dst, m.efirst, m.elast, m.status, m.ecover, m.seg, m.super, m.cnt);
        zk_launch_scan64(st, m.cnt, v.count, m.coff);
    }
    {
        zk_kernel_timer t(e, ZK_K_VIEW_MARK, st);
        const uint32_t nseg = zkv_nseg(v.vcount);
        hipLaunchKernelGGL(zk_k_view_bases, dim3(zkv_blocks(nseg)), tb, 0, st, m.seg, m.super, nseg, m.ebase);
        if (v.vcount) hipLaunchKernelGGL(zk_k_view_mark, dim3(zkv_blocks(v.vcount)), tb, 0, st, v.ids, v.voff, v.vcount, m.ecover, m.ebase, err, m.fcover);
        zk_launch_range_compact(st, v.d_off, v.n_frames, m.fcover, m.slot, m.uids, m.uoff, m.words);
    }
}
void launch_view_gather(hipStream_t st, const ViewArgs &v, const ViewMeta &m, const uint64_t *dst_off, const uint8_t *scratch, uint32_t a, uint32_t b)
{
    const uint32_t small_wgs = zkv_small_wgs(v.count);
    hipLaunchKernelGGL(zk_k_view_gather, dim3(small_wgs + zkv_chunk_wgs(v.count, v.dst_cap)), dim3(ZKV_THREADS), 0, st, scratch, v.dst, v.ids, v.voff, v.vcount, v.offs,
                       v.lens, dst_off, m.efirst, m.coff, v.count, m.slot, m.uoff, a, b, small_wgs);
}
void launch_view_status(hipStream_t st, const ViewArgs &v, const ViewMeta &m, bool any_failed, const uint64_t *pass_err, int32_t *out)
{
    hipLaunchKernelGGL(zk_k_view_status, dim3(zkv_blocks(v.count)), dim3(ZKV_THREADS), 0, st, v.ids, v.voff, v.count, m.efirst, m.elast, m.slot, m.fstat,
                       any_failed ? 1 : 0, pass_err, m.status, out, (unsigned long long *)(m.words + ZKV_W_FIRST_ERR));
}
}   // namespace

extern "C" int zk_read_view_ranges_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                                       const void *d_view_ids, const void *d_view_off, uint32_t view_count,
                                       const void *d_offs, const void *d_lens, const void *d_dst_off, uint32_t count, void *d_dst, uint64_t dst_cap,
                                       int verify, void *d_range_status, void *stream)
{
    if (!e || !d_d_off || !d_view_off || (view_count && !d_view_ids) || (count && (!d_offs || !d_lens)) || (n_frames && (!d_comp || !d_c_off))) return ZK_ERR_ARGUMENT;
    if (count && e->slot_busy[0]) return ZK_ERR_ARGUMENT;   // a submitted batch still owns context 0: zk_decode_wait first (nothing touched, the counter included)
    e->ranges_frames = 0;
    if (count == 0) return 0;
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &x = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, x, stream);
    int rc;
    if ((rc = zk_devbuf_reserve(e, x.rng_meta, ViewMeta(nullptr, count, view_count, n_frames).bytes))) return rc;
    if ((rc = zk_devbuf_reserve(e, x.words, 16 * sizeof(uint64_t)))) return rc;
    const ViewMeta m(x.rng_meta.p, count, view_count, n_frames);
    const ViewArgs v{(const uint64_t *)d_d_off, n_frames, (const uint32_t *)d_view_ids, (const uint64_t *)d_view_off, view_count,
                     (const uint64_t *)d_offs, (const uint64_t *)d_lens, (const uint64_t *)d_dst_off, count, (uint8_t *)d_dst, dst_cap};
    const uint64_t *dst_off = v.dst_off ? v.dst_off : m.packed;
    // the statuses stay in the engine's array until the view is known to be good: a refused view leaves d_range_status as it was
    int32_t *status_out = d_range_status ? (int32_t *)d_range_status : m.status;
    uint64_t *hw = e->h_words + ZK_HW_RANGES;               // [0] frames touched, [1] their decompressed bytes, [2] the view's error bits, later the first failing range

    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(m.ecover, 0, m.zero_bytes, st));
    ZK_HIP(hipMemsetAsync(m.words + ZKV_W_VIEW_ERR, 0, sizeof(uint64_t), st));
    ZK_HIP(hipMemsetAsync(m.words + ZKV_W_FIRST_ERR, 0xFF, sizeof(uint64_t), st));
    launch_view_plan(e, st, v, m);
    ZK_HIP(hipMemcpyAsync(hw, m.words, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    float plan_ms = 0.f, mark_ms = 0.f;
    if (e->profiling) {
        (void)hipEventElapsedTime(&plan_ms, e->ev_start[ZK_K_VIEW_PLAN], e->ev_stop[ZK_K_VIEW_PLAN]);
        (void)hipEventElapsedTime(&mark_ms, e->ev_start[ZK_K_VIEW_MARK], e->ev_stop[ZK_K_VIEW_MARK]);
    }
    if (hw[2] != 0) return ZK_ERR_ARGUMENT;                 // the view is not one of this archive: nothing decoded, nothing written
    const uint32_t nt = (uint32_t)hw[0];
    const uint64_t bytes = hw[1];
    if (nt && !d_dst) return ZK_ERR_ARGUMENT;

    // Passes over slices [a, b) of the distinct frames, each at most `cap` decoded bytes and at least one frame (zk_read_ranges_dev's loop).
    uint64_t cap = e->range_pass_bytes ? e->range_pass_bytes : ZK_RANGE_PASS_DEFAULT;
    std::vector<uint64_t> h_uoff;
    bool any_failed = false, status_queued = false;
    for (uint32_t a = 0; a < nt;) {
        uint32_t b = nt;
        uint64_t pass_bytes = bytes;
        if (a != 0 || bytes > cap) {
            if (h_uoff.empty()) {
                h_uoff.resize((size_t)nt + 1);
                ZK_HIP(hipMemcpyAsync(h_uoff.data(), m.uoff, ((size_t)nt + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
                ZK_HIP(hipStreamSynchronize(st));
            }
            b = a + 1;
            while (b < nt && h_uoff[b + 1] - h_uoff[a] <= cap) b++;
            pass_bytes = h_uoff[b] - h_uoff[a];
        }
        // scratch the device cannot give: half the pass, down to one frame, before the error is the caller's
        rc = zk_devbuf_reserve(e, x.rng, (size_t)pass_bytes + 64);
        const uint64_t *out_off = m.uoff;
        if (!rc && a != 0) { zk_launch_range_rebase(st, m.uoff, a, b - a, m.poff); out_off = m.poff; }
        const zk_dec_args da{d_comp, comp_size, d_c_off, d_d_off, 0, b - a, m.uids + a, out_off, x.rng.p, pass_bytes, verify, m.fstat + a, nullptr, 0,
                             /*alone*/ !e->slot_busy[1]};
        if (!rc) rc = zk_decode_enqueue(e, x, st, da);
        if (rc == ZK_ERR_HIP && b - a > 1) {
            (void)hipStreamSynchronize(st);
            (void)hipGetLastError();
            cap = pass_bytes / 2 ? pass_bytes / 2 : 1;
            continue;
        }
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        { zk_kernel_timer t(e, ZK_K_VIEW_GATHER, st); launch_view_gather(st, v, m, dst_off, (const uint8_t *)x.rng.p, a, b); }
        if (b == nt) {      // the last pass: the statuses ride behind it, one synchronisation for both
            zk_kernel_timer t(e, ZK_K_VIEW_STATUS, st);
            launch_view_status(st, v, m, any_failed, (const uint64_t *)x.words.p + 3, status_out);
            status_queued = true;
        }
        if (status_queued) ZK_HIP(hipMemcpyAsync(hw + 2, m.words + ZKV_W_FIRST_ERR, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        rc = zk_decode_finish(e, x, st);
        if (rc <= -1000) return rc;
        if (rc) any_failed = true;
        e->ranges_frames += b - a;
        a = b;
    }
    if (!status_queued) {       // nothing to decode: validation codes only
        { zk_kernel_timer t(e, ZK_K_VIEW_STATUS, st); launch_view_status(st, v, m, false, nullptr, status_out); }
        ZK_HIP(hipMemcpyAsync(hw + 2, m.words + ZKV_W_FIRST_ERR, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipGetLastError());
        zk_profile_collect(e);
    }
    if (e->profiling) { e->kernel_ms[ZK_K_VIEW_PLAN] = plan_ms; e->kernel_ms[ZK_K_VIEW_MARK] = mark_ms; }      // (every decode pass begins a profile of its own; the plan ran before the first)
    return hw[2] != ~0ull ? -(int)(uint32_t)(hw[2] & 0xFFFFFFFFu) : 0;
}

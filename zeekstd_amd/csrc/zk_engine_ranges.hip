// zk_engine_ranges.hip -- zk_read_ranges_dev / zk_read_ranges (include/zeekstd_amd.h): byte ranges of the decompressed stream of a
// device-resident archive, many per call.  Plan on the device (zk_ranges.hip), the touched frames decoded ONCE each through
// zk_decode_enqueue into engine-owned scratch -- pass after pass over slices of the sorted frame list when they exceed the pass
// size --, the wanted bytes copied out by zk_k_range_gather, a status per range.
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_kernels.h"
#include "zk_ranges.h"

extern "C" uint64_t zk_engine_ranges_frames_decoded(const zk_engine *e) { return e ? e->ranges_frames : 0; }

namespace {
// the plan's arrays, carved out of one allocation (every piece 16-byte aligned)
struct Carver {
    uint8_t *base; size_t at = 0;
    template <typename T> T *take(size_t n) { T *p = base ? (T *)(base + at) : nullptr; at += (n * sizeof(T) + 15) & ~(size_t)15; return p; }
};
struct RangeMeta {
    uint64_t *eff, *packed, *cnt, *coff, *uoff, *poff, *words;
    ZkRangeCopy *copies;
    uint32_t *rfirst, *rlast, *cover, *slot, *ids;
    int32_t *status, *fstat;
    size_t bytes;
    RangeMeta(void *p, uint32_t count, uint32_t n_frames)
    {
        Carver c{(uint8_t *)p};
        const size_t n = count, f = n_frames;
        eff = c.take<uint64_t>(n); packed = c.take<uint64_t>(n); cnt = c.take<uint64_t>(n + 1); coff = c.take<uint64_t>(n + 1);
        uoff = c.take<uint64_t>(f + 1); poff = c.take<uint64_t>(f + 1); words = c.take<uint64_t>(4);
        copies = c.take<ZkRangeCopy>(n);
        rfirst = c.take<uint32_t>(n); rlast = c.take<uint32_t>(n); cover = c.take<uint32_t>(f + 2); slot = c.take<uint32_t>(f + 1); ids = c.take<uint32_t>(f + 1);
        status = c.take<int32_t>(n); fstat = c.take<int32_t>(f + 1);
        bytes = c.at;
    }
};
}   // namespace

extern "C" int zk_read_ranges_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_frames,
                                  const void *d_offs, const void *d_lens, const void *d_dst_off, uint32_t count, void *d_dst, uint64_t dst_cap,
                                  int verify, void *d_range_status, void *stream)
{
    if (!e || !d_d_off || (count && (!d_offs || !d_lens)) || (n_frames && (!d_comp || !d_c_off))) return ZK_ERR_ARGUMENT;
    if (count && e->slot_busy[0]) return ZK_ERR_ARGUMENT;   // a submitted batch still owns context 0: zk_decode_wait first (nothing touched, the counter included)
    e->ranges_frames = 0;
    if (count == 0) return 0;
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &x = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, x, stream);
    int rc;
    if ((rc = zk_devbuf_reserve(e, x.rng_meta, RangeMeta(nullptr, count, n_frames).bytes))) return rc;
    if ((rc = zk_devbuf_reserve(e, x.words, 16 * sizeof(uint64_t)))) return rc;
    const RangeMeta m(x.rng_meta.p, count, n_frames);
    int32_t *status = d_range_status ? (int32_t *)d_range_status : m.status;
    const ZkRangeArgs r{(const uint64_t *)d_d_off, n_frames, (const uint64_t *)d_offs, (const uint64_t *)d_lens, (const uint64_t *)d_dst_off, count, d_dst, dst_cap};
    const uint64_t *dst_off = r.dst_off ? r.dst_off : m.packed;
    uint64_t *hw = e->h_words + ZK_HW_RANGES;               // [0] frames touched, [1] their decompressed bytes, [2] first failing range

    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(m.cover, 0, ((size_t)n_frames + 2) * sizeof(uint32_t), st));
    ZK_HIP(hipMemsetAsync(m.words + 2, 0xFF, sizeof(uint64_t), st));
    { zk_kernel_timer t(e, ZK_K_RANGE_PLAN, st); zk_launch_range_plan(st, r, m.eff, m.packed, m.rfirst, m.rlast, status, m.cover, m.slot, m.ids, m.uoff, m.words); }
    ZK_HIP(hipMemcpyAsync(hw, m.words, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    float plan_ms = 0.f;
    if (e->profiling) (void)hipEventElapsedTime(&plan_ms, e->ev_start[ZK_K_RANGE_PLAN], e->ev_stop[ZK_K_RANGE_PLAN]);
    const uint32_t nt = (uint32_t)hw[0];
    const uint64_t bytes = hw[1];
    if (nt && !d_dst) return ZK_ERR_ARGUMENT;

    // Passes over slices [a, b) of the unique list, each at most `cap` decoded bytes and at least one frame.  The slices' ends come from
    // the list's prefix sums, read back only when one pass does not hold everything.
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
        const zk_dec_args da{d_comp, comp_size, d_c_off, d_d_off, 0, b - a, m.ids + a, out_off, x.rng.p, pass_bytes, verify, m.fstat + a, nullptr, 0,
                             /*alone*/ !e->slot_busy[1]};
        if (!rc) rc = zk_decode_enqueue(e, x, st, da);
        if (rc == ZK_ERR_HIP && b - a > 1) {
            (void)hipStreamSynchronize(st);
            (void)hipGetLastError();
            cap = pass_bytes / 2 ? pass_bytes / 2 : 1;
            continue;
        }
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        { zk_kernel_timer t(e, ZK_K_RANGE_PIECES, st); zk_launch_range_pieces(st, r, dst_off, m.rfirst, m.rlast, m.slot, m.ids, m.uoff, a, b, m.copies, m.cnt, m.coff); }
        { zk_kernel_timer t(e, ZK_K_RANGE_GATHER, st); zk_launch_range_gather(st, (const uint8_t *)x.rng.p, (uint8_t *)d_dst, m.copies, m.coff, count, pass_bytes); }
        if (b == nt) {      // the last pass: the statuses ride behind it, one synchronisation for both
            zk_kernel_timer t(e, ZK_K_RANGE_STATUS, st);
            zk_launch_range_status(st, r, m.rfirst, m.rlast, m.slot, m.fstat, any_failed, (const uint64_t *)x.words.p + 3, status, m.words + 2);
            status_queued = true;
        }
        if (status_queued) ZK_HIP(hipMemcpyAsync(hw + 2, m.words + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        rc = zk_decode_finish(e, x, st);
        if (rc <= -1000) return rc;
        if (rc) any_failed = true;
        e->ranges_frames += b - a;
        a = b;
    }
    if (!status_queued) {       // nothing to decode: validation codes only
        { zk_kernel_timer t(e, ZK_K_RANGE_STATUS, st); zk_launch_range_status(st, r, m.rfirst, m.rlast, m.slot, m.fstat, false, nullptr, status, m.words + 2); }
        ZK_HIP(hipMemcpyAsync(hw + 2, m.words + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipGetLastError());
        zk_profile_collect(e);
    }
    if (e->profiling) e->kernel_ms[ZK_K_RANGE_PLAN] = plan_ms;      // (every decode pass begins a profile of its own; the plan ran before the first)
    return hw[2] != ~0ull ? -(int)(uint32_t)(hw[2] & 0xFFFFFFFFu) : 0;
}

// Host pointers.  The plan runs here first (the same zk_ranges.h): only the compressed bytes of touched frames are uploaded, as a
// compact archive of those frames, the ranges' offsets moved along; the bytes come back packed in one download and are dealt to
// dst + dst_off[i] by the host, so nothing between the destinations is written.
extern "C" int zk_read_ranges(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, const uint64_t *d_off, uint32_t n_frames,
                              const uint64_t *offs, const uint64_t *lens, const uint64_t *dst_off, uint32_t count, uint8_t *dst, uint64_t dst_cap,
                              int verify, int32_t *range_status)
{
    if (!e || !d_off || (count && (!offs || !lens)) || (n_frames && (!comp || !c_off))) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    const uint64_t total = d_off[n_frames];
    std::vector<int32_t> hst(count);
    std::vector<uint64_t> h_len(count), h_off(count, 0), h_dst(count);
    std::vector<uint32_t> cover((size_t)n_frames + 2, 0);
    std::vector<uint32_t> rfirst(count, ~0u);
    uint64_t packed = 0;
    for (uint32_t i = 0; i < count; i++) {
        const bool src_ok = zkr_check_src(total, offs[i], lens[i]) == ZKR_OK;
        h_dst[i] = dst_off ? dst_off[i] : packed;           // packed: a range outside the stream takes no room
        if (!dst_off && src_ok) packed += lens[i];
        hst[i] = zkr_check(total, offs[i], lens[i], dst_cap, h_dst[i]);
        h_len[i] = hst[i] == ZKR_OK ? lens[i] : 0;
        uint32_t first, last;
        if (hst[i] == ZKR_OK && zkr_span(d_off, n_frames, offs[i], lens[i], &first, &last)) { cover[first]++; cover[last + 1]--; rfirst[i] = first; }
    }
    // the compact archive: touched frames only, in order
    std::vector<uint64_t> cc(1, 0), cd(1, 0);
    std::vector<uint64_t> new_start((size_t)n_frames, 0);   // where a touched frame starts in the compact stream
    struct Run { uint64_t lo, hi, at; };
    std::vector<Run> runs;
    uint32_t cv = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        cv += cover[f];
        if (cv == 0 || d_off[f + 1] == d_off[f]) continue;
        if (c_off[f + 1] < c_off[f] || c_off[f + 1] > comp_size) return -(int)ZK_E_SRC_SIZE_WRONG;
        new_start[f] = cd.back();
        if (!runs.empty() && runs.back().hi == c_off[f]) runs.back().hi = c_off[f + 1];
        else runs.push_back(Run{c_off[f], c_off[f + 1], cc.back()});
        cc.push_back(cc.back() + (c_off[f + 1] - c_off[f]));
        cd.push_back(cd.back() + (d_off[f + 1] - d_off[f]));
    }
    const uint32_t m = (uint32_t)(cc.size() - 1);
    uint64_t out_bytes = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (rfirst[i] != ~0u) h_off[i] = new_start[rfirst[i]] + (offs[i] - d_off[rfirst[i]]);
        out_bytes += h_len[i];
    }
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;            // refused before the staging: its uploads ride on context 0's queue, behind the batch
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    int rc;
    const size_t tab = ((size_t)m + 1) * 8, per = (size_t)count * 8;
    if ((rc = zk_devbuf_reserve(e, e->st_comp, (size_t)cc.back() + 64))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->st_off, 2 * tab + 2 * per + (size_t)count * 4 + 64))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->st_dst, (size_t)out_bytes + 64))) return rc;
    uint8_t *d_comp = (uint8_t *)e->st_comp.p;
    uint64_t *d_cc = (uint64_t *)e->st_off.p, *d_cd = d_cc + m + 1, *d_o = d_cd + m + 1, *d_l = d_o + count;
    int32_t *d_st = (int32_t *)(d_l + count);
    ZK_HIP(hipMemsetAsync(d_comp + cc.back(), 0, 64, st));          // readable padding behind the last frame
    for (const Run &u : runs) ZK_HIP(hipMemcpyAsync(d_comp + u.at, comp + u.lo, u.hi - u.lo, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_cc, cc.data(), tab, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_cd, cd.data(), tab, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_o, h_off.data(), per, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_l, h_len.data(), per, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));                               // (the vectors above are pageable)
    rc = zk_read_ranges_dev(e, d_comp, cc.back(), d_cc, d_cd, m, d_o, d_l, nullptr, count, e->st_dst.p, out_bytes, verify, d_st, nullptr);
    if (rc <= -1000 && rc != ZK_ERR_OFFSET_OUT_OF_RANGE) return rc;
    std::vector<int32_t> dev_st(count);
    std::vector<uint8_t> out((size_t)out_bytes);
    ZK_HIP(hipMemcpy(dev_st.data(), d_st, (size_t)count * 4, hipMemcpyDeviceToHost));
    if (out_bytes) ZK_HIP(hipMemcpy(out.data(), e->st_dst.p, (size_t)out_bytes, hipMemcpyDeviceToHost));
    int ret = 0;
    uint64_t at = 0;
    for (uint32_t i = 0; i < count; i++) {
        const int32_t s = hst[i] ? hst[i] : dev_st[i];
        if (h_len[i]) { memcpy(dst + h_dst[i], out.data() + at, (size_t)h_len[i]); at += h_len[i]; }
        if (range_status) range_status[i] = s;
        if (s && !ret) ret = s;
    }
    return ret;
}

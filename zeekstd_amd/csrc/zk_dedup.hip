// zk_dedup.hip -- zk_dedup_frames[_dev], zk_encode_dedup[_dev]: which frames of a list are byte-identical, and each distinct frame encoded
// once (include/zeekstd_amd.h; the kernels and the scheme: zk_dedup.h).
//   the map      the offsets come to the host and are checked (one wait, as in zk_encode_frame_list_dev); zk_k_dedup_hash over every frame; then ROUNDS
//                over the open frames: the table cleared, zk_k_dedup_insert, zk_k_dedup_verify, the two counters read back (a wait), and when
//                frames longer than a lane compares are to be compared zk_k_dedup_verify_long + zk_k_dedup_settle_long and the counter of
//                open frames once more (a wait).  With all 64 key bits a second round takes two different frames of one length and one hash.  Then flags, zk_k_scan64,
//                zk_k_dedup_emit, and n_unique read back (a wait)
//   the encode   the indices of the unique frames come to the host; they are cut into slices of whole frames of at most
//                ZK_CHOICE_DEDUP_SLICE_KIB, each gathered back to back into engine scratch (zk_k_dedup_gather) and handed to
//                zk_encode_frame_list_dev with its own offsets, destination after destination.  A list without duplicates is handed over as
//                it is.  A destination below the bound of the unique frames with more than one slice: the slices are encoded into scratch
//                first, so that -70 leaves the destination untouched
// All scratch is the encoder's (zk_engine::Enc::dd*): a submitted decode batch is not touched.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_dedup.h"

constexpr uint64_t ZKD_SLICE_BYTES = 1ull << 30;         // ZK_CHOICE_DEDUP_SLICE_KIB's default

namespace {
struct ZkDedupScratch { uint64_t *hash, *flags, *pos; uint32_t *ref, *slot, *list[2], *longl, *differ, *uniq, *ids, *cnt, *table; };
constexpr int ZKD_TIMED[] = {ZK_K_DEDUP_HASH, ZK_K_DEDUP_INSERT, ZK_K_DEDUP_VERIFY, ZK_K_DEDUP_VERIFY_LONG, ZK_K_DEDUP_COMPACT, ZK_K_DEDUP_GATHER};
// a kernel's pair of events holds one launch: after a wait the times of the launches since the last one are added up here
struct ZkDedupTimes {
    float ms[ZK_NKERNELS] = {};
    void collect(zk_engine *e)
    {
        if (!e->profiling) return;
        zk_profile_collect(e);
        for (int k : ZKD_TIMED) { ms[k] += e->kernel_ms[k]; e->kernel_ms[k] = 0.f; e->ev_used[k] = false; }
    }
    void publish(zk_engine *e) const { if (e->profiling) for (int k : ZKD_TIMED) e->kernel_ms[k] = ms[k]; }
};

// the caller's offsets to the engine's pinned memory, checked: *h_off (count + 1 entries; room for count indices behind them).  One wait
int zk_dedup_offsets(zk_engine *e, hipStream_t st, const void *d_off, uint32_t count, uint64_t **h_off, uint64_t *max_frame)
{
    int rc;
    if ((rc = zk_pin_reserve(e, e->enc.pin_dd, e->enc.pin_dd_cap, ((size_t)count + 1) * 8 + (size_t)count * 4))) return rc;
    uint64_t *off = (uint64_t *)e->enc.pin_dd;
    ZK_HIP(hipMemcpyAsync(off, d_off, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    if ((rc = zk_enc_list_check(off, count, max_frame))) return rc;
    *h_off = off;
    return 0;
}

// The map of `count` > 0 checked frames; src: the byte off[0] names.  ref, uniq and ids are left in the engine's scratch (S), *n_unique is set.
// The stream is synchronised.
int zk_dedup_core(zk_engine *e, hipStream_t st, const uint8_t *src, const uint64_t *d_off, uint64_t base, uint32_t count, uint64_t max_frame,
                  ZkDedupScratch &S, ZkDedupTimes &T, uint32_t *n_unique)
{
    const ZkDedupLayout L = zkd_layout(count);
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.dd, L.end + 64))) return rc;
    uint8_t *b = (uint8_t *)e->enc.dd.p;
    S = ZkDedupScratch{(uint64_t *)(b + L.hash), (uint64_t *)(b + L.flags), (uint64_t *)(b + L.pos), (uint32_t *)(b + L.ref), (uint32_t *)(b + L.slot),
                       {(uint32_t *)(b + L.list[0]), (uint32_t *)(b + L.list[1])}, (uint32_t *)(b + L.longl), (uint32_t *)(b + L.differ),
                       (uint32_t *)(b + L.uniq), (uint32_t *)(b + L.ids), (uint32_t *)(b + L.cnt), (uint32_t *)(b + L.table)};
    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(S.hash, 0, (size_t)count * 8, st));
    {
        zk_kernel_timer t(e, ZK_K_DEDUP_HASH, st);
        hipLaunchKernelGGL(zk_k_dedup_hash, dim3(count < ZKD_GRID_MAX ? count : ZKD_GRID_MAX, zkd_pieces(max_frame)), dim3(ZKD_THREADS), 0, st, src, d_off, base, count, (uint32_t *)S.hash);
    }
    ZK_HIP(hipMemsetAsync(S.ref, 0xFF, (size_t)count * 4, st));
    const ZkDedupIn in{src, d_off, base, S.hash, e->enc.dedup_key_bits};
    const uint32_t *list = nullptr;
    uint32_t nopen = count, w = 0;
    while (nopen) {
        const uint32_t slots = zkd_slots(nopen), blocks = zkd_blocks(nopen);
        const ZkDedupRound r{list, nopen, slots - 1};
        uint32_t *next = S.list[w];
        ZK_HIP(hipMemsetAsync(S.table, 0xFF, (size_t)slots * 4, st));
        ZK_HIP(hipMemsetAsync(S.cnt, 0, ZKD_CNT_WORDS * 4, st));
        { zk_kernel_timer t(e, ZK_K_DEDUP_INSERT, st); hipLaunchKernelGGL(zk_k_dedup_insert, dim3(blocks), dim3(ZKD_THREADS), 0, st, in, r, S.table, S.slot); }
        // (a launch of its own: the table's words, written by atomics of every XCD, are read with plain loads from here on)
        { zk_kernel_timer t(e, ZK_K_DEDUP_VERIFY, st); hipLaunchKernelGGL(zk_k_dedup_verify, dim3(blocks), dim3(ZKD_THREADS), 0, st, in, r, S.table, S.slot, S.ref, next, S.longl, S.differ, S.cnt); }
        uint32_t cnt[2] = {0, 0};
        ZK_HIP(hipMemcpyAsync(cnt, S.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        T.collect(e);
        if (const uint32_t nlong = cnt[ZKD_CNT_LONG]) {
            const dim3 grid(nlong < ZKD_GRID_MAX ? nlong : ZKD_GRID_MAX, zkd_pieces(max_frame));
            {
                zk_kernel_timer t(e, ZK_K_DEDUP_VERIFY_LONG, st);
                hipLaunchKernelGGL(zk_k_dedup_verify_long, grid, dim3(ZKD_THREADS), 0, st, in, S.table, S.slot, S.longl, nlong, S.differ);
                hipLaunchKernelGGL(zk_k_dedup_settle_long, dim3(zkd_blocks(nlong)), dim3(ZKD_THREADS), 0, st, S.table, S.slot, S.longl, nlong, S.differ, S.ref, next, S.cnt);
            }
            ZK_HIP(hipMemcpyAsync(cnt, S.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
            ZK_HIP(hipStreamSynchronize(st));
            T.collect(e);
        }
        ZK_HIP(hipGetLastError());
        if (cnt[ZKD_CNT_NEXT] >= nopen) return -(int)ZK_E_GENERIC;               // (every round settles its leaders: cannot happen)
        nopen = cnt[ZKD_CNT_NEXT]; list = next; w ^= 1;
    }
    {
        zk_kernel_timer t(e, ZK_K_DEDUP_COMPACT, st);
        hipLaunchKernelGGL(zk_k_dedup_flags, dim3(zkd_blocks((uint64_t)count + 1)), dim3(ZKD_THREADS), 0, st, S.ref, count, S.flags);
        zk_launch_scan64(st, S.flags, count + 1, S.pos);
        hipLaunchKernelGGL(zk_k_dedup_emit, dim3(zkd_blocks(count)), dim3(ZKD_THREADS), 0, st, S.ref, count, S.pos, S.uniq, S.ids);
    }
    uint64_t nu = 0;
    ZK_HIP(hipMemcpyAsync(&nu, S.pos + count, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    T.collect(e);
    T.publish(e);
    *n_unique = (uint32_t)nu;
    return 0;
}

// what both device entry points begin with: the offsets to the host and checked, then the map
int zk_dedup_map_dev(zk_engine *e, hipStream_t st, const void *d_src, const void *d_off, uint32_t count, ZkDedupScratch &S, ZkDedupTimes &T,
                     uint64_t **h_off, uint64_t *max_frame, uint32_t *n_unique)
{
    int rc;
    if ((rc = zk_dedup_offsets(e, st, d_off, count, h_off, max_frame))) return rc;
    const uint64_t *off = *h_off;
    if (off[count] != off[0] && !d_src) return ZK_ERR_ARGUMENT;
    return zk_dedup_core(e, st, d_src ? (const uint8_t *)d_src + off[0] : nullptr, (const uint64_t *)d_off, off[0], count, *max_frame, S, T, n_unique);
}
}  // namespace

extern "C" int zk_dedup_frames_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, void *d_ref, void *d_ids, void *d_uniq,
                                   uint32_t *n_unique, void *stream)
{
    if (!e || !n_unique) return ZK_ERR_ARGUMENT;
    *n_unique = 0;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!d_off) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    ZkDedupScratch S;
    ZkDedupTimes T;
    uint64_t *off = nullptr, max_frame = 0;
    uint32_t nu = 0;
    if (const int rc = zk_dedup_map_dev(e, st, d_src, d_off, count, S, T, &off, &max_frame, &nu)) return rc;
    if (d_ref) ZK_HIP(hipMemcpyAsync(d_ref, S.ref, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    if (d_ids) ZK_HIP(hipMemcpyAsync(d_ids, S.ids, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    if (d_uniq) ZK_HIP(hipMemcpyAsync(d_uniq, S.uniq, (size_t)nu * 4, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    *n_unique = nu;
    return 0;
}

namespace {
// the host entry points' upload: the source whole, its offsets -- counted from off[0] -- behind it (16-byte aligned) -> where they lie on the
// device.  The stream is synchronised
int zk_dedup_upload(zk_engine *e, hipStream_t st, const uint8_t *src, const uint64_t *off, uint32_t count, const uint8_t **d_src, const uint64_t **d_off)
{
    const uint64_t n = off[count] - off[0];
    const size_t off_at = ((size_t)n + 15) & ~(size_t)15;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.dd_up, off_at + ((size_t)count + 1) * 8 + 64))) return rc;
    uint8_t *b = (uint8_t *)e->enc.dd_up.p;
    if (n) ZK_HIP(hipMemcpyAsync(b, src + off[0], (size_t)n, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> rel((size_t)count + 1);
    for (uint32_t i = 0; i <= count; i++) rel[i] = off[i] - off[0];
    ZK_HIP(hipMemcpyAsync(b + off_at, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    *d_src = b; *d_off = (const uint64_t *)(b + off_at);
    return 0;
}
}  // namespace

extern "C" int zk_dedup_frames(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count, uint32_t *ref, uint32_t *ids, uint32_t *uniq,
                               uint32_t *n_unique)
{
    if (!e || !n_unique) return ZK_ERR_ARGUMENT;
    *n_unique = 0;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!off) return ZK_ERR_ARGUMENT;
    uint64_t max_frame = 0;
    int rc;
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    if (off[count] != off[0] && !src) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const uint8_t *d_src = nullptr;
    const uint64_t *d_off = nullptr;
    if ((rc = zk_dedup_upload(e, st, src, off, count, &d_src, &d_off))) return rc;
    ZkDedupScratch S;
    ZkDedupTimes T;
    uint32_t nu = 0;
    if ((rc = zk_dedup_core(e, st, d_src, d_off, 0, count, max_frame, S, T, &nu))) return rc;
    if (ref) ZK_HIP(hipMemcpyAsync(ref, S.ref, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    if (ids) ZK_HIP(hipMemcpyAsync(ids, S.ids, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    if (uniq) ZK_HIP(hipMemcpyAsync(uniq, S.uniq, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    *n_unique = nu;
    return 0;
}

namespace {
// The encode behind the map: frame i is src[d_off[i] - base ...], off a host copy of the offsets (only their differences are used), S.uniq the
// unique frames.
int zk_dedup_encode(zk_engine *e, hipStream_t st, const uint8_t *src, const uint64_t *d_off, uint64_t base, const uint64_t *off, uint32_t count, uint32_t nu, uint64_t max_frame,
                    const ZkDedupScratch &S, ZkDedupTimes &T, int level, int checksum, const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict,
                    uint8_t *d_dst, uint64_t dst_cap, uint32_t *d_c_sizes, uint32_t *d_d_sizes, uint64_t *written)
{
    int rc;
    if (nu == count) {
        // no duplicate: the frames lie back to back where they are (the list encoder addresses frame i at its source + d_off[i])
        rc = zk_encode_frame_list_dev(e, src ? src - base : nullptr, d_off, count, level, checksum, d_prefix, prefix_len, cdict, d_dst, dst_cap, d_c_sizes, d_d_sizes, written, st);
        T.publish(e);
        return rc;
    }
    uint32_t *uniq = (uint32_t *)(e->enc.pin_dd + ((size_t)count + 1) * 8);          // (zk_dedup_offsets left the room)
    ZK_HIP(hipMemcpyAsync(uniq, S.uniq, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    // slices of whole frames: as many as fit into slice_max bytes, one at least
    const uint64_t slice_max = e->enc.dedup_slice_bytes ? e->enc.dedup_slice_bytes : ZKD_SLICE_BYTES;
    const auto len_of = [&](uint32_t k) { return off[uniq[k] + 1] - off[uniq[k]]; };
    std::vector<uint32_t> cut{0};
    uint64_t ubytes = 0, largest = 0;
    while (cut.back() < nu) {
        const uint32_t k0 = cut.back(), k1 = zkd_slice_end(k0, nu, slice_max, len_of);
        uint64_t in_slice = 0;
        for (uint32_t k = k0; k < k1; k++) in_slice += len_of(k);
        ubytes += in_slice;
        if (in_slice > largest) largest = in_slice;
        cut.push_back(k1);
    }
    const size_t nslices = cut.size() - 1;
    uint32_t most = 0;
    for (size_t s = 0; s < nslices; s++) if (cut[s + 1] - cut[s] > most) most = cut[s + 1] - cut[s];
    if ((rc = zk_devbuf_reserve(e, e->enc.dd_src, (size_t)largest + 64))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.dd_off, ((size_t)most + 1) * 8))) return rc;
    uint8_t *g_src = (uint8_t *)e->enc.dd_src.p;
    uint64_t *g_off = (uint64_t *)e->enc.dd_off.p;
    std::vector<uint64_t> h_goff((size_t)most + 1);
    const int dict = cdict != nullptr;
    const bool tight = dst_cap < zk_compress_bound_list(ubytes, nu, dict);
    // pass 0 (a tight destination and several slices only): into scratch, for the total; pass 1: into the destination
    for (int pass = tight && nslices > 1 ? 0 : 1; pass < 2; pass++) {
        uint64_t total = 0;
        for (size_t s = 0; s < nslices; s++) {
            const uint32_t k0 = cut[s], m = cut[s + 1] - k0;
            h_goff[0] = 0;
            for (uint32_t k = 0; k < m; k++) h_goff[k + 1] = h_goff[k] + (off[uniq[k0 + k] + 1] - off[uniq[k0 + k]]);
            ZK_HIP(hipMemcpyAsync(g_off, h_goff.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, st));
            {
                zk_kernel_timer t(e, ZK_K_DEDUP_GATHER, st);
                hipLaunchKernelGGL(zk_k_dedup_gather, dim3(m < ZKD_GRID_MAX ? m : ZKD_GRID_MAX, zkd_pieces(max_frame)), dim3(ZKD_THREADS), 0, st,
                                   src, d_off, base, S.uniq + k0, m, g_off, g_src);
            }
            // (the pageable h_goff is reused: the list encoder's first wait, for its offsets, is behind the copy above)
            uint64_t wr = 0;
            if (pass == 0) {
                const uint64_t bound = zk_compress_bound_list(h_goff[m], m, dict);
                if ((rc = zk_devbuf_reserve(e, e->enc.dd_dry, (size_t)bound + 64))) return rc;
                rc = zk_encode_frame_list_dev(e, g_src, g_off, m, level, checksum, d_prefix, prefix_len, cdict, e->enc.dd_dry.p, bound, nullptr, nullptr, &wr, st);
            } else
                rc = zk_encode_frame_list_dev(e, g_src, g_off, m, level, checksum, d_prefix, prefix_len, cdict, d_dst + total, dst_cap - total,
                                              d_c_sizes ? d_c_sizes + k0 : nullptr, d_d_sizes ? d_d_sizes + k0 : nullptr, &wr, st);
            if (rc) return rc;
            // (the list encoder began a profile of its own: the gather's time is taken before it is lost)
            if (e->profiling) { float ms = 0.f; if (hipEventElapsedTime(&ms, e->ev_start[ZK_K_DEDUP_GATHER], e->ev_stop[ZK_K_DEDUP_GATHER]) == hipSuccess) T.ms[ZK_K_DEDUP_GATHER] += ms; }
            total += wr;
        }
        if (pass == 0 && total > dst_cap) return -(int)ZK_E_DST_TOO_SMALL;
        if (pass == 1 && written) *written = total;
    }
    T.publish(e);
    return 0;
}
}  // namespace

extern "C" int zk_encode_dedup_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, int level, int checksum,
                                   const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict, void *d_dst, uint64_t dst_cap,
                                   void *d_ids, void *d_uniq, void *d_c_sizes, void *d_d_sizes, uint32_t *n_unique, uint64_t *written, void *stream)
{
    if (!e || !n_unique || (cdict && cdict->e != e) || (cdict && d_prefix && prefix_len)) return ZK_ERR_ARGUMENT;
    *n_unique = 0;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) { if (written) *written = 0; return 0; }
    if (!d_off || !d_dst) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    ZkDedupScratch S;
    ZkDedupTimes T;
    uint64_t *off = nullptr, max_frame = 0;
    uint32_t nu = 0;
    int rc;
    if ((rc = zk_dedup_map_dev(e, st, d_src, d_off, count, S, T, &off, &max_frame, &nu))) return rc;
    // the encode first: -70 leaves the caller's arrays as they are, like the destination
    uint64_t wr = 0;
    if ((rc = zk_dedup_encode(e, st, d_src ? (const uint8_t *)d_src + off[0] : nullptr, (const uint64_t *)d_off, off[0], off, count, nu, max_frame, S, T, level, checksum,
                              d_prefix, prefix_len, cdict, (uint8_t *)d_dst, dst_cap, (uint32_t *)d_c_sizes, (uint32_t *)d_d_sizes, &wr))) return rc;
    if (d_ids) ZK_HIP(hipMemcpyAsync(d_ids, S.ids, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    if (d_uniq) ZK_HIP(hipMemcpyAsync(d_uniq, S.uniq, (size_t)nu * 4, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    *n_unique = nu;
    if (written) *written = wr;
    return 0;
}

extern "C" int zk_encode_dedup(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count, int level, int checksum,
                               const uint8_t *prefix, uint64_t prefix_len, const zk_cdict *cdict, uint8_t *dst, uint64_t dst_cap,
                               uint32_t *ids, uint32_t *uniq, uint32_t *c_sizes, uint32_t *d_sizes, uint32_t *n_unique, uint64_t *written)
{
    if (!e || !n_unique || (cdict && cdict->e != e) || (cdict && prefix && prefix_len)) return ZK_ERR_ARGUMENT;
    *n_unique = 0;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) { if (written) *written = 0; return 0; }
    if (!off || !dst) return ZK_ERR_ARGUMENT;
    uint64_t max_frame = 0;
    int rc;
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    const uint64_t n = off[count] - off[0];
    if (n && !src) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // the prefix as zk_encode_frame_list stages it: the tail the matcher can reach
    const void *d_prefix = nullptr;
    uint64_t tail = 0;
    if (!cdict) {
        tail = prefix ? zke_ldm_usable(prefix_len) : 0;
        if ((rc = zk_engine_stage_prefix(e, nullptr, tail ? prefix + (prefix_len - tail) : nullptr, tail, true, &d_prefix))) return rc;
    }
    const uint8_t *d_src = nullptr;
    const uint64_t *d_off = nullptr;
    if ((rc = zk_dedup_upload(e, st, src, off, count, &d_src, &d_off))) return rc;
    // the destination and the two size arrays on the device: what the caller's can hold, the bound at most
    const uint64_t bound = zk_compress_bound_list(n, count, cdict != nullptr), cap = dst_cap < bound ? dst_cap : bound;
    const size_t sizes_at = ((size_t)cap + 15) & ~(size_t)15;
    if ((rc = zk_devbuf_reserve(e, e->enc.dd_out, sizes_at + (size_t)count * 8 + 64))) return rc;
    uint8_t *d_dst = (uint8_t *)e->enc.dd_out.p;
    uint32_t *d_cs = (uint32_t *)(d_dst + sizes_at), *d_ds = d_cs + count;
    ZkDedupScratch S;
    ZkDedupTimes T;
    uint32_t nu = 0;
    uint64_t wr = 0;
    // (the host copy of the offsets the encode reads is the caller's own; the room for the indices behind a copy is the engine's)
    if ((rc = zk_pin_reserve(e, e->enc.pin_dd, e->enc.pin_dd_cap, ((size_t)count + 1) * 8 + (size_t)count * 4))) return rc;
    if ((rc = zk_dedup_core(e, st, d_src, d_off, 0, count, max_frame, S, T, &nu))) return rc;
    if ((rc = zk_dedup_encode(e, st, d_src, d_off, 0, off, count, nu, max_frame, S, T, level, checksum, tail ? d_prefix : nullptr, tail, cdict, d_dst, cap, d_cs, d_ds, &wr))) return rc;
    if (wr) ZK_HIP(hipMemcpyAsync(dst, d_dst, (size_t)wr, hipMemcpyDeviceToHost, st));
    if (c_sizes) ZK_HIP(hipMemcpyAsync(c_sizes, d_cs, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    if (d_sizes) ZK_HIP(hipMemcpyAsync(d_sizes, d_ds, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    if (ids) ZK_HIP(hipMemcpyAsync(ids, S.ids, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    if (uniq) ZK_HIP(hipMemcpyAsync(uniq, S.uniq, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    *n_unique = nu;
    if (written) *written = wr;
    return 0;
}

// zk_dedup_against_dev and its siblings build on the map and the encode above and on the kernels of zk_dedup.h, which one translation unit
// only can define: they are compiled here
#include "zk_dedup_index.hip"

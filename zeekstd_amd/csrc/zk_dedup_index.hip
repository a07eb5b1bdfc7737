// zk_dedup_index.hip -- zk_dedup_index_*, zk_frame_keys[_dev], zk_dedup_against_dev, zk_encode_dedup_against_dev: a frame list deduplicated
// against an archive that already exists (include/zeekstd_amd.h; the kernels and the scheme: zk_dedup_index.h).
//   the index    keys, lengths and the table in device memory of its own; the number of frames m and the sizes on the host.  Every call that
//                changes it synchronises its stream before it returns, so m and the device arrays agree between calls
//   the map      zk_dedup_map_dev (offsets checked, hashes, ref / uniq / ids of the list alone); the unique frames'
//                indices come to the host; then ROUNDS: zk_k_dxi_lookup over the open unique frames, the candidates to the host (a wait), the
//                (frame, candidate) pairs and their places made there and uploaded, and pass after pass of at most ZK_CHOICE_DEDUP_PASS_KIB
//                decoded bytes: zk_decode_enqueue on context 0 with the pairs' archive ids (the route of zk_decode_frame_list_dev and
//                zk_read_ranges_dev, checksums verified, the engine's dictionary applied) into dctx[0].rng, zk_k_dxi_compare behind it on the
//                same queue, zk_decode_finish (a wait).  The differ words come to the host (a wait), which opens the next round.  Then
//                zk_k_dxi_flags, zk_k_scan64, zk_k_dxi_emit and n_fresh read back (a wait).  One round unless an archive frame shares key
//                and length with a frame it differs from.
//   the encode   zk_dedup_encode over the fresh frames in place of the unique ones; on success their keys (the hashes the map made) and
//                lengths are appended to the index: nothing is decoded for that.
// The lookup's scratch is zk_engine::Enc::dx; the decoded candidates take context 0, so a batch submitted there refuses the call.
// Included by zk_dedup.hip (behind its own functions, which this file calls): zk_dedup.h defines its kernels, so one translation unit holds both.
#include "zk_kernels.h"
#include "zk_dedup_index.h"

struct zk_dedup_index {
    zk_engine *e = nullptr;
    uint32_t bits = 0;                      // ZK_CHOICE_DEDUP_KEY_BITS when it was made
    uint32_t m = 0, cap = 0;                // frames; room in keys / lens
    uint32_t slots = 0, table_cap = 0;      // slots in use (zkx_slots of the frames it was last built for); room in table
    uint64_t *keys = nullptr;
    uint32_t *lens = nullptr, *table = nullptr;
};

namespace {
constexpr int ZKX_OWN[] = {ZK_K_DXI_INSERT, ZK_K_DXI_LOOKUP, ZK_K_DXI_COMPARE, ZK_K_DXI_EMIT};
// a kernel's pair of events holds one launch, and every decode pass begins a profile of its own: after each wait the times are added up here
struct ZkDxTimes {
    float ms[ZK_NKERNELS] = {};
    void take(zk_engine *e)
    {
        if (!e->profiling) return;
        zk_profile_collect(e);
        for (int k = 0; k < ZK_NKERNELS; k++) { ms[k] += e->kernel_ms[k]; e->kernel_ms[k] = 0.f; e->ev_used[k] = false; }
    }
    void publish(zk_engine *e, bool all) const
    {
        if (!e->profiling) return;
        if (all) { for (int k = 0; k < ZK_NKERNELS; k++) e->kernel_ms[k] = ms[k]; return; }
        for (int k = 0; k < ZK_K_ENC_MATCH; k++) e->kernel_ms[k] = ms[k];       // (behind an encode, which began a profile of its own: the decode passes' and ours)
        for (int k : ZKX_OWN) e->kernel_ms[k] = ms[k];
    }
};

// room for `total` frames: keys / lens (the first m kept) and a table buffer for zkx_slots(total) (its slots in use kept).  The stream is
// synchronised when anything moved
int zkx_reserve(zk_dedup_index *x, hipStream_t st, uint32_t total)
{
    zk_engine *e = x->e;
    if (total > x->cap) {
        const uint64_t want64 = (uint64_t)total + total / 2 + 1024;
        const uint32_t want = want64 > ZK_SEEKABLE_MAX_FRAMES ? ZK_SEEKABLE_MAX_FRAMES : (uint32_t)want64;
        uint64_t *keys = nullptr;
        uint32_t *lens = nullptr;
        ZK_HIP(hipMalloc((void **)&keys, (size_t)want * 8));
        if (hipMalloc((void **)&lens, (size_t)want * 4) != hipSuccess) { (void)hipFree(keys); e->last_err = "hipMalloc: the index's lengths"; return ZK_ERR_HIP; }
        if (x->m) {
            (void)hipMemcpyAsync(keys, x->keys, (size_t)x->m * 8, hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(lens, x->lens, (size_t)x->m * 4, hipMemcpyDeviceToDevice, st);
        }
        if (hipStreamSynchronize(st) != hipSuccess) { (void)hipFree(keys); (void)hipFree(lens); e->last_err = "the index's arrays could not be moved"; return ZK_ERR_HIP; }
        (void)hipFree(x->keys); (void)hipFree(x->lens);
        x->keys = keys; x->lens = lens; x->cap = want;
    }
    const uint32_t slots = zkx_slots(total);
    if (slots > x->table_cap) {
        uint32_t *table = nullptr;
        ZK_HIP(hipMalloc((void **)&table, (size_t)slots * 4));
        if (x->slots) (void)hipMemcpyAsync(table, x->table, (size_t)x->slots * 4, hipMemcpyDeviceToDevice, st);
        if (hipStreamSynchronize(st) != hipSuccess) { (void)hipFree(table); e->last_err = "the index's table could not be moved"; return ZK_ERR_HIP; }
        (void)hipFree(x->table);
        x->table = table; x->table_cap = slots;
    }
    return 0;
}
// the table made anew from the keys of `frames` frames
int zkx_rebuild(zk_dedup_index *x, hipStream_t st, uint32_t frames)
{
    zk_engine *e = x->e;
    x->slots = zkx_slots(frames);
    ZK_HIP(hipMemsetAsync(x->table, 0xFF, (size_t)x->slots * 4, st));
    if (frames) {
        zk_kernel_timer t(e, ZK_K_DXI_INSERT, st);
        hipLaunchKernelGGL(zk_k_dxi_insert, dim3(zkd_blocks(frames)), dim3(ZKD_THREADS), 0, st, x->keys, x->lens, x->bits, 0u, frames, x->table, x->slots - 1);
    }
    return 0;
}
// frames m .. m + n - 1, whose keys and lengths are in place (zkx_reserve came first): into the table, or the table rebuilt at twice the size.
// The stream is synchronised
int zkx_commit(zk_dedup_index *x, hipStream_t st, uint32_t n)
{
    zk_engine *e = x->e;
    const uint32_t total = x->m + n;
    if (zkx_slots(total) > x->slots) { if (const int rc = zkx_rebuild(x, st, total)) return rc; }
    else if (n) {
        zk_kernel_timer t(e, ZK_K_DXI_INSERT, st);
        hipLaunchKernelGGL(zk_k_dxi_insert, dim3(zkd_blocks(n)), dim3(ZKD_THREADS), 0, st, x->keys, x->lens, x->bits, x->m, n, x->table, x->slots - 1);
    }
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    x->m = total;
    return 0;
}
int zkx_add_check(const zk_dedup_index *x, uint32_t count)
{
    if (!x) return ZK_ERR_ARGUMENT;
    if ((uint64_t)x->m + count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    return 0;
}
void zkx_hash_launch(hipStream_t st, const uint8_t *src, const uint64_t *d_off, uint64_t base, uint32_t count, uint64_t max_frame, void *d_keys)
{
    hipLaunchKernelGGL(zk_k_dedup_hash, dim3(count < ZKD_GRID_MAX ? count : ZKD_GRID_MAX, zkd_pieces(max_frame)), dim3(ZKD_THREADS), 0, st, src, d_off, base, count,
                       (uint32_t *)d_keys);
}
}  // namespace

extern "C" zk_dedup_index *zk_dedup_index_create(zk_engine *e)
{
    if (!e || hipSetDevice(e->device) != hipSuccess) return nullptr;
    zk_dedup_index *x = new zk_dedup_index();
    x->e = e;
    x->bits = e->enc.dedup_key_bits;
    if (zkx_reserve(x, e->stream, 0) || zkx_rebuild(x, e->stream, 0) || hipStreamSynchronize(e->stream) != hipSuccess) { zk_dedup_index_free(x); return nullptr; }
    return x;
}
extern "C" void zk_dedup_index_free(zk_dedup_index *x)
{
    if (!x) return;
    (void)hipSetDevice(x->e->device);
    (void)hipFree(x->keys); (void)hipFree(x->lens); (void)hipFree(x->table);
    delete x;
}
extern "C" uint32_t zk_dedup_index_count(const zk_dedup_index *x) { return x ? x->m : 0; }

extern "C" int zk_dedup_index_add_dev(zk_dedup_index *x, const void *d_keys, const void *d_d_sizes, uint32_t count, void *stream)
{
    if (const int rc = zkx_add_check(x, count)) return rc;
    if (count == 0) return 0;
    if (!d_keys || !d_d_sizes) return ZK_ERR_ARGUMENT;
    zk_engine *e = x->e;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    if (const int rc = zkx_reserve(x, st, x->m + count)) return rc;
    zk_profile_begin(e);
    ZK_HIP(hipMemcpyAsync(x->keys + x->m, d_keys, (size_t)count * 8, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipMemcpyAsync(x->lens + x->m, d_d_sizes, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    return zkx_commit(x, st, count);
}
extern "C" int zk_dedup_index_add(zk_dedup_index *x, const uint64_t *keys, const uint32_t *d_sizes, uint32_t count)
{
    if (const int rc = zkx_add_check(x, count)) return rc;
    if (count == 0) return 0;
    if (!keys || !d_sizes) return ZK_ERR_ARGUMENT;
    for (uint32_t i = 0; i < count; i++) if (d_sizes[i] > ZK_SEEKABLE_MAX_FRAME_SIZE) return ZK_ERR_ARGUMENT;
    zk_engine *e = x->e;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    if (const int rc = zkx_reserve(x, st, x->m + count)) return rc;
    zk_profile_begin(e);
    ZK_HIP(hipMemcpyAsync(x->keys + x->m, keys, (size_t)count * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(x->lens + x->m, d_sizes, (size_t)count * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));                       // (the caller's arrays are pageable)
    return zkx_commit(x, st, count);
}
extern "C" int zk_dedup_index_export(const zk_dedup_index *x, uint32_t first, uint32_t count, uint64_t *keys_out, uint32_t *d_sizes_out)
{
    if (!x || (uint64_t)first + count > x->m) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    zk_engine *e = x->e;
    ZK_HIP(hipSetDevice(e->device));
    if (keys_out) ZK_HIP(hipMemcpy(keys_out, x->keys + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    if (d_sizes_out) ZK_HIP(hipMemcpy(d_sizes_out, x->lens + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int zk_dedup_index_truncate(zk_dedup_index *x, uint32_t count)
{
    if (!x || count > x->m) return ZK_ERR_ARGUMENT;
    zk_engine *e = x->e;
    ZK_HIP(hipSetDevice(e->device));
    ZK_HIP(hipStreamSynchronize(e->stream));
    x->m = count;
    zk_profile_begin(e);
    if (const int rc = zkx_rebuild(x, e->stream, count)) return rc;
    ZK_HIP(hipStreamSynchronize(e->stream));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    return 0;
}

extern "C" int zk_frame_keys_dev(zk_engine *e, const void *d_src, const void *d_off, uint32_t count, void *d_keys, void *stream)
{
    if (!e) return ZK_ERR_ARGUMENT;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!d_off || !d_keys || ((uintptr_t)d_keys & 7u)) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    int rc;
    if ((rc = zk_pin_reserve(e, e->enc.pin_dd, e->enc.pin_dd_cap, ((size_t)count + 1) * 8 + (size_t)count * 4))) return rc;
    uint64_t *off = (uint64_t *)e->enc.pin_dd, max_frame = 0;
    ZK_HIP(hipMemcpyAsync(off, d_off, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    if (off[count] != off[0] && !d_src) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipMemsetAsync(d_keys, 0, (size_t)count * 8, st));
    zkx_hash_launch(st, d_src ? (const uint8_t *)d_src + off[0] : nullptr, (const uint64_t *)d_off, off[0], count, max_frame, d_keys);
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return 0;
}
extern "C" int zk_frame_keys(zk_engine *e, const uint8_t *src, const uint64_t *off, uint32_t count, uint64_t *keys)
{
    if (!e) return ZK_ERR_ARGUMENT;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!off || !keys) return ZK_ERR_ARGUMENT;
    uint64_t max_frame = 0;
    int rc;
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    const uint64_t n = off[count] - off[0];
    if (n && !src) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // the source whole, its offsets -- counted from off[0] -- and the keys behind it
    const size_t off_at = ((size_t)n + 15) & ~(size_t)15, keys_at = off_at + ((((size_t)count + 1) * 8 + 15) & ~(size_t)15);
    if ((rc = zk_devbuf_reserve(e, e->enc.dd_up, keys_at + (size_t)count * 8 + 64))) return rc;
    uint8_t *b = (uint8_t *)e->enc.dd_up.p;
    if (n) ZK_HIP(hipMemcpyAsync(b, src + off[0], (size_t)n, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> rel((size_t)count + 1);
    for (uint32_t i = 0; i <= count; i++) rel[i] = off[i] - off[0];
    ZK_HIP(hipMemcpyAsync(b + off_at, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemsetAsync(b + keys_at, 0, (size_t)count * 8, st));
    zkx_hash_launch(st, b, (const uint64_t *)(b + off_at), 0, count, max_frame, b + keys_at);
    ZK_HIP(hipMemcpyAsync(keys, b + keys_at, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return 0;
}

extern "C" int zk_dedup_index_add_archive_dev(zk_dedup_index *x, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                                              uint32_t n_frames, void *stream)
{
    if (!x || n_frames < x->m) return ZK_ERR_ARGUMENT;
    zk_engine *e = x->e;
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;            // a submitted batch still owns context 0: zk_decode_wait first
    if (n_frames > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    const uint32_t m = x->m, add = n_frames - m;
    if (add == 0) return 0;
    if (!d_comp || !d_c_off || !d_d_off) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &c = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, c, stream);
    int rc;
    std::vector<uint64_t> doff((size_t)add + 1);
    ZK_HIP(hipMemcpyAsync(doff.data(), (const uint64_t *)d_d_off + m, doff.size() * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    uint64_t max_frame = 0;
    if ((rc = zk_enc_list_check(doff.data(), add, &max_frame))) return rc;
    if ((rc = zkx_reserve(x, st, n_frames))) return rc;
    const uint64_t pass_max = e->enc.dedup_pass_bytes ? e->enc.dedup_pass_bytes : ZKX_PASS_BYTES;
    const auto len_of = [&](uint32_t k) { return doff[k + 1] - doff[k]; };
    ZK_HIP(hipMemsetAsync(x->keys + m, 0, (size_t)add * 8, st));
    for (uint32_t a = 0; a < add;) {
        const uint32_t b = zkx_pass_end(a, add, pass_max, len_of);
        const uint64_t bytes = doff[b] - doff[a];
        if (bytes) {
            if ((rc = zk_devbuf_reserve(e, c.rng, (size_t)bytes + 64))) return rc;
            const zk_dec_args da{d_comp, comp_size, d_c_off, d_d_off, m + a, b - a, nullptr, nullptr, c.rng.p, bytes, 1, nullptr, nullptr, 0, /*alone*/ !e->slot_busy[1]};
            if ((rc = zk_decode_enqueue(e, c, st, da))) { (void)hipStreamSynchronize(st); return rc; }
            zkx_hash_launch(st, (const uint8_t *)c.rng.p, (const uint64_t *)d_d_off + m + a, doff[a], b - a, max_frame, x->keys + m + a);
            if ((rc = zk_decode_finish(e, c, st))) return rc;
        }
        a = b;
    }
    hipLaunchKernelGGL(zk_k_dxi_lens, dim3(zkd_blocks(add)), dim3(ZKD_THREADS), 0, st, (const uint64_t *)d_d_off + m, add, x->lens + m);
    return zkx_commit(x, st, add);
}

namespace {
// what zk_dedup_map_dev left: the in-call map in the engine's scratch, its kernel times, the offsets on the host
struct ZkDxMap { ZkDedupScratch S; ZkDedupTimes T; uint64_t *off = nullptr; uint64_t max_frame = 0; uint32_t nu = 0; };
struct ZkDxScratch { uint64_t *flags, *pos, *poff; uint32_t *cand, *out, *list, *pid, *pk, *differ, *ids, *fresh, *cs, *ds; int32_t *fstat; };

// The lookup behind the in-call map.  ids and fresh are left in the engine's scratch (D), *n_fresh is set; the stream is synchronised
int zkx_map(zk_engine *e, const zk_dedup_index *x, hipStream_t st, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
            const void *d_src, const void *d_off, uint32_t count, ZkDxMap &H, ZkDxScratch &D, ZkDxTimes &T, uint32_t *n_fresh)
{
    int rc;
    if ((rc = zk_dedup_map_dev(e, st, d_src, d_off, count, H.S, H.T, &H.off, &H.max_frame, &H.nu))) return rc;
    T.take(e);
    const uint32_t nu = H.nu;
    const uint64_t *off = H.off;
    const uint8_t *src = d_src ? (const uint8_t *)d_src + off[0] : nullptr;
    const ZkDxLayout L = zkx_layout(count);
    if ((rc = zk_devbuf_reserve(e, e->enc.dx, L.end + 64))) return rc;
    uint8_t *b = (uint8_t *)e->enc.dx.p;
    D = ZkDxScratch{(uint64_t *)(b + L.flags), (uint64_t *)(b + L.pos), (uint64_t *)(b + L.poff), (uint32_t *)(b + L.cand), (uint32_t *)(b + L.out), (uint32_t *)(b + L.list),
                    (uint32_t *)(b + L.pid), (uint32_t *)(b + L.pk), (uint32_t *)(b + L.differ), (uint32_t *)(b + L.ids), (uint32_t *)(b + L.fresh), (uint32_t *)(b + L.cs), (uint32_t *)(b + L.ds), (int32_t *)(b + L.fstat)};
    zk_engine::DecCtx &c = e->dctx[0];
    const ZkDxIndex xi{x->keys, x->lens, x->table, x->m, x->slots - 1, x->bits};
    const uint64_t pass_max = e->enc.dedup_pass_bytes ? e->enc.dedup_pass_bytes : ZKX_PASS_BYTES;
    std::vector<uint32_t> uniq(nu), open, next, out, pid, pk, differ;
    std::vector<uint64_t> poff;
    ZK_HIP(hipMemcpyAsync(uniq.data(), H.S.uniq, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemsetAsync(D.cand, 0xFF, (size_t)nu * 4, st));
    uint32_t nopen = nu;
    for (uint32_t round = 0; nopen; round++) {
        if (round) ZK_HIP(hipMemcpyAsync(D.list, open.data(), (size_t)nopen * 4, hipMemcpyHostToDevice, st));
        {
            zk_kernel_timer t(e, ZK_K_DXI_LOOKUP, st);
            hipLaunchKernelGGL(zk_k_dxi_lookup, dim3(zkd_blocks(nopen)), dim3(ZKD_THREADS), 0, st, xi, (const uint64_t *)d_d_off, H.S.hash, (const uint64_t *)d_off, H.S.uniq,
                               round ? D.list : nullptr, nopen, D.cand, D.out);
        }
        out.resize(nopen);
        ZK_HIP(hipMemcpyAsync(out.data(), D.out, (size_t)nopen * 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipGetLastError());
        T.take(e);
        // the round's pairs: an open frame with a candidate and at least one byte (an empty frame is its empty candidate)
        pid.clear(); pk.clear();
        for (uint32_t t = 0; t < nopen; t++) {
            const uint32_t k = round ? open[t] : t;
            if (out[t] == ZKX_FRESH || off[uniq[k] + 1] == off[uniq[k]]) continue;
            pid.push_back(out[t]); pk.push_back(k);
        }
        const uint32_t np = (uint32_t)pid.size();
        if (!np) break;
        const auto len_of = [&](uint32_t p) { return off[uniq[pk[p]] + 1] - off[uniq[pk[p]]]; };
        // the passes: pass s holds pairs [cut[s], cut[s + 1]), its places -- from 0 -- are poff[cut[s] + s ...]
        std::vector<uint32_t> cut{0};
        poff.clear();
        while (cut.back() < np) {
            const uint32_t p0 = cut.back(), p1 = zkx_pass_end(p0, np, pass_max, len_of);
            uint64_t at = 0;
            for (uint32_t p = p0; p < p1; p++) { poff.push_back(at); at += len_of(p); }
            poff.push_back(at);
            cut.push_back(p1);
        }
        ZK_HIP(hipMemcpyAsync(D.pid, pid.data(), (size_t)np * 4, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(D.pk, pk.data(), (size_t)np * 4, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(D.poff, poff.data(), poff.size() * 8, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemsetAsync(D.differ, 0, (size_t)np * 4, st));
        ZK_HIP(hipStreamSynchronize(st));                   // (the vectors are pageable)
        for (size_t s = 0; s + 1 < cut.size(); s++) {
            const uint32_t p0 = cut[s], n = cut[s + 1] - p0;
            const uint64_t *d_poff = D.poff + p0 + s;
            const uint64_t bytes = poff[p0 + s + n];
            if ((rc = zk_devbuf_reserve(e, c.rng, (size_t)bytes + 64))) return rc;
            const zk_dec_args da{d_comp, comp_size, d_c_off, d_d_off, 0, n, D.pid + p0, d_poff, c.rng.p, bytes, 1, D.fstat + p0, nullptr, 0, /*alone*/ !e->slot_busy[1]};
            if ((rc = zk_decode_enqueue(e, c, st, da))) { (void)hipStreamSynchronize(st); return rc; }
            {
                zk_kernel_timer t(e, ZK_K_DXI_COMPARE, st);
                hipLaunchKernelGGL(zk_k_dxi_compare, dim3(n < ZKD_GRID_MAX ? n : ZKD_GRID_MAX, zkd_pieces(H.max_frame)), dim3(ZKD_THREADS), 0, st, src, (const uint64_t *)d_off,
                                   off[0], H.S.uniq, D.pk + p0, d_poff, (const uint8_t *)c.rng.p, n, D.differ + p0);
            }
            rc = zk_decode_finish(e, c, st);
            T.take(e);
            if (rc) return rc;                              // a candidate that does not decode or verify: its -(code)
        }
        differ.resize(np);
        ZK_HIP(hipMemcpyAsync(differ.data(), D.differ, (size_t)np * 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        next.clear();
        for (uint32_t p = 0; p < np; p++) if (differ[p]) next.push_back(pk[p]);
        open.swap(next);
        nopen = (uint32_t)open.size();
    }
    {
        zk_kernel_timer t(e, ZK_K_DXI_EMIT, st);
        hipLaunchKernelGGL(zk_k_dxi_flags, dim3(zkd_blocks((uint64_t)nu + 1)), dim3(ZKD_THREADS), 0, st, D.cand, nu, D.flags);
        zk_launch_scan64(st, D.flags, nu + 1, D.pos);
        hipLaunchKernelGGL(zk_k_dxi_emit, dim3(zkd_blocks(count)), dim3(ZKD_THREADS), 0, st, H.S.ids, H.S.uniq, D.cand, D.pos, count, nu, x->m, D.ids, D.fresh);
    }
    uint64_t nf = 0;
    ZK_HIP(hipMemcpyAsync(&nf, D.pos + nu, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    T.take(e);
    *n_fresh = (uint32_t)nf;
    return 0;
}
// what both calls refuse for, before anything is read, reserved or waited for
int zkx_refuse(const zk_engine *e, const zk_dedup_index *x, const void *d_comp, const void *d_c_off, const void *d_d_off, uint32_t n_frames, uint32_t count,
               uint32_t *n_fresh)
{
    if (count && e->slot_busy[0]) return ZK_ERR_ARGUMENT;   // a submitted batch still owns context 0: zk_decode_wait first (nothing touched, *n_fresh included)
    *n_fresh = 0;
    if (x->e != e || n_frames < x->m) return ZK_ERR_ARGUMENT;
    if (count && x->m && (!d_comp || !d_c_off || !d_d_off)) return ZK_ERR_ARGUMENT;
    return 0;
}
}  // namespace

extern "C" int zk_dedup_against_dev(zk_engine *e, const zk_dedup_index *x, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                                    uint32_t n_frames, const void *d_src, const void *d_off, uint32_t count, void *d_ids, void *d_fresh, uint32_t *n_fresh,
                                    void *stream)
{
    if (!e || !x || !n_fresh) return ZK_ERR_ARGUMENT;
    if (const int rc = zkx_refuse(e, x, d_comp, d_c_off, d_d_off, n_frames, count, n_fresh)) return rc;
    if (count > ZK_SEEKABLE_MAX_FRAMES || (uint64_t)x->m + count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!d_off) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = zk_dec_stream(e, e->dctx[0], stream);
    ZkDxMap H;
    ZkDxScratch D;
    ZkDxTimes T;
    uint32_t nf = 0;
    if (const int rc = zkx_map(e, x, st, d_comp, comp_size, d_c_off, d_d_off, d_src, d_off, count, H, D, T, &nf)) return rc;
    if (d_ids) ZK_HIP(hipMemcpyAsync(d_ids, D.ids, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    if (d_fresh) ZK_HIP(hipMemcpyAsync(d_fresh, D.fresh, (size_t)nf * 4, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    T.publish(e, true);
    *n_fresh = nf;
    return 0;
}

extern "C" int zk_encode_dedup_against_dev(zk_engine *e, zk_dedup_index *x, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                                           uint32_t n_frames, const void *d_src, const void *d_off, uint32_t count, int level, int checksum, const zk_cdict *cdict,
                                           void *d_dst, uint64_t dst_cap, void *d_ids, void *d_fresh, void *d_c_sizes, void *d_d_sizes, uint32_t *n_fresh,
                                           uint64_t *written, void *stream)
{
    if (!e || !x || !n_fresh || (cdict && cdict->e != e)) return ZK_ERR_ARGUMENT;
    if (const int rc = zkx_refuse(e, x, d_comp, d_c_off, d_d_off, n_frames, count, n_fresh)) return rc;
    if (count > ZK_SEEKABLE_MAX_FRAMES || (uint64_t)x->m + count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) { if (written) *written = 0; return 0; }
    if (!d_off || !d_dst) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = zk_dec_stream(e, e->dctx[0], stream);
    ZkDxMap H;
    ZkDxScratch D;
    ZkDxTimes T;
    uint32_t nf = 0;
    int rc;
    if ((rc = zkx_map(e, x, st, d_comp, comp_size, d_c_off, d_d_off, d_src, d_off, count, H, D, T, &nf))) return rc;
    // room in the index first, the encode second: a call that fails leaves the index, the destination and the caller's arrays as they were
    // (the list encoder writes its sizes before it knows whether the destination holds the frames: they go to scratch)
    if ((rc = zkx_reserve(x, st, x->m + nf))) return rc;
    uint64_t wr = 0;
    ZkDedupScratch F = H.S;
    F.uniq = D.fresh;                                       // the fresh frames in the unique ones' place
    if (nf && (rc = zk_dedup_encode(e, st, d_src ? (const uint8_t *)d_src + H.off[0] : nullptr, (const uint64_t *)d_off, H.off[0], H.off, count, nf, H.max_frame, F, H.T, level,
                                    checksum, nullptr, 0, cdict, (uint8_t *)d_dst, dst_cap, D.cs, D.ds, &wr))) return rc;
    T.publish(e, nf == 0);
    if (nf) hipLaunchKernelGGL(zk_k_dxi_take, dim3(zkd_blocks(nf)), dim3(ZKD_THREADS), 0, st, H.S.hash, (const uint64_t *)d_off, D.fresh, nf, x->keys + x->m, x->lens + x->m);
    if (d_ids) ZK_HIP(hipMemcpyAsync(d_ids, D.ids, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    if (d_fresh) ZK_HIP(hipMemcpyAsync(d_fresh, D.fresh, (size_t)nf * 4, hipMemcpyDeviceToDevice, st));
    if (d_c_sizes) ZK_HIP(hipMemcpyAsync(d_c_sizes, D.cs, (size_t)nf * 4, hipMemcpyDeviceToDevice, st));
    if (d_d_sizes) ZK_HIP(hipMemcpyAsync(d_d_sizes, D.ds, (size_t)nf * 4, hipMemcpyDeviceToDevice, st));
    {
        zk_profiling_off quiet(e);                          // (the insert's events would be read by nobody)
        if ((rc = zkx_commit(x, st, nf))) return rc;
    }
    *n_fresh = nf;
    if (written) *written = wr;
    return 0;
}

// zk_dedup_index_compact_dev (zk_compact.hip) moves the kept frames' keys and lengths to the front of the arrays and has the table rebuilt here
ZkDxArrays zk_dedup_index_arrays(zk_dedup_index *x) { return ZkDxArrays{x->e, x->m, x->keys, x->lens}; }
int zk_dedup_index_rebuilt(zk_dedup_index *x, hipStream_t st, uint32_t m)
{
    zk_engine *e = x->e;
    x->m = m;
    if (const int rc = zkx_rebuild(x, st, m)) return rc;
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    return 0;
}

// zk_digest.hip -- zk_frame_digests[_dev], zk_archive_digests_dev: a cryptographic digest per frame of a list, or per decoded frame of a
// device-resident archive (include/zeekstd_amd.h "THE DIGEST"; the lane code, the kernels and the scheme: zk_digest.h).
//   a list       the offsets come to the host and are checked (one wait, as in zk_frame_keys_dev) -- the host then knows the number of leaves,
//                so nothing is read back for it --; SHA-256: zk_k_digest_sha256; BLAKE2s tree: zk_k_digest_counts, zk_k_scan64,
//                zk_k_digest_leaves into engine scratch, zk_k_digest_roots; one wait at the end
//   an archive   the loop of zk_dedup_index_add_archive_dev: passes of at most ZK_CHOICE_DEDUP_PASS_KIB decoded bytes (one whole frame at
//                least) through zk_decode_enqueue on context 0 into dctx[0].rng, the digest kernels behind the decode on the same queue,
//                zk_decode_finish (a wait)
// The scratch is the encoder's (zk_engine::Enc::dg, dg_up): a submitted decode batch is not touched by the list calls.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_kernels.h"
#include "zk_digest.h"

static_assert(ZKG_SHA256 == ZK_DIGEST_SHA256 && ZKG_BLAKE2S_TREE == ZK_DIGEST_BLAKE2S_TREE && ZKG_BYTES == ZK_DIGEST_BYTES && ZKG_LEAF == ZK_DIGEST_LEAF,
              "zk_digest.h restates the header's constants");

namespace {
bool zkg_algo_ok(int algo) { return algo == ZK_DIGEST_SHA256 || algo == ZK_DIGEST_BLAKE2S_TREE; }

// The digests of `count` > 0 checked frames, enqueued on st: frame i is src[off[i] - off[0] ...] (src: the byte off[0] names), d_off the
// offsets on the device, off a host copy of them.  No wait
int zkg_enqueue(zk_engine *e, hipStream_t st, int algo, const uint8_t *src, const uint64_t *d_off, const uint64_t *off, uint32_t count, uint32_t *d_digests)
{
    const dim3 tb(ZKG_THREADS);
    if (algo == ZK_DIGEST_SHA256) {
        zk_kernel_timer t(e, ZK_K_DIGEST_LEAVES, st);
        hipLaunchKernelGGL(zk_k_digest_sha256, dim3(zkg_blocks(count)), tb, 0, st, src, d_off, off[0], count, d_digests);
        return 0;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < count; i++) total += zkg_leaves(off[i + 1] - off[i]);
    const ZkgLayout L = zkg_layout(count, total);
    if (const int rc = zk_devbuf_reserve(e, e->enc.dg, L.end + 64)) return rc;
    uint8_t *b = (uint8_t *)e->enc.dg.p;
    uint64_t *cnt = (uint64_t *)(b + L.cnt), *lp = (uint64_t *)(b + L.lp);
    uint32_t *leaves = (uint32_t *)(b + L.leaves);
    {
        zk_kernel_timer t(e, ZK_K_DIGEST_PLAN, st);
        hipLaunchKernelGGL(zk_k_digest_counts, dim3(zkg_blocks(count)), tb, 0, st, d_off, count, cnt);
        zk_launch_scan64(st, cnt, count, lp);
    }
    { zk_kernel_timer t(e, ZK_K_DIGEST_LEAVES, st); hipLaunchKernelGGL(zk_k_digest_leaves, dim3(zkg_blocks(total)), tb, 0, st, src, d_off, off[0], count, lp, total, leaves); }
    { zk_kernel_timer t(e, ZK_K_DIGEST_ROOTS, st); hipLaunchKernelGGL(zk_k_digest_roots, dim3(zkg_blocks(count)), tb, 0, st, leaves, lp, count, d_digests); }
    return 0;
}
}  // namespace

extern "C" int zk_frame_digests_dev(zk_engine *e, int algo, const void *d_src, const void *d_off, uint32_t count, void *d_digests, void *stream)
{
    if (!e || !zkg_algo_ok(algo)) return ZK_ERR_ARGUMENT;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!d_off || !d_digests || ((uintptr_t)d_digests & 3u)) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    int rc;
    if ((rc = zk_pin_reserve(e, e->enc.pin_dd, e->enc.pin_dd_cap, ((size_t)count + 1) * 8 + (size_t)count * 4))) return rc;
    uint64_t *off = (uint64_t *)e->enc.pin_dd, max_frame = 0;
    ZK_HIP(hipMemcpyAsync(off, d_off, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    if (off[count] != off[0] && !d_src) return ZK_ERR_ARGUMENT;
    zk_profile_begin(e);
    if ((rc = zkg_enqueue(e, st, algo, d_src ? (const uint8_t *)d_src + off[0] : nullptr, (const uint64_t *)d_off, off, count, (uint32_t *)d_digests))) return rc;
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    return 0;
}

extern "C" int zk_frame_digests(zk_engine *e, int algo, const uint8_t *src, const uint64_t *off, uint32_t count, uint8_t *digests)
{
    if (!e || !zkg_algo_ok(algo)) return ZK_ERR_ARGUMENT;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if (count == 0) return 0;
    if (!off || !digests) return ZK_ERR_ARGUMENT;
    uint64_t max_frame = 0;
    int rc;
    if ((rc = zk_enc_list_check(off, count, &max_frame))) return rc;
    const uint64_t n = off[count] - off[0];
    if (n && !src) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // the source whole, its offsets -- counted from off[0] -- and the digests behind it
    const size_t off_at = ((size_t)n + 15) & ~(size_t)15, out_at = off_at + ((((size_t)count + 1) * 8 + 15) & ~(size_t)15);
    if ((rc = zk_devbuf_reserve(e, e->enc.dg_up, out_at + (size_t)count * ZK_DIGEST_BYTES + 64))) return rc;
    uint8_t *b = (uint8_t *)e->enc.dg_up.p;
    if (n) ZK_HIP(hipMemcpyAsync(b, src + off[0], (size_t)n, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> rel((size_t)count + 1);
    for (uint32_t i = 0; i <= count; i++) rel[i] = off[i] - off[0];
    ZK_HIP(hipMemcpyAsync(b + off_at, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
    zk_profile_begin(e);
    if ((rc = zkg_enqueue(e, st, algo, b, (const uint64_t *)(b + off_at), rel.data(), count, (uint32_t *)(b + out_at)))) { (void)hipStreamSynchronize(st); return rc; }
    ZK_HIP(hipMemcpyAsync(digests, b + out_at, (size_t)count * ZK_DIGEST_BYTES, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    return 0;
}

extern "C" int zk_archive_digests_dev(zk_engine *e, int algo, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off,
                                      uint32_t first, uint32_t count, void *d_digests, void *stream)
{
    if (!e || !zkg_algo_ok(algo)) return ZK_ERR_ARGUMENT;
    if (count && e->slot_busy[0]) return ZK_ERR_ARGUMENT;   // a submitted batch still owns context 0: zk_decode_wait first
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    if ((uint64_t)first + count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_ARGUMENT;
    if (count == 0) return 0;
    if (!d_comp || !d_c_off || !d_d_off || !d_digests || ((uintptr_t)d_digests & 3u)) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &c = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, c, stream);
    int rc;
    std::vector<uint64_t> doff((size_t)count + 1);
    ZK_HIP(hipMemcpyAsync(doff.data(), (const uint64_t *)d_d_off + first, doff.size() * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    uint64_t max_frame = 0;
    if ((rc = zk_enc_list_check(doff.data(), count, &max_frame))) return rc;
    const uint64_t pass_max = e->enc.dedup_pass_bytes ? e->enc.dedup_pass_bytes : ZKG_PASS_BYTES;
    // (every decode pass begins a profile of its own: the passes' times are added up here)
    float ms[ZK_NKERNELS] = {};
    const auto take = [&] {
        if (!e->profiling) return;
        zk_profile_collect(e);
        for (int k = 0; k < ZK_NKERNELS; k++) { ms[k] += e->kernel_ms[k]; e->kernel_ms[k] = 0.f; e->ev_used[k] = false; }
    };
    zk_profile_begin(e);
    for (uint32_t a = 0; a < count;) {
        const uint32_t b = zkg_pass_end(doff.data(), a, count, pass_max);
        const uint64_t bytes = doff[b] - doff[a];
        if (bytes) {
            if ((rc = zk_devbuf_reserve(e, c.rng, (size_t)bytes + 64))) return rc;
            const zk_dec_args da{d_comp, comp_size, d_c_off, d_d_off, first + a, b - a, nullptr, nullptr, c.rng.p, bytes, 1, nullptr, nullptr, 0, /*alone*/ !e->slot_busy[1]};
            if ((rc = zk_decode_enqueue(e, c, st, da))) { (void)hipStreamSynchronize(st); return rc; }
        }
        if ((rc = zkg_enqueue(e, st, algo, bytes ? (const uint8_t *)c.rng.p : nullptr, (const uint64_t *)d_d_off + first + a, doff.data() + a, b - a,
                              (uint32_t *)d_digests + (size_t)a * (ZK_DIGEST_BYTES / 4)))) { (void)hipStreamSynchronize(st); return rc; }
        if (bytes) rc = zk_decode_finish(e, c, st);
        else { ZK_HIP(hipStreamSynchronize(st)); ZK_HIP(hipGetLastError()); }
        take();
        if (rc) return rc;                                  // a frame that does not decode or verify: its -(code)
        a = b;
    }
    if (e->profiling) for (int k = 0; k < ZK_NKERNELS; k++) e->kernel_ms[k] = ms[k];
    return 0;
}

// zk_cdc.hip -- zk_chunk_boundaries[_dev], zk_encode_chunked[_dev]: content-defined frame boundaries on the device (include/zeekstd_amd.h;
// DESIGN.md 5j).  Per slice of the input (ZK_CHOICE_CDC_SLICE_KIB, 64 MiB by default):
//   1. zk_k_cdc_mark     a candidate bit per position, the candidates counted per tile (zk_cdc.h)
//   2. zk_k_scan64       where each tile's candidates go
//   3. zk_k_cdc_emit     the candidates as a sorted list
//   4. the selection     zk_k_cdc_select, one wave that walks the chain of cuts over the list, for a slice of one segment; else zk_k_cdc_spec (a
//                        speculative chain per segment, side by side), zk_k_cdc_fix (the true chain adopts them) and zk_k_cdc_copy.  The chain's
//                        cut and count stay on the device for the next slice
// Nothing comes to the host between the slices; the count is read once at the end.
// The device entry point writes the caller's array in the pass that finds the cuts when off_cap >= n / min + 1 (no chain has more cuts);
// with less room it counts first -- a pass that stores nothing -- and runs again only when the count fits.
// All scratch is the encoder's (zk_engine::Enc::cdc, cdc_src, cdc_off): a submitted decode batch is not touched.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_cdc.h"

constexpr uint64_t ZKC_SLICE_BYTES = 64ull << 20;         // ZK_CHOICE_CDC_SLICE_KIB's default

namespace {
// the parameters' defaults and ranges: 0 or ZK_ERR_ARGUMENT
int zk_cdc_rule(const zk_chunk_params *p, ZkCdcRule &r)
{
    static const zk_chunk_params defaults = {0, 0, 0, 0};
    if (!p) p = &defaults;
    if (p->flags) return ZK_ERR_ARGUMENT;
    const uint32_t avg = p->avg_size ? p->avg_size : 1u << 21;
    if (avg < (1u << 8) || avg > (1u << 24) || (avg & (avg - 1))) return ZK_ERR_ARGUMENT;
    const uint32_t mn = p->min_size ? p->min_size : avg / 4;
    if (mn < 64 || mn > avg) return ZK_ERR_ARGUMENT;
    const uint64_t mx4 = 4ull * avg;
    const uint32_t mx = p->max_size ? p->max_size : (uint32_t)(mx4 < (1ull << 30) ? mx4 : 1ull << 30);
    if (mx < mn || mx > ZK_SEEKABLE_MAX_FRAME_SIZE) return ZK_ERR_ARGUMENT;
    r.min = mn; r.max = mx; r.bits = 0;
    while ((1u << r.bits) < avg) r.bits++;
    return 0;
}

struct ZkCdcTimes { float mark = 0.f, select = 0.f; };
// One pass over the input: the chain's cuts to d_off[1 ...] (device memory of off_cap + 1 entries, or null: counted only), d_off[0] = 0;
// *count_out: the cuts behind d_off[0], also those that found no room.  h_src: the source in host memory, uploaded slice by slice; else
// d_src.  n > 0.  The stream is synchronised.
int zk_cdc_pass(zk_engine *e, hipStream_t st, const uint8_t *d_src, const uint8_t *h_src, uint64_t n, const ZkCdcRule &r, uint64_t *d_off, uint64_t off_cap,
                uint64_t *count_out)
{
    const uint64_t slice_max = e->enc.cdc_slice_bytes ? e->enc.cdc_slice_bytes : ZKC_SLICE_BYTES;
    const uint64_t slice = n < slice_max ? n : slice_max;
    const ZkCdcLayout L = zkc_layout(slice, r.min, r.bits);
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.cdc, L.end + 64))) return rc;
    if (h_src && (rc = zk_devbuf_reserve(e, e->enc.cdc_src, (size_t)slice + ZKC_LEAD + 64))) return rc;
    uint8_t *base = (uint8_t *)e->enc.cdc.p;
    uint4 *bitmap = (uint4 *)(base + L.bitmap);
    uint64_t *counts = (uint64_t *)(base + L.counts), *bases = (uint64_t *)(base + L.bases);
    ZkCdcState *state = (ZkCdcState *)(base + L.state);
    uint32_t *list = (uint32_t *)(base + L.list);
    uint64_t *nruns = (uint64_t *)(base + L.nruns), *rows = (uint64_t *)(base + L.rows);
    ZkCdcSegMeta *meta = (ZkCdcSegMeta *)(base + L.meta);
    ZkCdcRun *runs = (ZkCdcRun *)(base + L.runs);
    zk_profile_begin(e);
    ZkCdcTimes ms;
    ZK_HIP(hipMemsetAsync(state, 0, sizeof(ZkCdcState), st));
    if (d_off) ZK_HIP(hipMemsetAsync(d_off, 0, 8, st));
    for (uint64_t s0 = 0; s0 < n; s0 += slice) {
        const uint64_t len = n - s0 < slice ? n - s0 : slice;
        const uint32_t tiles = zkc_tiles(len);
        const uint8_t *src = d_src;
        uint64_t src_pos = 0;
        if (h_src) {
            // the slice and the 31 bytes before it
            src_pos = s0 >= ZKC_LEAD ? s0 - ZKC_LEAD : 0;
            ZK_HIP(hipMemcpyAsync(e->enc.cdc_src.p, h_src + src_pos, (size_t)(s0 + len - src_pos), hipMemcpyHostToDevice, st));
            src = (const uint8_t *)e->enc.cdc_src.p;
        }
        const ZkCdcSlice a{src, src_pos, s0, len, r.bits};
        { zk_kernel_timer t(e, ZK_K_CDC_MARK, st); hipLaunchKernelGGL(zk_k_cdc_mark, dim3(tiles), dim3(ZKC_THREADS), 0, st, a, bitmap, counts); }
        zk_launch_scan64(st, counts, tiles, bases);
        hipLaunchKernelGGL(zk_k_cdc_emit, dim3(tiles), dim3(ZKC_THREADS), 0, st, bitmap, bases, list);
        // one segment: the serial walk; more: a speculative chain per segment, the true chain's fix-up, the runs it adopted
        const uint32_t nseg = (uint32_t)((len + L.g.seg - 1) / L.g.seg);
        const ZkCdcSel sel{n, s0, s0 + len, r.min, r.max, off_cap, L.g.seg, nseg, L.g.row};
        {
            zk_kernel_timer t(e, ZK_K_CDC_SELECT, st);
            if (nseg == 1) hipLaunchKernelGGL(zk_k_cdc_select, dim3(1), dim3(ZKC_SEL_THREADS), 0, st, sel, list, bases + tiles, state, d_off);
            else {
                hipLaunchKernelGGL(zk_k_cdc_spec, dim3(nseg), dim3(ZKC_SEL_THREADS), 0, st, sel, list, bases + tiles, rows, meta);
                hipLaunchKernelGGL(zk_k_cdc_fix, dim3(1), dim3(ZKC_SEL_THREADS), 0, st, sel, list, bases + tiles, rows, meta, state, d_off, runs, nruns);
                hipLaunchKernelGGL(zk_k_cdc_copy, dim3(nseg), dim3(ZKC_THREADS), 0, st, sel, rows, runs, nruns, d_off);
            }
        }
        if (e->profiling) {
            // (a kernel's pair of events holds one launch: the slices' times are added up here)
            ZK_HIP(hipStreamSynchronize(st));
            zk_profile_collect(e);
            ms.mark += e->kernel_ms[ZK_K_CDC_MARK]; ms.select += e->kernel_ms[ZK_K_CDC_SELECT];
        }
    }
    ZkCdcState end;
    ZK_HIP(hipMemcpyAsync(&end, state, sizeof end, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    if (e->profiling) { e->kernel_ms[ZK_K_CDC_MARK] = ms.mark; e->kernel_ms[ZK_K_CDC_SELECT] = ms.select; }
    if (end.cut != n) return -(int)ZK_E_GENERIC;
    *count_out = end.count;
    return 0;
}
}  // namespace

extern "C" uint64_t zk_compress_bound_chunked(uint64_t n, const zk_chunk_params *p, int with_dictionary)
{
    ZkCdcRule r;
    if (zk_cdc_rule(p, r)) return 0;
    const uint64_t frames = n / r.min + 1;
    if (frames > ZK_SEEKABLE_MAX_FRAMES) return 0;
    return zk_compress_bound_list(n, (uint32_t)frames, with_dictionary);
}

extern "C" int zk_chunk_boundaries_dev(zk_engine *e, const void *d_src, uint64_t n, const zk_chunk_params *p, void *d_off_out, uint32_t off_cap,
                                       uint32_t *count, void *stream)
{
    ZkCdcRule r;
    if (const int rc = zk_cdc_rule(p, r)) return rc;
    if (!e || !count || (n && !d_src) || (off_cap && !d_off_out)) return ZK_ERR_ARGUMENT;
    *count = 0;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    if (n == 0) {
        // the empty frame of the other routes
        *count = 1;
        if (off_cap < 1) return -(int)ZK_E_DST_TOO_SMALL;
        ZK_HIP(hipMemsetAsync(d_off_out, 0, 16, st));
        ZK_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const uint64_t most = n / r.min + 1;                    // every frame but the last has min bytes or more
    const bool direct = off_cap >= most;
    uint64_t cuts = 0;
    int rc;
    if ((rc = zk_cdc_pass(e, st, (const uint8_t *)d_src, nullptr, n, r, direct ? (uint64_t *)d_off_out : nullptr, off_cap, &cuts))) return rc;
    if (cuts > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    *count = (uint32_t)cuts;
    if (direct) return 0;
    if (cuts > off_cap) return -(int)ZK_E_DST_TOO_SMALL;
    return zk_cdc_pass(e, st, (const uint8_t *)d_src, nullptr, n, r, (uint64_t *)d_off_out, off_cap, &cuts);
}

extern "C" int zk_chunk_boundaries(zk_engine *e, const uint8_t *src, uint64_t n, const zk_chunk_params *p, uint64_t *off_out, uint32_t off_cap, uint32_t *count)
{
    ZkCdcRule r;
    if (const int rc = zk_cdc_rule(p, r)) return rc;
    if (!e || !count || (n && !src) || (off_cap && !off_out)) return ZK_ERR_ARGUMENT;
    *count = 0;
    if (n == 0) {
        *count = 1;
        if (off_cap < 1) return -(int)ZK_E_DST_TOO_SMALL;
        off_out[0] = off_out[1] = 0;
        return 0;
    }
    ZK_HIP(hipSetDevice(e->device));
    // the cuts that find room go to a device array of the engine's in the one pass, and from there to the caller when all did
    const uint64_t most = n / r.min + 1, room = off_cap < most ? off_cap : most;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.cdc_off, ((size_t)room + 1) * 8))) return rc;
    uint64_t cuts = 0;
    if ((rc = zk_cdc_pass(e, e->stream, nullptr, src, n, r, (uint64_t *)e->enc.cdc_off.p, room, &cuts))) return rc;
    if (cuts > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;
    *count = (uint32_t)cuts;
    if (cuts > off_cap) return -(int)ZK_E_DST_TOO_SMALL;
    ZK_HIP(hipMemcpyAsync(off_out, e->enc.cdc_off.p, ((size_t)cuts + 1) * 8, hipMemcpyDeviceToHost, e->stream));
    ZK_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int zk_encode_chunked_dev(zk_engine *e, const void *d_src, uint64_t n, const zk_chunk_params *p, int level, int checksum,
                                     const void *d_prefix, uint64_t prefix_len, const zk_cdict *cdict, void *d_dst, uint64_t dst_cap,
                                     void *d_off_out, uint32_t off_cap, void *d_c_sizes, void *d_d_sizes, uint32_t *n_frames,
                                     uint64_t *written, void *stream)
{
    if (!e || !d_off_out || !d_dst || !n_frames || (cdict && cdict->e != e) || (cdict && d_prefix && prefix_len)) return ZK_ERR_ARGUMENT;
    if (const int rc = zk_chunk_boundaries_dev(e, d_src, n, p, d_off_out, off_cap, n_frames, stream)) return rc;
    return zk_encode_frame_list_dev(e, d_src, d_off_out, *n_frames, level, checksum, d_prefix, prefix_len, cdict, d_dst, dst_cap, d_c_sizes, d_d_sizes, written, stream);
}

extern "C" int zk_encode_chunked(zk_engine *e, const uint8_t *src, uint64_t n, const zk_chunk_params *p, int level, int checksum,
                                 const uint8_t *prefix, uint64_t prefix_len, const zk_cdict *cdict, uint8_t *dst, uint64_t dst_cap,
                                 uint64_t *off_out, uint32_t off_cap, uint32_t *c_sizes, uint32_t *d_sizes, uint32_t *n_frames, uint64_t *written)
{
    if (!e || !off_out || !dst || !n_frames || (cdict && cdict->e != e) || (cdict && prefix && prefix_len)) return ZK_ERR_ARGUMENT;
    if (const int rc = zk_chunk_boundaries(e, src, n, p, off_out, off_cap, n_frames)) return rc;
    return zk_encode_frame_list(e, src, off_out, *n_frames, level, checksum, prefix, prefix_len, cdict, dst, dst_cap, c_sizes, d_sizes, written);
}

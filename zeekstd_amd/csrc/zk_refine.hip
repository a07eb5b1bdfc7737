// zk_refine.hip -- zk_refine_entries_dev / zk_refine_entries (include/zeekstd_amd.h): a seek table refined to one entry per frame, on the
// device.  DESIGN.md 5f has the scheme; the stages:
//   zk_k_refine_split (count)   one lane per entry: how many pieces it has (zk_split_entry, zk_refine.h)
//   zk_k_scan64                 where each entry's pieces go in the scratch table; the total is read back (it sizes the scratch)
//   zk_k_refine_split (emit)    the scratch table: prefix offsets of every piece, the entry each came from
//   the size stages             counting walk, scan, filling walk, sequence walks, zk_k_frame_sizes over the scratch table: what
//                               zk_frame_content_sizes_dev runs -- a piece's size and its verdict
//   zk_k_refine_mark            one lane per piece: the first failing piece of each entry (atomicMin on (piece, code))
//   zk_k_refine_fold            one lane per entry: its verdict, how many refined entries it yields (its pieces, or 1) and their bytes
//   zk_k_scan64 x 3             the pieces' sizes, the yields, the entries' bytes
//   zk_k_refine_emit            one lane per piece: c_out / d_out / entry_of, every element written once
// The entry kernels are latency chains of dependent global loads like zk_k_walk: no LDS, nothing to tune.  Entry-level parallelism is
// the design; a stream without a table is ONE chain by nature (frame i + 1 begins where frame i's last block ends).
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_kernels.h"
#include "zk_refine.h"

constexpr unsigned long long ZK_REFINE_NONE = ~0ull;

// base == nullptr: count (cnt[e] = pieces of entry e).  Else emit: fc[base[e] + j] = first byte of piece j, ent[..] = e, and the words of
// the fold (first[e]: no piece has failed yet).  An entry whose range is not inside the buffer is one piece that zk_k_walk refuses.
__global__ __launch_bounds__(64) void zk_k_refine_split(const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, uint32_t n,
                                                        uint64_t *cnt, const uint64_t *base, uint64_t *fc, uint32_t *ent, unsigned long long *first)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint64_t cb = c_off[e], ce = c_off[e + 1];
    const bool inside = cb <= ce && ce <= comp_size;
    if (!base) {
        cnt[e] = inside ? zk_split_entry(comp, cb, ce, nullptr).n : 1u;
        return;
    }
    uint64_t *starts = fc + base[e];
    const uint64_t k = base[e + 1] - base[e];
    if (inside) zk_split_entry(comp, cb, ce, starts);
    else starts[0] = cb;
    for (uint64_t j = 0; j < k; j++) ent[base[e] + j] = e;
    first[e] = ZK_REFINE_NONE;
    if (e == n - 1) fc[base[n]] = ce;
}

// one lane per piece: a piece that failed (fstat: -ZSTD_ErrorCode) bids for "the first failing piece of its entry"
__global__ __launch_bounds__(256) void zk_k_refine_mark(const int32_t *fstat, const uint32_t *ent, const uint64_t *base, uint64_t total, unsigned long long *first)
{
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= total) return;
    const int32_t st = fstat[f];
    if (st == 0) return;
    const uint32_t e = ent[f];
    atomicMin(&first[e], ((unsigned long long)(f - base[e]) << 32) | (uint32_t)(-st));
}

// one lane per entry.  szs: exclusive scan of the pieces' sizes.  yields[e]: refined entries of entry e; ebytes[e]: what they decode to
// (d_off == nullptr: a bad entry counts 0).  err: (entry << 32 | code) of the first bad entry.
__global__ __launch_bounds__(256) void zk_k_refine_fold(const uint64_t *c_off, const uint64_t *d_off, uint32_t n, const uint64_t *base, const uint64_t *szs,
                                                        const unsigned long long *first, uint64_t *yields, uint64_t *ebytes, int32_t *entry_status,
                                                        unsigned long long *err)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint64_t sum = szs[base[e + 1]] - szs[base[e]];
    uint32_t st = ZK_OK;
    const unsigned long long w = first[e];
    if (w != ZK_REFINE_NONE) st = zk_refine_verdict((uint32_t)(w >> 32), (uint32_t)w);
    // with sizes given, an entry's frames must make the entry's size
    if (st == ZK_OK && d_off && (d_off[e + 1] < d_off[e] || d_off[e + 1] - d_off[e] != sum)) st = ZK_E_CORRUPTION;
    yields[e] = st == ZK_OK ? base[e + 1] - base[e] : 1u;
    ebytes[e] = d_off ? d_off[e + 1] - d_off[e] : st == ZK_OK ? sum : 0u;
    entry_status[e] = -(int32_t)st;
    if (st != ZK_OK) atomicMin(err, ((unsigned long long)e << 32) | st);
}

// one lane per piece (+ one for the tables' last element): where it lands in the refined table.  A bad entry is its first piece's lane alone.
__global__ __launch_bounds__(256) void zk_k_refine_emit(const uint64_t *c_off, const uint64_t *d_off, uint32_t n, const uint64_t *base, const uint64_t *fc,
                                                        const uint32_t *ent, const uint64_t *szs, const uint64_t *yields, const uint64_t *obase,
                                                        const uint64_t *dbase, uint64_t total, uint64_t *c_out, uint64_t *d_out, uint32_t *entry_of)
{
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > total) return;
    if (f == total) {
        c_out[obase[n]] = c_off[n];
        d_out[obase[n]] = d_off ? d_off[n] : dbase[n];
        return;
    }
    const uint32_t e = ent[f];
    const uint64_t j = f - base[e];
    if (j >= yields[e]) return;                             // (a bad entry of several pieces yields one: piece 0 begins where the entry does)
    const uint64_t o = obase[e] + j;
    c_out[o] = fc[f];
    d_out[o] = (d_off ? d_off[e] : dbase[e]) + (szs[f] - szs[base[e]]);
    if (entry_of) entry_of[o] = e;
}

// ---------------------------------------------------------------------------------------------- the entry points
// scratch per entry (8-byte words; n + 1 where a scan's total follows): cnt | base | first | yields | obase | ebytes | dbase, then 2 words
static inline size_t zk_refine_entry_words(uint32_t n) { return 7 * ((size_t)n + 1) + 2; }

extern "C" int zk_refine_entries_dev(zk_engine *e, const void *d_comp, uint64_t comp_size, const void *d_c_off, const void *d_d_off, uint32_t n_entries,
                                     void *d_c_out, void *d_d_out, void *d_entry_of, uint32_t out_cap, uint32_t *n_out, void *d_entry_status, void *stream)
{
    if (!e || !n_out || (n_entries && (!d_comp || !d_c_off || !d_entry_status)) || (out_cap && (!d_c_out || !d_d_out))) return ZK_ERR_ARGUMENT;
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;            // it runs on context 0 (the table above zk_decode_submit_dev)
    *n_out = 0;
    if (n_entries == 0) return 0;                           // (no entry: no table to continue; the caller's arrays stay as they are)
    if (n_entries == 0xFFFFFFFFu) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    zk_engine::DecCtx &c = e->dctx[0];
    hipStream_t st = zk_dec_stream(e, c, stream);
    zk_profiling_off quiet(e);                              // (no per-kernel events here)
    const uint32_t n = n_entries;
    const uint8_t *comp = (const uint8_t *)d_comp;
    const uint64_t *c_off = (const uint64_t *)d_c_off, *d_off = (const uint64_t *)d_d_off;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->rf_entries, zk_refine_entry_words(n) * 8))) return rc;
    uint64_t *cnt = (uint64_t *)e->rf_entries.p, *base = cnt + n + 1, *first64 = base + n + 1, *yields = first64 + n + 1, *obase = yields + n + 1,
             *ebytes = obase + n + 1, *dbase = ebytes + n + 1, *words = dbase + n + 1;
    unsigned long long *first = (unsigned long long *)first64, *err = (unsigned long long *)words;
    const dim3 egrid((n + 63) / 64);
    hipLaunchKernelGGL(zk_k_refine_split, egrid, dim3(64), 0, st, comp, comp_size, c_off, n, cnt, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                       (unsigned long long *)nullptr);
    zk_launch_scan64(st, cnt, n, base);
    ZK_HIP(hipMemcpyAsync(c.h_words + 12, base + n, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    const uint64_t total = c.h_words[12];
    if (total >= 0xFFFFFFFFull) return -(int)ZK_E_GENERIC;   // more pieces than a batch has frames
    // scratch per piece: fc (total + 1) | sizes (total) | szs (total + 1) | ent (u32) | fstat (i32)
    if ((rc = zk_devbuf_reserve(e, e->rf_frames, (3 * (size_t)total + 2) * 8 + (size_t)total * 8))) return rc;
    uint64_t *fc = (uint64_t *)e->rf_frames.p, *sizes = fc + total + 1, *szs = sizes + total;
    uint32_t *ent = (uint32_t *)(szs + total + 1);
    int32_t *fstat = (int32_t *)(ent + total);
    hipLaunchKernelGGL(zk_k_refine_split, egrid, dim3(64), 0, st, comp, comp_size, c_off, n, cnt, (const uint64_t *)base, fc, ent, first);
    // the pieces' sizes and verdicts: the stages of zk_frame_content_sizes_dev over the scratch table (the engine's dictionary applies there)
    if ((rc = zk_frame_content_sizes_dev(e, d_comp, comp_size, fc, 0, (uint32_t)total, sizes, fstat, st))) return rc;
    const dim3 fgrid((uint32_t)((total + 1 + 255) / 256));
    ZK_HIP(hipMemsetAsync(err, 0xFF, 8, st));
    hipLaunchKernelGGL(zk_k_refine_mark, fgrid, dim3(256), 0, st, (const int32_t *)fstat, (const uint32_t *)ent, (const uint64_t *)base, total, first);
    zk_launch_scan64(st, sizes, (uint32_t)total, szs);
    hipLaunchKernelGGL(zk_k_refine_fold, dim3((n + 255) / 256), dim3(256), 0, st, c_off, d_off, n, (const uint64_t *)base, (const uint64_t *)szs,
                       (const unsigned long long *)first, yields, ebytes, (int32_t *)d_entry_status, err);
    zk_launch_scan64(st, yields, n, obase);
    zk_launch_scan64(st, ebytes, n, dbase);
    ZK_HIP(hipMemcpyAsync(c.h_words + 12, obase + n, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(c.h_words + 13, err, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    const uint64_t yielded = c.h_words[12], first_err = c.h_words[13];
    *n_out = (uint32_t)yielded;
    if (yielded > out_cap) return -(int)ZK_E_DST_TOO_SMALL;
    hipLaunchKernelGGL(zk_k_refine_emit, fgrid, dim3(256), 0, st, c_off, d_off, n, (const uint64_t *)base, (const uint64_t *)fc, (const uint32_t *)ent,
                       (const uint64_t *)szs, (const uint64_t *)yields, (const uint64_t *)obase, (const uint64_t *)dbase, total,
                       (uint64_t *)d_c_out, (uint64_t *)d_d_out, (uint32_t *)d_entry_of);
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    return first_err == ~0ull ? 0 : -(int)(uint32_t)(first_err & 0xFFFFFFFFu);
}

// host pointers: comp[c_off[0] .. c_off[n_entries]) is uploaded; the arrays come back (c_out in the caller's own offsets)
extern "C" int zk_refine_entries(zk_engine *e, const uint8_t *comp, uint64_t comp_size, const uint64_t *c_off, const uint64_t *d_off, uint32_t n_entries,
                                 uint64_t *c_out, uint64_t *d_out, uint32_t *entry_of, uint32_t out_cap, uint32_t *n_out, int32_t *entry_status)
{
    if (!e || !n_out || (n_entries && (!comp || !c_off || !entry_status)) || (out_cap && (!c_out || !d_out))) return ZK_ERR_ARGUMENT;
    if (e->slot_busy[0]) return ZK_ERR_ARGUMENT;            // refused before the staging: its uploads ride on context 0's queue, behind the batch
    *n_out = 0;
    if (n_entries == 0) return 0;
    const uint32_t n = n_entries;
    const uint64_t lo = c_off[0], hi = c_off[n];
    if (hi < lo || hi > comp_size) return -(int)ZK_E_SRC_SIZE_WRONG;
    ZK_HIP(hipSetDevice(e->device));
    int rc;
    // offsets as staged: c_off relative to the uploaded bytes, then d_off as it is
    std::vector<uint64_t> offs((size_t)(n + 1) * (d_off ? 2 : 1));
    for (uint32_t i = 0; i <= n; i++) offs[i] = c_off[i] - lo;          // (an entry that leaves [lo, hi) wraps round and is refused as outside the buffer)
    if (d_off) memcpy(offs.data() + n + 1, d_off, (size_t)(n + 1) * 8);
    const size_t cap1 = (size_t)out_cap + 1;
    if ((rc = zk_devbuf_reserve(e, e->st_comp, (size_t)(hi - lo) + 64))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->st_off, offs.size() * 8))) return rc;
    if ((rc = zk_devbuf_reserve(e, e->st_misc, cap1 * 20 + (size_t)n * 4))) return rc;
    hipStream_t st = e->stream;
    ZK_HIP(hipMemsetAsync((uint8_t *)e->st_comp.p + (hi - lo), 0, 64, st));                  // readable padding behind the last frame
    ZK_HIP(hipMemcpyAsync(e->st_comp.p, comp + lo, hi - lo, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(e->st_off.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));                        // (offs is this call's own memory)
    uint64_t *dc = (uint64_t *)e->st_misc.p, *dd = dc + cap1;
    uint32_t *deo = (uint32_t *)(dd + cap1);
    int32_t *dst = (int32_t *)(deo + cap1);
    const uint64_t *s_c = (const uint64_t *)e->st_off.p;
    rc = zk_refine_entries_dev(e, e->st_comp.p, hi - lo, s_c, d_off ? s_c + n + 1 : nullptr, n, out_cap ? dc : nullptr, out_cap ? dd : nullptr,
                               out_cap ? deo : nullptr, out_cap, n_out, dst, nullptr);
    if (rc <= -1000 || *n_out == 0) return rc;              // an engine error: nothing came back
    ZK_HIP(hipMemcpy(entry_status, dst, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (*n_out > out_cap) return rc;                        // -70: nothing else is written
    const size_t m = *n_out;
    ZK_HIP(hipMemcpy(c_out, dc, (m + 1) * 8, hipMemcpyDeviceToHost));
    ZK_HIP(hipMemcpy(d_out, dd, (m + 1) * 8, hipMemcpyDeviceToHost));
    if (entry_of) ZK_HIP(hipMemcpy(entry_of, deo, m * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i <= m; i++) c_out[i] += lo;
    return rc;
}

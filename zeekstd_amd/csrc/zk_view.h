// zk_view.h -- byte ranges of a VIEW of a device-resident archive (zk_read_view_ranges_dev, include/zeekstd_amd.h "THE RULE"): the
// kernels (included by zk_view.hip, which keeps their launchers; tests/sim/zk_view_sim.cpp runs the same source on the CPU under the workgroup
// emulator, against the model of tests/helpers/view_model.py).  A view is ids[vcount] (archive frames) and voff[vcount + 1] (where the entries
// lie in the view's stream): the stream is a permutation-with-repeats of the archive's frames, so what one decode pass holds of a range is not
// one stretch of the scratch, as it is for zk_read_ranges_dev (zk_k_range_pieces), but a piece per entry, anywhere in it.
//   zk_k_view_check    a lane per entry: id < n_frames, voff non-decreasing, the entry's size == the frame's; an atomic OR into one error word
//   zk_k_view_lens     (packed destinations only) the bytes each range will deliver; zk_k_scan64 turns them into destinations
//   zk_k_view_plan     a lane per range: validation (off >= voff[0] FIRST: zkr_frame_of assumes it), first / last ENTRY by binary search of voff,
//                      +1 / -1 in a difference array over the entries AND in its sums over segments of 64 and of 4096 entries (where the two
//                      do not fall into one cell and cancel) -- O(1) per range however many entries it crosses --, and the number of 64 KiB
//                      chunks its destination is dealt in
//   zk_k_view_bases    a lane per segment of 64 entries: the ranges that cover the entries in front of it (<= 63 + vcount / 4096 additions)
//   zk_k_view_mark     a lane per entry: its coverage (<= 64 additions); a covered, non-empty entry adds its frame to the difference array over
//                      the archive's FRAMES (+1 at id, -1 at id + 1).  From there zk_k_range_compact (zk_ranges.hip) gives the sorted list of
//                      distinct frames, the prefix sums of their sizes and frame -> slot, as it does for zk_read_ranges_dev
//   zk_k_view_gather   per decode pass [a, b) of that list, scratch -> destination, divided by DESTINATION bytes: a wave per small range, a
//                      workgroup per 64 KiB chunk (on the destination's 16-byte grid) of a large one.  Either finds its first entry -- the
//                      range's, or by binary search of voff -- and walks the entries that meet its bytes; an entry whose frame's slot lies in
//                      [a, b) is copied from scratch + uoff[slot] - uoff[a] + (lo - voff[j]) by zk_range_copy.  No list of pieces exists.
//   zk_k_view_status   a lane per range: its own validation code, or the first failing frame, in view order, among the entries it touches
//                      (walked only when some frame failed at all)
// Every write is a vector store or a vector atomic.  No barrier and no wave collective: no lane waits for another.
#pragma once
#include <stdint.h>
#include "zk_ranges.h"
#include "zk_range_copy.h"

constexpr uint32_t ZKV_THREADS = 256;
constexpr uint64_t ZKV_SMALL = 16u << 10;                   // ZK_RANGE_SMALL: ranges up to here are a wave's
constexpr uint64_t ZKV_CHUNK = 64u << 10;                   // ZK_RANGE_CHUNK: destination bytes a workgroup takes at a time
constexpr uint32_t ZKV_SEG = 64;                            // entries per segment; ZKV_SEG segments per super-segment
constexpr uint32_t ZKV_GRID_MAX = 4096;                     // chunk workgroups of zk_k_view_gather: more chunks are strided over
enum { ZKV_ERR_ID = 1, ZKV_ERR_ORDER = 2, ZKV_ERR_SIZE = 4 };
enum { ZKV_W_FRAMES = 0, ZKV_W_BYTES, ZKV_W_VIEW_ERR, ZKV_W_FIRST_ERR, ZKV_W_WORDS };   // the words the host reads ([0], [1]: zk_k_range_compact's)

ZKR_HD uint32_t zkv_blocks(uint64_t items) { return (uint32_t)((items + ZKV_THREADS - 1) / ZKV_THREADS); }
ZKR_HD uint32_t zkv_nseg(uint32_t vcount) { return (uint32_t)(((uint64_t)vcount + 1) / ZKV_SEG + 1); }                       // segments over vcount + 2 cells
ZKR_HD uint32_t zkv_nsuper(uint32_t vcount) { return (uint32_t)(((uint64_t)vcount + 1) / (ZKV_SEG * ZKV_SEG) + 1); }
// the gather's grid: a workgroup per four ranges (a wave each) and the chunk workgroups behind them.  A valid range's chunks: at most
// len / ZKV_CHUNK + 2 with len <= dst_cap
ZKR_HD uint32_t zkv_small_wgs(uint32_t count) { return (uint32_t)(((uint64_t)count + 3) / 4); }
ZKR_HD uint32_t zkv_chunk_wgs(uint32_t count, uint64_t dst_cap)
{
    const uint64_t most = dst_cap / ZKV_CHUNK + 2 * (uint64_t)count;
    return most > ZKV_GRID_MAX ? ZKV_GRID_MAX : (uint32_t)most;
}
// The plan's arrays, in entries (the engine carves them out of one allocation, the emulator harness allocates each exactly):
//   per range   eff | cnt (count), packed | coff (count + 1: zk_k_scan64 leaves the total behind the sums), efirst | elast | status (count)
//   per entry   ecover (vcount + 2), seg (zkv_nseg), super (zkv_nsuper), ebase (zkv_nseg)
//   per frame   fcover (n_frames + 2), slot | uids | fstat (n_frames + 1), uoff | poff (n_frames + 1)
// ecover | seg | super | fcover are cleared together before the plan
struct ZkViewSizes { size_t eff, cnt, packed, coff, efirst, elast, status, ecover, seg, super, ebase, fcover, slot, uids, fstat, uoff, poff; };
ZKR_HD ZkViewSizes zkv_sizes(uint32_t count, uint32_t vcount, uint32_t n_frames)
{
    ZkViewSizes s;
    const size_t n = count, f = n_frames;
    s.eff = n; s.cnt = n; s.packed = n + 1; s.coff = n + 1; s.efirst = n; s.elast = n; s.status = n;
    s.ecover = (size_t)vcount + 2; s.seg = zkv_nseg(vcount); s.super = zkv_nsuper(vcount); s.ebase = zkv_nseg(vcount);
    s.fcover = f + 2; s.slot = f + 1; s.uids = f + 1; s.fstat = f + 1; s.uoff = f + 1; s.poff = f + 1;
    return s;
}

// One range against the view's stream [v0, vend]: inside it, and off + len without overflow.  off < v0 is refused HERE, before any search
ZKR_HD int32_t zkv_check_src(uint64_t v0, uint64_t vend, uint64_t off, uint64_t len)
{
    return (off < v0 || off > vend || len > vend - off) ? ZKR_E_OFFSET_OUT_OF_RANGE : ZKR_OK;
}
ZKR_HD int32_t zkv_check(uint64_t v0, uint64_t vend, uint64_t off, uint64_t len, uint64_t dst_cap, uint64_t dst_off)
{
    const int32_t s = zkv_check_src(v0, vend, off, len);
    return s ? s : zkr_check_dst(dst_cap, dst_off, len);
}
// chunks of a range of len bytes whose destination begins at address dst: cut on the destination's 16-byte grid, so that only the range's own
// two ends are ragged; chunk k holds the range's bytes [zkv_chunk_begin, zkv_chunk_end)
ZKR_HD uint64_t zkv_chunks(uint64_t len, uintptr_t dst) { return len > ZKV_SMALL ? (len + (dst & 15) + ZKV_CHUNK - 1) / ZKV_CHUNK : 0; }
ZKR_HD uint64_t zkv_chunk_begin(uint64_t k, uintptr_t dst) { return k ? k * ZKV_CHUNK - (dst & 15) : 0; }
ZKR_HD uint64_t zkv_chunk_end(uint64_t k, uintptr_t dst, uint64_t len) { const uint64_t e = (k + 1) * ZKV_CHUNK - (dst & 15); return e < len ? e : len; }

__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_check(const uint64_t *d_off, uint32_t n_frames, const uint32_t *ids, const uint64_t *voff, uint32_t vcount,
                                                               uint32_t *err)
{
    const uint32_t j = blockIdx.x * ZKV_THREADS + threadIdx.x;
    if (j >= vcount) return;
    const uint32_t id = ids[j];
    const uint64_t v0 = voff[j], v1 = voff[j + 1];
    uint32_t bad = 0;
    if (v1 < v0) bad |= ZKV_ERR_ORDER;
    if (id >= n_frames) bad |= ZKV_ERR_ID;
    else if (v1 - v0 != d_off[id + 1] - d_off[id]) bad |= ZKV_ERR_SIZE;
    if (bad) atomicOr(err, bad);
}

__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_lens(const uint64_t *voff, uint32_t vcount, const uint64_t *offs, const uint64_t *lens, uint32_t count,
                                                              uint64_t *eff)
{
    const uint32_t i = blockIdx.x * ZKV_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint64_t len = lens[i];
    eff[i] = zkv_check_src(voff[0], voff[vcount], offs[i], len) == ZKR_OK ? len : 0;     // a range outside the stream takes no room
}

// ecover (vcount + 2 cells), seg and super (their sums over 64 and 4096 cells) must be zero.  efirst / elast: ~0 for a range that copies nothing
__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_plan(const uint64_t *voff, uint32_t vcount, const uint64_t *offs, const uint64_t *lens, const uint64_t *dst_off,
                                                              uint32_t count, uint64_t dst_cap, uintptr_t dst_base, uint32_t *efirst, uint32_t *elast, int32_t *status,
                                                              uint32_t *ecover, uint32_t *seg, uint32_t *super, uint64_t *cnt)
{
    const uint32_t i = blockIdx.x * ZKV_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint64_t off = offs[i], len = lens[i], to = dst_off[i];
    const int32_t st = zkv_check(voff[0], voff[vcount], off, len, dst_cap, to);
    uint32_t first = ~0u, last = ~0u;
    if (st == ZKR_OK && zkr_span(voff, vcount, off, len, &first, &last)) {
        const uint32_t z = last + 1;                    // (-1: the sums wrap back)
        atomicAdd(&ecover[first], 1u);
        atomicAdd(&ecover[z], ~0u);
        // a +1 and a -1 in the same cell of the sums cancel: many short ranges do not all meet in the few cells of seg and super
        if (first / ZKV_SEG != z / ZKV_SEG) { atomicAdd(&seg[first / ZKV_SEG], 1u); atomicAdd(&seg[z / ZKV_SEG], ~0u); }
        if (first / (ZKV_SEG * ZKV_SEG) != z / (ZKV_SEG * ZKV_SEG)) { atomicAdd(&super[first / (ZKV_SEG * ZKV_SEG)], 1u); atomicAdd(&super[z / (ZKV_SEG * ZKV_SEG)], ~0u); }
    }
    efirst[i] = first; elast[i] = last;
    status[i] = st;
    cnt[i] = first != ~0u ? zkv_chunks(len, dst_base + to) : 0;
}

// ebase[s] = the sum of ecover over the cells in front of segment s
__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_bases(const uint32_t *seg, const uint32_t *super, uint32_t nseg, uint32_t *ebase)
{
    const uint32_t s = blockIdx.x * ZKV_THREADS + threadIdx.x;
    if (s >= nseg) return;
    uint32_t x = 0;
    for (uint32_t u = 0; u < s / ZKV_SEG; u++) x += super[u];
    for (uint32_t t = s / ZKV_SEG * ZKV_SEG; t < s; t++) x += seg[t];
    ebase[s] = x;
}

// (behind zk_k_view_check: nothing is marked when the view is refused, and no id is used unchecked)  fcover: n_frames + 2 cells, zero
__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_mark(const uint32_t *ids, const uint64_t *voff, uint32_t vcount, const uint32_t *ecover, const uint32_t *ebase,
                                                              const uint32_t *err, uint32_t *fcover)
{
    const uint32_t j = blockIdx.x * ZKV_THREADS + threadIdx.x;
    if (j >= vcount || *err != 0) return;
    uint32_t cov = ebase[j / ZKV_SEG];
    for (uint32_t t = j / ZKV_SEG * ZKV_SEG; t <= j; t++) cov += ecover[t];
    if (cov == 0 || voff[j + 1] == voff[j]) return;
    const uint32_t id = ids[j];
    atomicAdd(&fcover[id], 1u);
    atomicAdd(&fcover[id + 1], ~0u);
}

// The bytes [lo, hi) of the view's stream (lo < hi, inside a valid range) -> out (where the byte at lo goes), by T lanes: from the entry j that
// holds lo on, every entry that meets them.  The pass holds slots [a, b) of the distinct frames, packed at scratch + (uoff[s] - uoff[a])
template <uint32_t T> __device__ __forceinline__ void zkv_walk(const uint8_t *scratch, uint8_t *out, const uint32_t *ids, const uint64_t *voff, uint32_t vcount, uint32_t j,
                                                               uint64_t lo, uint64_t hi, const uint32_t *slot, const uint64_t *uoff, uint32_t a, uint32_t b, uint32_t t)
{
    const uint64_t base = uoff[a];
    for (; j < vcount; j++) {
        const uint64_t e0 = voff[j];
        if (e0 >= hi) break;
        const uint64_t e1 = voff[j + 1];
        const uint64_t p0 = e0 > lo ? e0 : lo, p1 = e1 < hi ? e1 : hi;
        if (p1 <= p0) continue;                         // (an empty entry)
        const uint32_t s = slot[ids[j]];
        if (s >= a && s < b) zk_range_copy<T>(out + (p0 - lo), scratch + (uoff[s] - base) + (p0 - e0), p1 - p0, t);
    }
}

// Workgroups [0, small_wgs): four waves, a small range each.  The others: the 64 KiB chunks of the large ranges, dealt round robin; coff (the
// prefix sums of the ranges' chunk counts, the total at [count]) says whose chunk a number is.  status: the validation codes of zk_k_view_plan
__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_gather(const uint8_t *scratch, uint8_t *dst, const uint32_t *ids, const uint64_t *voff, uint32_t vcount,
                                                                const uint64_t *offs, const uint64_t *lens, const uint64_t *dst_off, const uint32_t *efirst,
                                                                const uint64_t *coff, uint32_t count, const uint32_t *slot, const uint64_t *uoff, uint32_t a, uint32_t b,
                                                                uint32_t small_wgs)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < small_wgs) {
        const uint64_t i = (uint64_t)blockIdx.x * 4 + (tid >> 6);
        if (i >= count) return;
        const uint32_t first = efirst[i];
        const uint64_t len = lens[i];
        if (first == ~0u || len > ZKV_SMALL) return;
        const uint64_t off = offs[i];
        zkv_walk<64>(scratch, dst + dst_off[i], ids, voff, vcount, first, off, off + len, slot, uoff, a, b, tid & 63);
        return;
    }
    const uint64_t total = coff[count];
    for (uint64_t k = blockIdx.x - small_wgs; k < total; k += gridDim.x - small_wgs) {
        uint32_t r = 0, above = count;                  // the last range with coff[r] <= k (ranges without chunks share their successor's entry)
        while (above - r > 1) { const uint32_t mid = r + ((above - r) >> 1); if (coff[mid] <= k) r = mid; else above = mid; }
        const uint64_t off = offs[r], len = lens[r];
        uint8_t *to = dst + dst_off[r];
        const uint64_t c = k - coff[r];
        const uint64_t b0 = zkv_chunk_begin(c, (uintptr_t)to), b1 = zkv_chunk_end(c, (uintptr_t)to, len);
        if (b0 >= b1) continue;
        const uint32_t j = c ? zkr_frame_of(voff, vcount, off + b0) : efirst[r];
        zkv_walk<ZKV_THREADS>(scratch, to + b0, ids, voff, vcount, j, off + b0, off + b1, slot, uoff, a, b, tid);
    }
}

// fstat[s]: the ZSTD_ErrorCode of distinct frame s (0 = fine).  The entries of a range are looked at only when some frame failed at all
// (any_failed, or *pass_err != ~0: the first-error word of the decode pass still in flight).  status -> out (which may be the same array)
__global__ __launch_bounds__(ZKV_THREADS) void zk_k_view_status(const uint32_t *ids, const uint64_t *voff, uint32_t count, const uint32_t *efirst, const uint32_t *elast,
                                                                const uint32_t *slot, const int32_t *fstat, int any_failed, const uint64_t *pass_err,
                                                                const int32_t *status, int32_t *out, unsigned long long *first_err)
{
    const uint32_t i = blockIdx.x * ZKV_THREADS + threadIdx.x;
    if (i >= count) return;
    int32_t st = status[i];
    const uint32_t first = efirst[i];
    if (st == ZKR_OK && first != ~0u && (any_failed || (pass_err && *pass_err != ~0ull))) {
        const uint32_t last = elast[i];
        for (uint32_t j = first; j <= last && st == ZKR_OK; j++)
            if (voff[j + 1] != voff[j]) st = -fstat[slot[ids[j]]];
    }
    out[i] = st;
    if (st != ZKR_OK) atomicMin(first_err, ((unsigned long long)i << 32) | (uint32_t)(-st));
}

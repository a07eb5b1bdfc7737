// zk_compact.h -- frames removed from a device-resident archive: the kernels of zk_mark_frames_dev, zk_compact_archive_dev, zk_remap_ids_dev and
// zk_dedup_index_compact_dev (included by zk_compact.hip, which keeps their launchers; tests/sim/zk_compact_sim.cpp runs the same source on
// the CPU under the workgroup emulator, against the model of tests/helpers/compact_model.py).  The rule (include/zeekstd_amd.h),
// for an archive of n frames and live[n]:
//   kept      the s with live[s] != 0, ascending;  remap[s] = the position of s in kept, or ZKC_REMOVED
//   c_off_out / d_off_out    c_off[0] / d_off[0] and the prefix sums of the kept frames' sizes behind them
//   dst[c_off_out[k], c_off_out[k + 1])  the bytes of frame kept[k];  written = c_off_out[n_kept]
// No frame is decoded: bytes move, nothing looks inside them.
//   zk_k_cmp_check_ids / zk_k_cmp_mark     a lane per id: ids at or above n_frames are an atomic OR into one error word; live[id] = 1
//   zk_k_cmp_flags      a lane per frame (and one for the end, s = n): keep | head << 32, the kept sizes; a decreasing offset is an error bit
//   (zk_k_scan64        zk_encode.hip's, three times: kept count | run number, compressed and decompressed positions)
//   zk_k_cmp_emit       a lane per frame: remap, c_off_out, d_off_out (into scratch: the entry point copies them out once nothing can refuse
//                       the call any more), the RUN TABLE and the totals the host reads
//   zk_k_cmp_move       the bytes.  A RUN is a maximal stretch of consecutive kept frames: contiguous in the source and in the destination, one
//                       extent however many frames it holds.  The work is cut by DESTINATION bytes: workgroup t owns tile
//                       [lo + t * ZKC_TILE, lo + (t + 1) * ZKC_TILE) of the moved range [lo, hi) (and strides over the tiles when there are
//                       more than the grid), finds the run of its first byte by binary search over the runs' destinations and walks the
//                       runs that meet the tile.  Every meeting: up to 15 bytes one by one until the destination is 16-byte aligned,
//                       aligned 16-byte stores fed by 16-byte loads at whatever alignment the source has, four per lane in flight, the
//                       last bytes one by one.  Nothing is loaded outside a kept frame, nothing stored outside [lo, hi)
//   zk_k_cmp_remap_ids  a lane per id: remap[ids[i]] (into scratch); an id out of range or removed is an error bit
//   zk_k_cmp_remap_check / zk_k_cmp_take   the index: is remap what a compaction leaves (kept frames numbered 0, 1, ... in order)?  Then
//                       keys_out[remap[s]] = keys[s], lens_out[remap[s]] = lens[s]
// IN PLACE (dst == src): every kept byte moves toward lower addresses, and the gap src - dst at a destination byte -- the bytes removed
// before it -- never decreases.  The moved range begins at the first removed frame and is done in STEPS of whole tiles, in stream order
// (zkc_step_bytes, zkc_nsteps, zkc_step_begin / _end); a step whose gap at its first byte is at least its length reads nothing below its own
// destination end and goes source -> destination DIRECTLY; any other step is STAGED: moved into scratch, then copied to its place
// (zkc_step_direct).  Either way a step writes [a, b) only and every later step reads at or above b.
// Every write is a vector store or a vector atomic.  Plain C++ only: no barrier, and no lane waits for another.
#pragma once
#include <stdint.h>
#include <string.h>
#include "zk_device.h"

constexpr uint32_t ZKC_THREADS = 256;
constexpr uint32_t ZKC_TILE = 64u << 10;                    // destination bytes a workgroup of zk_k_cmp_move takes at a time
constexpr uint32_t ZKC_GRID_MAX = 1u << 16;                 // its workgroups: more tiles are strided over
constexpr uint32_t ZKC_REMOVED = 0xFFFFFFFFu;               // remap[] of a removed frame (ZK_FRAME_REMOVED)
constexpr uint64_t ZKC_SLICE_BYTES = 1ull << 28;            // ZK_CHOICE_COMPACT_SLICE_KIB's default
enum { ZKC_ERR_ID = 1, ZKC_ERR_ORDER = 2, ZKC_ERR_REMOVED = 4, ZKC_ERR_REMAP = 8 };
// the words zk_k_cmp_emit leaves for the host
enum { ZKC_W_ERR = 0, ZKC_W_KEPT, ZKC_W_RUNS, ZKC_W_BEGIN, ZKC_W_WRITTEN, ZKC_W_END, ZKC_W_FIRST_REMOVED, ZKC_W_WORDS = 8 };

ZK_HD uint32_t zkc_blocks(uint64_t items) { return (uint32_t)((items + ZKC_THREADS - 1) / ZKC_THREADS); }

// ---- the plan of an in-place compaction (the engine, the launchers and the emulator harness all call these)
// destination bytes per step: `slice` bytes (0 = the default) in whole tiles, one at least
ZK_HD uint64_t zkc_step_bytes(uint64_t slice)
{
    const uint64_t s = (slice ? slice : ZKC_SLICE_BYTES) / ZKC_TILE * ZKC_TILE;
    return s ? s : ZKC_TILE;
}
// the steps of `moved` bytes: step k is [zkc_step_begin, zkc_step_end) of the moved range, the last one short
ZK_HD uint64_t zkc_nsteps(uint64_t moved, uint64_t step) { return (moved + step - 1) / step; }
ZK_HD uint64_t zkc_step_begin(uint64_t k, uint64_t step) { return k * step; }
ZK_HD uint64_t zkc_step_end(uint64_t k, uint64_t step, uint64_t moved) { return (k + 1) * step < moved ? (k + 1) * step : moved; }
// may a step go source -> destination directly?  removed_before_step: the gap src - dst at the step's first destination byte.  The gap never
// decreases, so every byte the step reads lies at or above (its first byte + the gap): at or above its own end when gap >= length
ZK_HD bool zkc_step_direct(uint64_t removed_before_step, uint64_t step_bytes) { return removed_before_step >= step_bytes; }
// scratch a staged step needs: no more than the longest step
ZK_HD uint64_t zkc_stage_bytes(uint64_t moved, uint64_t step) { return moved < step ? moved : step; }
// zk_k_cmp_move's workgroups for `bytes` destination bytes
ZK_HD uint32_t zkc_move_grid(uint64_t bytes)
{
    const uint64_t tiles = (bytes + ZKC_TILE - 1) / ZKC_TILE;
    return tiles < 1 ? 1 : tiles > ZKC_GRID_MAX ? ZKC_GRID_MAX : (uint32_t)tiles;
}
// The scratch of one compaction of n frames, in bytes from its start (the emulator harness allocates the same):
// fk | pk | fc | pc | fd | pd (the flags and their scans: n + 1 values, n + 2 results) | co | dof (n + 1) | rsrc | rdst (n + 2: at most (n + 1) / 2
// runs and the end behind them) | remap (n) | words
struct ZkCmpLayout { size_t fk, pk, fc, pc, fd, pd, co, dof, rsrc, rdst, remap, words, end; };
ZK_HD ZkCmpLayout zkc_layout(uint32_t n)
{
    ZkCmpLayout L;
    const size_t a = 8 * ((size_t)n + 2);
    L.fk = 0; L.pk = L.fk + a; L.fc = L.pk + a; L.pc = L.fc + a; L.fd = L.pc + a; L.pd = L.fd + a;
    L.co = L.pd + a; L.dof = L.co + a; L.rsrc = L.dof + a; L.rdst = L.rsrc + a;
    L.remap = L.rdst + a;
    L.words = (L.remap + 4 * (size_t)n + 15) & ~(size_t)15;
    L.end = L.words + 8 * ZKC_W_WORDS;
    return L;
}

// err |= ZKC_ERR_ID when an id is at or above n_frames
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_check_ids(const uint32_t *ids, uint32_t count, uint32_t n_frames, uint32_t *err)
{
    const uint32_t i = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (i < count && ids[i] >= n_frames) atomicOr(err, (uint32_t)ZKC_ERR_ID);
}
// (behind zk_k_cmp_check_ids: every id is below n_frames)
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_mark(const uint32_t *ids, uint32_t count, uint8_t *live)
{
    const uint32_t i = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (i < count) live[ids[i]] = 1;
}

// s <= n.  fk[s] = keep | head << 32 (head: a kept frame whose predecessor is not kept), fc / fd: the kept frame's sizes; all 0 for s == n, so
// that the scans of n + 1 values leave the totals at [n].  A decreasing offset: err |= ZKC_ERR_ORDER
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_flags(const uint64_t *c_off, const uint64_t *d_off, const uint8_t *live, uint32_t n, uint64_t *fk,
                                                              uint64_t *fc, uint64_t *fd, uint32_t *err)
{
    const uint32_t s = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (s > n) return;
    if (s == n) { fk[s] = 0; fc[s] = 0; fd[s] = 0; return; }
    const uint64_t c0 = c_off[s], c1 = c_off[s + 1], d0 = d_off[s], d1 = d_off[s + 1];
    if (c1 < c0 || d1 < d0) atomicOr(err, (uint32_t)ZKC_ERR_ORDER);
    const bool keep = live[s] != 0, head = keep && (s == 0 || live[s - 1] == 0);
    fk[s] = (uint64_t)keep | (uint64_t)head << 32;
    fc[s] = keep ? c1 - c0 : 0;
    fd[s] = keep ? d1 - d0 : 0;
}

// s <= n, behind the scans pk / pc / pd of fk / fc / fd.  Positions are counted as the offsets are: from the first byte of the buffers.
//   remap[s]; co[k] / dof[k] for the k-th kept frame and, from the lane s == n, the end co[n_kept] / dof[n_kept]
//   rsrc[r] / rdst[r] of run r from its head, rdst[n_runs] = the end
//   words: the totals, and ZKC_W_FIRST_REMOVED = the offset of the first removed frame (the end when none is) -- where an in-place
//   compaction begins to move
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_emit(const uint64_t *c_off, const uint64_t *d_off, uint32_t n, const uint64_t *fk, const uint64_t *pk,
                                                             const uint64_t *pc, const uint64_t *pd, uint32_t *remap, uint64_t *co, uint64_t *dof, uint64_t *rsrc,
                                                             uint64_t *rdst, uint64_t *words)
{
    const uint32_t s = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (s > n) return;
    const uint64_t c_base = c_off[0], d_base = d_off[0];
    const uint32_t k = (uint32_t)pk[s], r = (uint32_t)(pk[s] >> 32);
    const uint64_t f = s < n ? fk[s] : 0;
    const bool keep = (f & 1u) != 0, head = (f >> 32) != 0;
    if (s < n) remap[s] = keep ? k : ZKC_REMOVED;
    if (keep || s == n) { co[k] = c_base + pc[s]; dof[k] = d_base + pd[s]; }
    if (head) { rsrc[r] = c_off[s]; rdst[r] = c_base + pc[s]; }
    if (!keep && k == s) words[ZKC_W_FIRST_REMOVED] = c_off[s];                   // every frame before s is kept and s is not: one lane
    if (s == n) {
        rdst[r] = c_base + pc[s];
        words[ZKC_W_KEPT] = k; words[ZKC_W_RUNS] = r;
        words[ZKC_W_BEGIN] = c_base; words[ZKC_W_WRITTEN] = c_base + pc[s]; words[ZKC_W_END] = c_off[n];
    }
}

// n bytes by the lanes of a workgroup; the stores: [to, to + n) and nothing else, the loads: [from, from + n)
__device__ __forceinline__ void zkc_copy_wg(uint8_t *to, const uint8_t *from, uint32_t n, uint32_t tid)
{
    const uint32_t to16 = (16u - (uint32_t)((uintptr_t)to & 15u)) & 15u, head = to16 < n ? to16 : n;
    const uint32_t nq = (n - head) >> 4, tail = head + 16 * nq;
    if (tid < head) to[tid] = from[tid];
    const uint8_t *f = from + head;
    uint8_t *t = to + head;
    for (uint32_t q0 = 0; q0 < nq; q0 += 4 * ZKC_THREADS) {
        uint4 v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t q = q0 + j * ZKC_THREADS + tid;
            if (q < nq) memcpy(&v[j], f + 16 * (size_t)q, 16);                    // any alignment
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t q = q0 + j * ZKC_THREADS + tid;
            if (q < nq) *(uint4 *)(t + 16 * (size_t)q) = v[j];                    // aligned
        }
    }
    if (tail + tid < n) to[tail + tid] = from[tail + tid];
}

// The destination bytes [lo, hi) (positions as the offsets count them): the byte at p is stored at out[p - obase] -- out = the destination
// and obase = 0, or out = the staging scratch and obase = lo -- and comes from src[rsrc[r] + (p - rdst[r])], r its run.  rdst[0] <= lo,
// rdst[nruns] >= hi, nruns > 0
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_move(const uint8_t *src, uint8_t *out, uint64_t obase, const uint64_t *rsrc, const uint64_t *rdst,
                                                             uint32_t nruns, uint64_t lo, uint64_t hi)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (hi - lo + ZKC_TILE - 1) / ZKC_TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t a = lo + t * ZKC_TILE, b = hi - a < ZKC_TILE ? hi : a + ZKC_TILE;
        // the last run that begins at or before a (runs without bytes share their successor's beginning: the last of them has the bytes)
        uint32_t r = 0, above = nruns;
        while (above - r > 1) {
            const uint32_t mid = r + (above - r) / 2;
            if (rdst[mid] <= a) r = mid; else above = mid;
        }
        for (; r < nruns; r++) {
            const uint64_t r0 = rdst[r], r1 = rdst[r + 1];
            if (r0 >= b) break;
            const uint64_t e0 = r0 > a ? r0 : a, e1 = r1 < b ? r1 : b;
            if (e1 > e0) zkc_copy_wg(out + (e0 - obase), src + rsrc[r] + (e0 - r0), (uint32_t)(e1 - e0), tid);
        }
    }
}

// (behind zk_k_cmp_emit) gaps[k] = src - dst at the first destination byte of step k of an in-place compaction -- what zkc_step_direct is
// asked with --, 0 for a k beyond the last step.  The steps: zkc_step_begin(k, step) from words[ZKC_W_FIRST_REMOVED]
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_step_gaps(const uint64_t *rsrc, const uint64_t *rdst, const uint64_t *words, uint64_t step, uint32_t max_steps,
                                                                  uint64_t *gaps)
{
    const uint32_t k = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (k >= max_steps) return;
    const uint32_t nruns = (uint32_t)words[ZKC_W_RUNS];
    const uint64_t lo = words[ZKC_W_FIRST_REMOVED], hi = words[ZKC_W_WRITTEN];
    uint64_t gap = 0;
    if (nruns && lo < hi && zkc_step_begin(k, step) < hi - lo) {
        const uint64_t p = lo + zkc_step_begin(k, step);
        uint32_t r = 0, above = nruns;
        while (above - r > 1) {
            const uint32_t mid = r + (above - r) / 2;
            if (rdst[mid] <= p) r = mid; else above = mid;
        }
        gap = rsrc[r] - rdst[r];
    }
    gaps[k] = gap;
}

// out[i] = remap[ids[i]]; an id at or above n_frames: err |= ZKC_ERR_ID, a removed frame: err |= ZKC_ERR_REMOVED
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_remap_ids(const uint32_t *remap, uint32_t n_frames, const uint32_t *ids, uint32_t count, uint32_t *out,
                                                                  uint32_t *err)
{
    const uint32_t i = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t id = ids[i];
    if (id >= n_frames) { atomicOr(err, (uint32_t)ZKC_ERR_ID); return; }
    const uint32_t to = remap[id];
    if (to == ZKC_REMOVED) { atomicOr(err, (uint32_t)ZKC_ERR_REMOVED); return; }
    out[i] = to;
}

// the index: flags[s] = frame s is kept (s <= n; 0 for s == n), then -- behind the scan pos of the flags -- is remap what zk_k_cmp_emit leaves?
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_remap_flags(const uint32_t *remap, uint32_t n, uint64_t *flags)
{
    const uint32_t s = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (s <= n) flags[s] = s < n && remap[s] != ZKC_REMOVED;
}
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_remap_check(const uint32_t *remap, uint32_t n, const uint64_t *pos, uint32_t *err)
{
    const uint32_t s = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (s < n && remap[s] != ZKC_REMOVED && remap[s] != (uint32_t)pos[s]) atomicOr(err, (uint32_t)ZKC_ERR_REMAP);
}
// keys_out[remap[s]] = keys[s], lens_out[remap[s]] = lens[s] for the kept frames (remap checked: the places are distinct and below n_kept)
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cmp_take(const uint32_t *remap, uint32_t n, const uint64_t *keys, const uint32_t *lens, uint64_t *keys_out,
                                                             uint32_t *lens_out)
{
    const uint32_t s = blockIdx.x * ZKC_THREADS + threadIdx.x;
    if (s >= n) return;
    const uint32_t to = remap[s];
    if (to == ZKC_REMOVED) return;
    keys_out[to] = keys[s];
    lens_out[to] = lens[s];
}

// zk_cdc.h -- content-defined frame boundaries on the device: the kernels of zk_chunk_boundaries[_dev] (included by zk_cdc.hip, which keeps
// their launchers; tests/sim/zk_cdc_sim.cpp runs the same source on the CPU under the workgroup emulator, against the numpy model of
// tests/helpers/cdc_model.py).  The rule (include/zeekstd_amd.h):
//   G[b]      a 32-bit mix of b + 1 (zkc_gear)
//   h(p)      sum over j = 0..31 of G[src[p - j]] << j, mod 2^32, terms before the first byte absent: the gear recurrence
//             h = (h << 1) + G[byte], which forgets a byte after 32 steps -- every position is hashed on its own from the 31 bytes before it
//   candidate p with h(p) >> (32 - bits) == 0, bits = log2(avg_size); it offers the cut q = p + 1
//   selection from a cut c < n: the smallest candidate offset in [c + min, min(c + max, n)], else min(c + max, n); the chain ends at n
// The input is worked on in SLICES of at most ZK_CHOICE_CDC_SLICE_KIB (all scratch is sized by the slice, not by n), a slice in tiles of
// ZKC_TILE positions:
//   zk_k_cdc_mark     a workgroup per tile: the tile and the 31 bytes before it staged in LDS (aligned 16-byte loads, the unaligned head and
//                     tail of the source byte by byte), every lane rolls over ZKC_RUN consecutive positions after warming up on the 31 bytes
//                     before them, keeps its candidate bits in registers and stores them as one 16-byte word; the tile's number of
//                     candidates goes to counts[tile]
//   (zk_k_scan64      zk_encode.hip's: where each tile's candidates go in the list)
//   zk_k_cdc_emit     a workgroup per tile: the bitmap's set bits as a sorted list of slice-relative positions
//   the selection     zkc_walk: ONE wave walks a chain of cuts over the slice's list, streamed through LDS; it takes a step per frame (64
//                     entries held in registers, a lane each: a ballot finds the first one at or behind c + min and a readlane fetches it, so
//                     a step reads no memory; a binary search in the chunk when there is none among them -- the dense case, a run that makes
//                     every position a candidate).  A slice of one segment (zkc_segs) is walked by zk_k_cdc_select alone.  A longer one
//                     by a wave per segment side by side, each on a speculative chain from its segment's first candidate
//                     (zk_k_cdc_spec), then by one wave on the true chain, which adopts a segment's chain from the first cut they share
//                     (zk_k_cdc_fix; zk_k_cdc_copy writes what it adopted).  The chain's cut and count live in device memory
//                     (ZkCdcState) and are carried from slice to slice: a slice decides every cut whose whole range
//                     [c + min, min(c + max, n)] it has seen.
// Bits of the bitmap: position s0 + i of the slice is bit i & 31 of dword i >> 5.  Plain C++ and wave intrinsics only.
#pragma once
#include <stdint.h>
#include "zk_device.h"

constexpr uint32_t ZKC_THREADS = 256;
constexpr uint32_t ZKC_RUN = 128;                           // positions per lane: 31 warm-up steps on 128, 24 % redundant
constexpr uint32_t ZKC_TILE = ZKC_THREADS * ZKC_RUN;        // positions per workgroup of zk_k_cdc_mark / zk_k_cdc_emit
constexpr uint32_t ZKC_LEAD = 31;                           // bytes before a position that its hash reads
constexpr uint32_t ZKC_CHUNK = 8192;                        // list entries zk_k_cdc_select holds in LDS at a time
constexpr uint32_t ZKC_SEL_THREADS = 64;                    // ... one wave
constexpr uint32_t ZKC_STEPS = ZKC_LEAD + ZKC_RUN;          // 159 steps of the recurrence per lane ...
constexpr uint32_t ZKC_DWORDS = (ZKC_STEPS + 3) / 4;        // ... out of 40 dwords, realigned from 41
// The staged tile: LDS byte x holds the byte at address A0 - 32 + x, A0 = the address of the tile's first staged byte rounded down to 16,
// so that an aligned 16-byte load goes to LDS as it is.  A lane's run starts ZKC_RUN bytes behind its neighbour's: logical dword w lies
// at dword w + (w >> 5), which makes that 33 dwords -- the 32 lanes that share an LDS cycle read 32 different banks.
constexpr uint32_t ZKC_LDS_LOGICAL = (32 + 15 + ZKC_LEAD + ZKC_TILE + 3) / 4 + 2;        // dwords a tile's lanes may read (the last lane's 41st included)
constexpr uint32_t ZKC_LDS_DWORDS = ZKC_LDS_LOGICAL + (ZKC_LDS_LOGICAL >> 5) + 1;
ZK_HD uint32_t zkc_phys(uint32_t w) { return w + (w >> 5); }                      // dword index
ZK_HD uint32_t zkc_phys_byte(uint32_t x) { return x + 4 * (x >> 7); }             // byte index

ZK_HD uint32_t zkc_gear(uint32_t b)
{
    uint32_t x = (b + 1) * 0x9E3779B1u;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// the rule's three numbers, resolved from the caller's parameters (zk_cdc.hip: zk_cdc_rule)
struct ZkCdcRule { uint32_t min, max, bits; };
ZK_HD uint32_t zkc_tiles(uint64_t slice_len) { return (uint32_t)((slice_len + ZKC_TILE - 1) / ZKC_TILE); }
// The parallel selection's segments for slices of at most `slice` bytes: about ZKC_SEG_FRAMES frames of the size the rule aims at each (the
// speculative chains are walked side by side, the fix-up pays per segment), at most ZKC_SEGS_MAX of them, whole KiB; a row holds the cuts
// inside a segment, min apart but for the input's last, and the one the chain starts from
constexpr uint32_t ZKC_SEG_FRAMES = 256, ZKC_SEGS_MAX = 1024;
struct ZkCdcSegs { uint64_t seg; uint32_t nseg, row; };
ZK_HD ZkCdcSegs zkc_segs(uint64_t slice, uint32_t min, uint32_t bits)
{
    ZkCdcSegs g;
    g.seg = ((uint64_t)min + (1ull << bits)) * ZKC_SEG_FRAMES;
    const uint64_t least = (slice + ZKC_SEGS_MAX - 1) / ZKC_SEGS_MAX;
    if (g.seg < least) g.seg = least;
    g.seg = (g.seg + 1023) & ~1023ull;
    g.nseg = (uint32_t)((slice + g.seg - 1) / g.seg);
    g.row = (uint32_t)(g.seg / min) + 3;
    return g;
}
// The scratch of one call, in bytes from its start, for slices of at most `slice` bytes (zk_cdc_pass reserves it, the emulator harness
// allocates the same): bitmap[tiles * 256 uint4] | counts[tiles] | bases[tiles + 1] | state | nruns | meta[nseg] | runs[nseg] |
// rows[nseg * row] | list[slice]
struct ZkCdcState { uint64_t cut, count; };                 // the chain so far: its last cut, the cuts made behind off[0]
struct ZkCdcLayout { size_t bitmap, counts, bases, state, nruns, meta, runs, rows, list, end; uint32_t tiles; ZkCdcSegs g; };
ZK_HD ZkCdcLayout zkc_layout(uint64_t slice, uint32_t min, uint32_t bits)
{
    ZkCdcLayout L;
    L.tiles = zkc_tiles(slice);
    L.g = zkc_segs(slice, min, bits);
    L.bitmap = 0;
    L.counts = (size_t)L.tiles * ZKC_THREADS * 16;
    L.bases = L.counts + (size_t)L.tiles * 8;
    L.state = L.bases + ((size_t)L.tiles + 1) * 8;
    L.nruns = L.state + sizeof(ZkCdcState);
    L.meta = L.nruns + 8;
    L.runs = L.meta + (size_t)L.g.nseg * 32;
    L.rows = L.runs + (size_t)L.g.nseg * 24 + 8 * (L.g.nseg & 1);
    L.list = L.rows + (size_t)L.g.nseg * L.g.row * 8;
    L.end = L.list + (size_t)slice * 4;
    return L;
}

struct ZkCdcSlice {
    const uint8_t *src;         // the byte at position src_pos: 0 for a source on the device, s0 - 31 (or 0) for a host-pointer call's staged slice
    uint64_t src_pos;
    uint64_t s0, len;           // the slice: positions [s0, s0 + len), s0 a multiple of 1024, s0 + len <= n
    uint32_t bits;
};
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cdc_mark(ZkCdcSlice a, uint4 *bitmap, uint64_t *counts)
{
    __shared__ uint32_t gear[256];
    __shared__ uint32_t tile[ZKC_LDS_DWORDS];
    __shared__ uint32_t total;
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    const uint64_t base = a.s0 + (uint64_t)t * ZKC_TILE;                        // the tile: positions [base, end)
    const uint64_t end = base + ZKC_TILE < a.s0 + a.len ? base + ZKC_TILE : a.s0 + a.len;
    const uint32_t lead = base >= ZKC_LEAD ? ZKC_LEAD : (uint32_t)base;         // (base is a multiple of 1024: 31, or 0 at the first byte)
    const uint8_t *A = a.src + (base - lead - a.src_pos);
    const uint32_t nbytes = (uint32_t)(end - base) + lead;
    const uint32_t shift = (uint32_t)((uintptr_t)A & 15);
    const uint8_t *A0 = A - shift;
    gear[tid] = zkc_gear(tid);
    if (tid == 0) total = 0;
    // [A, A + nbytes): whole aligned 16-byte pieces c0 .. c1 - 1 of A0, the bytes before and behind them one by one
    const uint32_t c0 = (shift + 15) >> 4, c1 = (shift + nbytes) >> 4;
    const uint32_t head_end = 16 * c0 < shift + nbytes ? 16 * c0 : shift + nbytes;
    const uint32_t tail_from = 16 * c1 > head_end ? 16 * c1 : head_end;
    for (uint32_t i = c0 + tid; i < c1; i += ZKC_THREADS) {
        const uint4 v = *(const uint4 *)(A0 + 16 * (size_t)i);
        const uint32_t at = zkc_phys(4 * i + 8);                                 // (four dwords of one group of 32: contiguous)
        tile[at] = v.x; tile[at + 1] = v.y; tile[at + 2] = v.z; tile[at + 3] = v.w;
    }
    uint8_t *tb = (uint8_t *)tile;
    for (uint32_t x = shift + tid; x < head_end; x += ZKC_THREADS) tb[zkc_phys_byte(x + 32)] = A0[x];
    for (uint32_t x = tail_from + tid; x < shift + nbytes; x += ZKC_THREADS) tb[zkc_phys_byte(x + 32)] = A0[x];
    __syncthreads();
    const uint64_t p0 = base + (uint64_t)ZKC_RUN * tid;                          // the lane's run: positions [p0, p0 + 128)
    uint32_t w[4] = {0, 0, 0, 0};
    if (p0 < end) {
        const uint32_t xr = 32 + shift + lead + ZKC_RUN * tid;                   // LDS byte of p0; the warm-up starts 31 bytes before it
        const uint32_t xw = xr - ZKC_LEAD, d0 = xw >> 2, sh = xw & 3;
        const uint32_t skip = p0 < ZKC_LEAD ? ZKC_LEAD - (uint32_t)p0 : 0;       // warm-up steps before the first byte: absent terms
        const uint32_t thr = 1u << (32 - a.bits);
        uint32_t h = 0, prev = tile[zkc_phys(d0)];
#pragma unroll
        for (uint32_t k = 0; k < ZKC_DWORDS; k++) {
            const uint32_t next = tile[zkc_phys(d0 + k + 1)];
            const uint32_t d = __builtin_amdgcn_alignbyte(next, prev, sh);       // bytes xw + 4 k ... + 3
            prev = next;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t s = 4 * k + j;
                if (s >= ZKC_STEPS) break;
                const uint32_t hn = (h << 1) + gear[(d >> (8 * j)) & 255u];
                if (s < ZKC_LEAD) h = s >= skip ? hn : h;
                else {
                    h = hn;
                    if (h < thr) w[(s - ZKC_LEAD) >> 5] |= 1u << ((s - ZKC_LEAD) & 31);
                }
            }
        }
        // positions from `end` on (garbage was hashed there) are no candidates
        const uint64_t left = end - p0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (left <= 32 * k) w[k] = 0;
            else if (left < 32 * k + 32) w[k] &= (1u << (uint32_t)(left - 32 * k)) - 1u;
        }
    }
    bitmap[(size_t)t * ZKC_THREADS + tid] = make_uint4(w[0], w[1], w[2], w[3]);
    const uint32_t pc = (uint32_t)__popcll(((uint64_t)w[1] << 32) | w[0]) + (uint32_t)__popcll(((uint64_t)w[3] << 32) | w[2]);
    if (pc) atomicAdd(&total, pc);
    __syncthreads();
    if (tid == 0) counts[t] = total;
}

// list[bases[t] ...]: the positions, counted from the slice's first, of the candidates of tile t in ascending order (bases: the exclusive
// scan of zk_k_cdc_mark's counts, tiles + 1 entries)
__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cdc_emit(const uint4 *bitmap, const uint64_t *bases, uint32_t *list)
{
    __shared__ uint32_t pre[2][ZKC_THREADS];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;
    if (bases[t + 1] == bases[t]) return;                                        // (the same for every lane)
    const uint4 v = bitmap[(size_t)t * ZKC_THREADS + tid];
    const uint32_t pc = (uint32_t)__popcll(((uint64_t)v.y << 32) | v.x) + (uint32_t)__popcll(((uint64_t)v.w << 32) | v.z);
    uint32_t cur = 0;
    pre[0][tid] = pc;
    __syncthreads();
    for (uint32_t st = 1; st < ZKC_THREADS; st <<= 1) {
        pre[cur ^ 1][tid] = pre[cur][tid] + (tid >= st ? pre[cur][tid - st] : 0);
        cur ^= 1;
        __syncthreads();
    }
    uint64_t at = bases[t] + (pre[cur][tid] - pc);
    const uint32_t rel = t * ZKC_TILE + tid * ZKC_RUN;
    const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t m = ws[k]; m; m &= m - 1) list[at++] = rel + 32 * k + ((uint32_t)__ffs((int)m) - 1);
}

struct ZkCdcSel {
    uint64_t n, s0, s1;         // the input's size; the slice: positions [s0, s1), which offers the cuts (s0, s1]
    uint32_t min, max;
    uint64_t off_cap;           // off[] holds off_cap + 1 entries: a cut beyond them is counted and not stored
    uint64_t seg;               // the parallel form: cut offsets (s0 + k seg, s0 + (k + 1) seg] are segment k's
    uint32_t nseg, row;         // segments of this slice; entries between the segments' rows of speculative cuts
};
// a value every lane holds alike, said so to the compiler: the walk's arithmetic then runs on the scalar unit
__device__ __forceinline__ uint32_t zkc_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t zkc_uni64(uint64_t v) { return ((uint64_t)zkc_uni((uint32_t)(v >> 32)) << 32) | zkc_uni((uint32_t)v); }

// How a walk ends: at n; at a cut whose range [c + min, min(c + max, n)] reaches into the next slice; because on_cut said so
enum { ZKC_END = 1, ZKC_CARRY = 2, ZKC_STOP = 3 };
// ONE wave walks the chain from `cut` over list[idx ...] (list[m]: zk_k_cdc_emit's), streamed through `chunk` (LDS, cap entries) -- every
// branch is taken by all 64 lanes.  Lane l holds entry window + l in a register: a step is a compare against c + min, a ballot, a find-first
// and a readlane, and reads no memory until the 64 entries are used up.  When none of the 64 is at or behind c + min and the chunk holds more
// (the dense case) the first that is is found by bisection in the chunk.  After every cut, with `cut` and `idx` (the first entry not yet
// passed) set, on_cut() is called; it may move both, and ends the walk by returning false.
template <class F> __device__ __forceinline__ uint32_t zkc_walk(const ZkCdcSel &a, const uint32_t *list, uint64_t m, uint32_t *chunk, uint32_t cap,
                                                                uint64_t &cut, uint64_t &idx, F on_cut)
{
    const uint32_t lane = threadIdx.x;
    for (;;) {
        const uint64_t b = idx;
        const uint32_t len = (uint32_t)(m - b < cap ? m - b : cap);
        __syncthreads();
        for (uint32_t i = lane; i < len; i += ZKC_SEL_THREADS) chunk[i] = list[b + i];
        __syncthreads();
        uint32_t j = 0, wb = 0;
        uint32_t ev = lane < len ? chunk[lane] : 0;
        for (;;) {
            if (cut >= a.n) return ZKC_END;
            const uint64_t lo = cut + a.min, hi = cut + a.max < a.n ? cut + a.max : a.n;
            if (j >= wb + 64) { wb = j; ev = wb + lane < len ? chunk[wb + lane] : 0; }
            const uint32_t nv = len - wb < 64 ? len - wb : 64;
            const uint64_t live = (nv == 64 ? ~0ull : (1ull << nv) - 1) & ~((1ull << (j - wb)) - 1);
            // entry e offers the cut s0 + e + 1: at or behind lo from e = lo - s0 - 1 on
            const uint64_t t = lo > a.s0 + 1 ? lo - a.s0 - 1 : 0;
            const uint64_t found = t >> 32 ? 0 : __ballot(ev >= (uint32_t)t) & live;
            uint64_t c;
            if (found) {
                const uint32_t flo = (uint32_t)found, fhi = (uint32_t)(found >> 32);
                const uint32_t f = flo ? (uint32_t)__ffs((int)flo) - 1 : 31 + (uint32_t)__ffs((int)fhi);
                const uint64_t qf = a.s0 + (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)f) + 1;
                if (qf <= hi) { c = qf; j = wb + f + 1; } else { c = hi; j = wb + f; }
            } else if (wb + 64 < len) {
                if (t >> 32 || chunk[len - 1] < (uint32_t)t) j = len;
                else {
                    uint32_t x = wb + 64, y = len - 1;
                    while (x < y) { const uint32_t mid = x + (y - x) / 2; if (chunk[mid] >= (uint32_t)t) y = mid; else x = mid + 1; }
                    j = zkc_uni(x);
                }
                continue;
            } else {
                // the chunk is used up: the next one, or the slice holds no candidate from lo on
                if (b + len < m) { idx = b + len; break; }
                if (hi > a.s1) { idx = m; return ZKC_CARRY; }
                c = hi; j = len;
            }
            cut = c; idx = b + j;
            if (!on_cut()) return ZKC_STOP;
            if (idx != b + j) break;                                             // (on_cut moved on: the chunk from there)
        }
    }
}

// The serial form (slices of one segment).  off may be null (a counting pass).
__global__ __launch_bounds__(ZKC_SEL_THREADS) void zk_k_cdc_select(ZkCdcSel a, const uint32_t *list, const uint64_t *total, ZkCdcState *state, uint64_t *off)
{
    __shared__ uint32_t chunk[ZKC_CHUNK];
    const uint32_t lane = threadIdx.x;
    const uint64_t m = zkc_uni64(*total);
    uint64_t cut = zkc_uni64(state->cut), count = zkc_uni64(state->count), idx = 0;
    zkc_walk(a, list, m, chunk, ZKC_CHUNK, cut, idx, [&]() {
        count++;
        if (lane == 0 && off && count <= a.off_cap) off[count] = cut;
        return true;
    });
    if (lane == 0) { state->cut = cut; state->count = count; }
}

// ---- The parallel form.  Where a frame ends depends on where it starts and on its own bytes, so two chains that share one cut share all later
// ones.  zk_k_cdc_spec: a wave per segment walks a SPECULATIVE chain from the segment's first candidate, taken for a cut, and keeps its cuts
// inside the segment in the segment's row, then how it left: the first cut behind the segment (and the list index there), the end of the
// input, or a cut the slice cannot decide.  zk_k_cdc_fix: one wave walks the TRUE chain; every cut it makes is looked up in its segment's row,
// and from the first one found there the rest of the row is the true chain's -- a run, noted with the place it takes in off[] --, which goes
// on at the row's exit.  zk_k_cdc_copy writes the runs.  Without candidates (zeros) no chain is speculated and the fix-up is the serial walk.
struct ZkCdcSegMeta { uint64_t exit, exit_idx; uint32_t ns, kind, pad[2]; };      // kind: ZKC_STOP (exit, exit_idx valid), ZKC_END, ZKC_CARRY
struct ZkCdcRun { uint64_t dst; uint32_t seg, from, cnt, pad; };                    // off[dst + i] = row[seg][from + i], i < cnt
constexpr uint32_t ZKC_SPEC_CHUNK = 1024;
__global__ __launch_bounds__(ZKC_SEL_THREADS) void zk_k_cdc_spec(ZkCdcSel a, const uint32_t *list, const uint64_t *total, uint64_t *rows, ZkCdcSegMeta *meta)
{
    __shared__ uint32_t chunk[ZKC_SPEC_CHUNK];
    const uint32_t lane = threadIdx.x, k = blockIdx.x;
    const uint64_t m = zkc_uni64(*total), len = a.s1 - a.s0;
    const uint64_t e0 = (uint64_t)k * a.seg, e1 = e0 + a.seg < len ? e0 + a.seg : len;       // entries [e0, e1) offer the segment's cuts
    uint64_t x = 0, y = m;                                                                  // the first entry at or behind e0
    while (x < y) { const uint64_t mid = x + (y - x) / 2; if (zkc_uni(list[mid]) >= e0) y = mid; else x = mid + 1; }
    uint64_t *row = rows + (uint64_t)k * a.row;
    ZkCdcSegMeta mt = {0, 0, 0, 0, {0, 0}};
    if (x < m && zkc_uni(list[x]) < e1) {
        uint64_t cut = a.s0 + zkc_uni(list[x]) + 1, idx = x + 1;
        const uint64_t seg_end = a.s0 + e1;
        uint32_t ns = 1;
        if (lane == 0) row[0] = cut;
        mt.kind = zkc_walk(a, list, m, chunk, ZKC_SPEC_CHUNK, cut, idx, [&]() {
            if (cut > seg_end) return false;
            if (lane == 0) row[ns] = cut;
            ns++;
            return true;
        });
        mt.ns = ns; mt.exit = cut; mt.exit_idx = idx;
    }
    if (lane == 0) meta[k] = mt;
}

__global__ __launch_bounds__(ZKC_SEL_THREADS) void zk_k_cdc_fix(ZkCdcSel a, const uint32_t *list, const uint64_t *total, const uint64_t *rows, const ZkCdcSegMeta *meta,
                                                                ZkCdcState *state, uint64_t *off, ZkCdcRun *runs, uint64_t *nruns)
{
    __shared__ uint32_t chunk[ZKC_SPEC_CHUNK];
    const uint32_t lane = threadIdx.x;
    const uint64_t m = zkc_uni64(*total);
    uint64_t cut = zkc_uni64(state->cut), count = zkc_uni64(state->count), idx = 0, nr = 0;
    // the true cut `cut` in its segment's row?  Then the rest of the row is a run, and the chain goes on at the row's exit, which is looked
    // up in turn.  Returns false when the chain is thereby at its end for this slice.
    auto adopt = [&]() {
        for (;;) {
            if (cut <= a.s0) return true;
            const uint32_t k = (uint32_t)((cut - a.s0 - 1) / a.seg);
            const uint32_t ns = zkc_uni(meta[k].ns), kind = zkc_uni(meta[k].kind);
            const uint64_t *row = rows + (uint64_t)k * a.row;
            uint32_t at = ns;                                                    // where in the row: 64 entries at a time
            for (uint32_t w = 0; w < ns; w += 64) {
                const uint64_t v = w + lane < ns ? row[w + lane] : ~0ull;
                const uint64_t hit = __ballot(v == cut), past = __ballot(v > cut);
                if (hit) { const uint32_t hl = (uint32_t)hit, hh = (uint32_t)(hit >> 32); at = w + (hl ? (uint32_t)__ffs((int)hl) - 1 : 31 + (uint32_t)__ffs((int)hh)); break; }
                if (past) break;
            }
            if (at == ns) return true;
            const uint32_t cnt = ns - at - 1;
            if (cnt) {
                if (lane == 0) runs[nr] = ZkCdcRun{count + 1, k, at + 1, cnt, 0};
                nr++; count += cnt;
            }
            if (kind == ZKC_STOP) {
                cut = zkc_uni64(meta[k].exit); idx = zkc_uni64(meta[k].exit_idx);
                count++;
                if (lane == 0 && off && count <= a.off_cap) off[count] = cut;
                continue;
            }
            cut = kind == ZKC_END ? a.n : zkc_uni64(row[ns - 1]);
            return false;
        }
    };
    if (adopt())
        zkc_walk(a, list, m, chunk, ZKC_SPEC_CHUNK, cut, idx, [&]() {
            count++;
            if (lane == 0 && off && count <= a.off_cap) off[count] = cut;
            return adopt();
        });
    if (lane == 0) { state->cut = cut; state->count = count; *nruns = nr; }
}

__global__ __launch_bounds__(ZKC_THREADS) void zk_k_cdc_copy(ZkCdcSel a, const uint64_t *rows, const ZkCdcRun *runs, const uint64_t *nruns, uint64_t *off)
{
    if (!off || blockIdx.x >= *nruns) return;
    const ZkCdcRun r = runs[blockIdx.x];
    const uint64_t *row = rows + (uint64_t)r.seg * a.row + r.from;
    for (uint32_t i = threadIdx.x; i < r.cnt; i += ZKC_THREADS) if (r.dst + i <= a.off_cap) off[r.dst + i] = row[i];
}

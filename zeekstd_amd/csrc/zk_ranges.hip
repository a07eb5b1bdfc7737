// zk_ranges.hip -- gfx950 kernels of the batched byte-range read (zk_read_ranges*, include/zeekstd_amd.h).
//   zk_k_range_lens     (packed destinations only) the bytes each range will deliver; zk_k_scan64 turns them into destinations
//   zk_k_range_plan     a lane per range: validation, first / last frame by binary search of d_off (zk_ranges.h), and the range's
//                       +1 / -1 in a difference array over the frames -- O(1) per range however many frames it crosses
//   zk_k_range_compact  one workgroup: prefix sums of the difference array = how many ranges cover a frame; the covered, non-empty
//                       frames compacted into the sorted list of unique ids + the prefix sums of their decompressed sizes -- the
//                       ids / out_off pair zk_decode_enqueue takes -- and frame -> position in that list
//   zk_k_range_pieces   per decode pass, a lane per range: the part of the range that the pass holds, as ONE copy (the unique
//                       frames are packed in stream order, and a range crosses no frame it does not touch: whatever a pass
//                       holds of a range is contiguous in the scratch), and how many 64 KiB chunks it is dealt in
//   zk_k_range_gather   scratch -> destination: a wave per small copy, a workgroup per 64 KiB chunk of a large one
//   zk_k_range_status   a lane per range: its own validation code, or the first failing frame among those it touches
// HBM-bound byte moving and integer work; no MFMA.
#include <hip/hip_runtime.h>
#include "zk_kernels.h"
#include "zk_ranges.h"
#include "zk_range_copy.h"

// ------------------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(256) void zk_k_range_lens(const uint64_t *d_off, uint32_t n_frames, const uint64_t *offs, const uint64_t *lens, uint32_t count, uint64_t *eff)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint64_t len = lens[i];
    eff[i] = zkr_check_src(d_off[n_frames], offs[i], len) == ZKR_OK ? len : 0;     // a range outside the stream takes no room
}

__global__ __launch_bounds__(256) void zk_k_range_plan(const uint64_t *d_off, uint32_t n_frames, const uint64_t *offs, const uint64_t *lens, const uint64_t *dst_off,
                                                       uint32_t count, uint64_t dst_cap, uint32_t *rfirst, uint32_t *rlast, int32_t *status, uint32_t *cover)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint64_t off = offs[i], len = lens[i];
    const int32_t st = zkr_check(d_off[n_frames], off, len, dst_cap, dst_off[i]);
    uint32_t first = ~0u, last = ~0u;
    if (st == ZKR_OK && zkr_span(d_off, n_frames, off, len, &first, &last)) {
        atomicAdd(&cover[first], 1u);
        atomicAdd(&cover[last + 1], ~0u);           // (-1: the sums wrap back)
    }
    rfirst[i] = first; rlast[i] = last;             // ~0: the range copies nothing
    status[i] = st;
}

// One workgroup, ZK_RANGE_PER_LANE consecutive frames per lane and round.  words: [0] frames touched, [1] their decompressed bytes.
constexpr uint32_t ZK_RANGE_PER_LANE = 16;
__global__ __launch_bounds__(1024) void zk_k_range_compact(const uint64_t *d_off, uint32_t n_frames, const uint32_t *cover, uint32_t *slot, uint32_t *ids,
                                                          uint64_t *uoff, uint64_t *words)
{
    __shared__ uint32_t w_cov[16], w_cnt[16];
    __shared__ uint64_t w_bytes[16];
    __shared__ uint32_t c_cov, c_cnt;
    __shared__ uint64_t c_bytes;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { c_cov = 0; c_cnt = 0; c_bytes = 0; }
    __syncthreads();
    for (uint64_t base = 0; base < n_frames; base += 1024ull * ZK_RANGE_PER_LANE) {
        const uint64_t f0 = base + (uint64_t)tid * ZK_RANGE_PER_LANE;
        // the lane's own sums first: coverage delta, touched frames and bytes need the coverage at the lane's first frame
        uint32_t dcov = 0;
        for (uint32_t j = 0; j < ZK_RANGE_PER_LANE; j++) if (f0 + j < n_frames) dcov += cover[f0 + j];
        uint32_t x = dcov;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if ((int)lane >= d) x += y; }
        if (lane == 63) w_cov[wave] = x;
        __syncthreads();
        uint32_t cov = c_cov + x - dcov;
        for (uint32_t w = 0; w < wave; w++) cov += w_cov[w];
        // cov: ranges that cover the frames in front of f0, carried over
        uint32_t cnt = 0, touched = 0;
        uint64_t bytes = 0;
        {
            uint32_t cv = cov;
            for (uint32_t j = 0; j < ZK_RANGE_PER_LANE; j++) if (f0 + j < n_frames) {
                cv += cover[f0 + j];
                const uint64_t sz = d_off[f0 + j + 1] - d_off[f0 + j];
                if (cv != 0 && sz != 0) { touched |= 1u << j; cnt++; bytes += sz; }
            }
        }
        uint32_t xc = cnt;
        uint64_t xb = bytes;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t yc = __shfl_up(xc, d, 64);
            const uint64_t yb = __shfl_up(xb, d, 64);
            if ((int)lane >= d) { xc += yc; xb += yb; }
        }
        if (lane == 63) { w_cnt[wave] = xc; w_bytes[wave] = xb; }
        __syncthreads();
        uint32_t s = c_cnt + xc - cnt;
        uint64_t b = c_bytes + xb - bytes;
        for (uint32_t w = 0; w < wave; w++) { s += w_cnt[w]; b += w_bytes[w]; }
        for (uint32_t j = 0; j < ZK_RANGE_PER_LANE; j++) if (f0 + j < n_frames) {
            slot[f0 + j] = s;
            if (touched >> j & 1) { ids[s] = (uint32_t)(f0 + j); uoff[s] = b; s++; b += d_off[f0 + j + 1] - d_off[f0 + j]; }
        }
        __syncthreads();
        if (tid == 1023) { c_cov = cov + dcov; c_cnt = s; c_bytes = b; }
        __syncthreads();
    }
    if (tid == 0) { uoff[c_cnt] = c_bytes; words[0] = c_cnt; words[1] = c_bytes; }
}

// out_off of a pass that does not begin the list: its slice of the prefix sums, from 0
__global__ __launch_bounds__(256) void zk_k_range_rebase(const uint64_t *uoff, uint32_t a, uint32_t n, uint64_t *poff)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n) poff[i] = uoff[a + i] - uoff[a];
}

// ------------------------------------------------------------------------------------------------ copy
// The pass holds positions [a, b) of the unique list: frames ids[a] .. ids[b - 1], packed at scratch + (uoff[s] - uoff[a]).
__global__ __launch_bounds__(256) void zk_k_range_pieces(const uint64_t *d_off, const uint64_t *offs, const uint64_t *lens, const uint64_t *dst_off, uint32_t count,
                                                         const uint32_t *rfirst, const uint32_t *rlast, const uint32_t *slot, const uint32_t *ids, const uint64_t *uoff,
                                                         uint32_t a, uint32_t b, uintptr_t dst_base, ZkRangeCopy *copies, uint64_t *cnt)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > count) return;
    if (i == count) { cnt[i] = 0; return; }            // (the scan's last entry is the total)
    ZkRangeCopy c{0, 0, 0};
    const uint32_t first = rfirst[i];
    const uint32_t fa = ids[a], fb = ids[b - 1];
    if (first != ~0u && first <= fb && rlast[i] >= fa) {
        const uint64_t off = offs[i];
        uint64_t lo, n;
        zkr_clip(off, lens[i], d_off[fa], d_off[fb + 1], &lo, &n);
        const uint32_t g = first >= fa ? first : fa;    // the frame `lo` lies in: the range's first, or the pass's
        c.src = uoff[slot[g]] - uoff[a] + (lo - d_off[g]);
        c.dst = dst_off[i] + (lo - off);
        c.n = n;
    }
    copies[i] = c;
    // chunks are cut on the destination's 16-byte grid, so that only a copy's own two ends are ragged
    cnt[i] = c.n > ZK_RANGE_SMALL ? (c.n + ((dst_base + c.dst) & 15) + ZK_RANGE_CHUNK - 1) / ZK_RANGE_CHUNK : 0;
}

// Workgroups [0, small_wgs): four waves, a small copy each.  The others: the 64 KiB chunks of the large copies, dealt round robin;
// coff (count + 1 prefix sums of the copies' chunk counts) says whose chunk a number is.
__global__ __launch_bounds__(256) void zk_k_range_gather(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ dst, const ZkRangeCopy *__restrict__ copies,
                                                         const uint64_t *__restrict__ coff, uint32_t count, uint32_t small_wgs)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < small_wgs) {
        const uint64_t i = (uint64_t)blockIdx.x * 4 + (tid >> 6);
        if (i >= count) return;
        const ZkRangeCopy c = copies[i];
        if (c.n == 0 || c.n > ZK_RANGE_SMALL) return;
        zk_range_copy<64>(dst + c.dst, scratch + c.src, c.n, tid & 63);
        return;
    }
    const uint64_t total = coff[count];
    for (uint64_t k = blockIdx.x - small_wgs; k < total; k += gridDim.x - small_wgs) {
        uint32_t lo = 0, hi = count;                    // the last copy with coff[i] <= k (copies without chunks share their successor's entry)
        while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (coff[mid] <= k) lo = mid; else hi = mid; }
        const ZkRangeCopy c = copies[lo];
        const uint64_t j = k - coff[lo];
        const uint64_t skew = (uintptr_t)(dst + c.dst) & 15;
        const uint64_t b0 = j ? j * ZK_RANGE_CHUNK - skew : 0;
        uint64_t b1 = (j + 1) * ZK_RANGE_CHUNK - skew;
        if (b1 > c.n) b1 = c.n;
        if (b0 < b1) zk_range_copy<256>(dst + c.dst + b0, scratch + c.src + b0, b1 - b0, tid);
    }
}

// ------------------------------------------------------------------------------------------------ status
// fstat[s]: the ZSTD_ErrorCode of unique frame s (0 = fine).  The frames of a range are looked at only when some frame failed at all
// (any_failed, or *pass_err != ~0: the first-error word of the decode pass still in flight).
__global__ __launch_bounds__(256) void zk_k_range_status(const uint64_t *d_off, uint32_t count, const uint32_t *rfirst, const uint32_t *rlast, const uint32_t *slot,
                                                         const int32_t *fstat, int any_failed, const uint64_t *pass_err, int32_t *status, unsigned long long *first_err)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    int32_t st = status[i];
    const uint32_t first = rfirst[i];
    if (st == ZKR_OK && first != ~0u && (any_failed || (pass_err && *pass_err != ~0ull))) {
        const uint32_t last = rlast[i];
        for (uint32_t f = first; f <= last && st == ZKR_OK; f++)
            if (d_off[f + 1] != d_off[f]) st = -fstat[slot[f]];
        status[i] = st;
    }
    if (st != ZKR_OK) atomicMin(first_err, ((unsigned long long)i << 32) | (uint32_t)(-st));
}

// ------------------------------------------------------------------------------------------------ launchers
void zk_launch_range_plan(hipStream_t st, const ZkRangeArgs &r, uint64_t *eff, uint64_t *packed, uint32_t *rfirst, uint32_t *rlast, int32_t *status, uint32_t *cover,
                          uint32_t *slot, uint32_t *ids, uint64_t *uoff, uint64_t *words)
{
    const dim3 grid((r.count + 255) / 256);
    if (!r.dst_off) {
        hipLaunchKernelGGL(zk_k_range_lens, grid, dim3(256), 0, st, r.d_off, r.n_frames, r.offs, r.lens, r.count, eff);
        zk_launch_scan64(st, eff, r.count, packed);
    }
    hipLaunchKernelGGL(zk_k_range_plan, grid, dim3(256), 0, st, r.d_off, r.n_frames, r.offs, r.lens, r.dst_off ? r.dst_off : packed, r.count, r.dst_cap, rfirst, rlast,
                       status, cover);
    hipLaunchKernelGGL(zk_k_range_compact, dim3(1), dim3(1024), 0, st, r.d_off, r.n_frames, cover, slot, ids, uoff, words);
}
void zk_launch_range_compact(hipStream_t st, const uint64_t *d_off, uint32_t n_frames, const uint32_t *cover, uint32_t *slot, uint32_t *ids, uint64_t *uoff, uint64_t *words)
{
    hipLaunchKernelGGL(zk_k_range_compact, dim3(1), dim3(1024), 0, st, d_off, n_frames, cover, slot, ids, uoff, words);
}
void zk_launch_range_rebase(hipStream_t st, const uint64_t *uoff, uint32_t a, uint32_t n, uint64_t *poff)
{
    hipLaunchKernelGGL(zk_k_range_rebase, dim3(n / 256 + 1), dim3(256), 0, st, uoff, a, n, poff);
}
void zk_launch_range_pieces(hipStream_t st, const ZkRangeArgs &r, const uint64_t *dst_off, const uint32_t *rfirst, const uint32_t *rlast, const uint32_t *slot,
                            const uint32_t *ids, const uint64_t *uoff, uint32_t a, uint32_t b, ZkRangeCopy *copies, uint64_t *cnt, uint64_t *coff)
{
    hipLaunchKernelGGL(zk_k_range_pieces, dim3(r.count / 256 + 1), dim3(256), 0, st, r.d_off, r.offs, r.lens, dst_off, r.count, rfirst, rlast, slot, ids, uoff, a, b,
                       (uintptr_t)r.dst, copies, cnt);
    zk_launch_scan64(st, cnt, r.count + 1, coff);
}
void zk_launch_range_gather(hipStream_t st, const uint8_t *scratch, uint8_t *dst, const ZkRangeCopy *copies, const uint64_t *coff, uint32_t count, uint64_t pass_bytes)
{
    const uint32_t small_wgs = (uint32_t)(((uint64_t)count + 3) / 4);
    // chunk workgroups: what the pass can hold in chunks (ranges that repeat bytes bring more: the kernel deals them round robin), at most eight per CU
    uint64_t big = pass_bytes / ZK_RANGE_CHUNK + 1;
    if (big > 2048) big = 2048;
    hipLaunchKernelGGL(zk_k_range_gather, dim3(small_wgs + (uint32_t)big), dim3(256), 0, st, scratch, dst, copies, coff, count, small_wgs);
}
void zk_launch_range_status(hipStream_t st, const ZkRangeArgs &r, const uint32_t *rfirst, const uint32_t *rlast, const uint32_t *slot, const int32_t *fstat,
                            bool any_failed, const uint64_t *pass_err, int32_t *status, uint64_t *first_err)
{
    hipLaunchKernelGGL(zk_k_range_status, dim3((r.count + 255) / 256), dim3(256), 0, st, r.d_off, r.count, rfirst, rlast, slot, fstat, any_failed ? 1 : 0, pass_err, status,
                       (unsigned long long *)first_err);
}

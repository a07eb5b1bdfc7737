// zk_train.h -- the kernels that train a dictionary's CONTENT on the device (included by zk_train.hip, which keeps their launchers;
// tests/sim/zk_train_sim.cpp runs the same source on the CPU under the workgroup emulator, against the numpy model of
// tests/helpers/train_model.py).  The rule follows fastCover's epoch scheme without its per-segment duplicate map:
//   zk_k_train_count    every position whose d bytes lie inside one sample: its d-mer hashed to f bits, one integer atomic into
//                       freq[1 << f]; the hash (or ZKT_NONE) is kept per position in `hpos`, so that the selection hashes nothing again
//   zk_k_train_select   a workgroup per candidate segment length k, each on its own copy of freq: epoch after epoch the segment of k
//                       bytes with the largest sum of freq over its k - d + 1 positions (lowest position on ties) joins the content and
//                       freq is cleared at its d-mers; rounds over the epochs until the content is full or a round adds nothing
//   zk_k_train_gather   every j-th sample behind one another (the trial encodes of samples above the trial limit)
//   zk_k_train_stats    256 literal values and 36 / 53 / 32 LL / ML / OF codes of everything the matcher left, counted per workgroup in LDS
// Positions count from the first sample's first byte (src = d_samples + off[0]); N, the number of positions, is the samples' total size.
// Integer atomics and integer sums only: the result does not depend on which lane or workgroup comes first.  Byte and gather work, no MFMA.
#pragma once
#include <stdint.h>
#include "zk_device.h"
#include "zk_enc_device.h"

constexpr uint32_t ZKT_NONE = 0xFFFFFFFFu;          // hpos: no d-mer of one sample starts here
constexpr uint32_t ZKT_K_MIN = 16, ZKT_K_MAX = 4096; // segment lengths the selection's tile holds (zk_train_params::k)
constexpr uint32_t ZKT_CANDS_MAX = 4;
constexpr uint32_t ZKT_HEADER_RESERVE = 512;        // of the caller's capacity: what a formatted dictionary's header may take
constexpr uint32_t ZKT_COUNT_WGS_MAX = 4096;        // zk_k_train_count's grid: a workgroup per 256 positions up to here, strided beyond
constexpr uint32_t ZKT_SEL_THREADS = 1024;
constexpr uint32_t ZKT_TILE = 1024;                 // segment starts scored per tile, one per lane ...
constexpr uint32_t ZKT_PER_LANE = 5;                // ... out of the prefix sums of per * 1024 >= ZKT_TILE + k positions, per = zkt_per_lane(k) <= ZKT_PER_LANE
static_assert(ZKT_PER_LANE * ZKT_SEL_THREADS >= ZKT_TILE + ZKT_K_MAX, "a tile's last start sees its whole segment");

// the d-mer at p, d = 6 or 8 bytes little endian, to f bits (10 ... 24): one multiplication, the top bits
ZK_HD uint32_t zkt_hash(const uint8_t *p, uint32_t d, uint32_t f)
{
    uint64_t v = 0;
    for (uint32_t j = 0; j < d; j++) v |= (uint64_t)p[j] << (8 * j);
    return (uint32_t)(((v << (64 - 8 * d)) * (d == 8 ? 0xCF1BBCDCB7A56463ull : 227718039650203ull)) >> (64 - f));
}
// positions a lane gathers per tile: the tile's starts and the k - d positions behind the last one, spread over the workgroup
ZK_HD uint32_t zkt_per_lane(uint32_t k) { return (ZKT_TILE + k + ZKT_SEL_THREADS - 1) / ZKT_SEL_THREADS; }
// The scratch of one training call, in bytes from its start (zk_train_run reserves it, the emulator harness allocates the same):
//   hpos[n] | freq[(nk + 1) << f] (the counted table, then a copy per candidate) | content[nk * stride] (a candidate's content ENDS at
//   c * stride + ccap; ZKE_LDM_SLACK zero bytes behind it for the matcher's long-distance table) | segs[nk * segs_cap] | out[2 nk] |
//   hist[ZKT_H_WORDS] | whatever the caller puts behind `end`
constexpr uint32_t ZKT_H_LL = 256, ZKT_H_ML = 292, ZKT_H_OF = 345, ZKT_H_WORDS = 377;
struct ZkTrainLayout { size_t hpos, freq, content, segs, out, hist, end; uint32_t stride, segs_cap; };
ZK_HD ZkTrainLayout zkt_layout(uint32_t n, uint32_t f, uint32_t nk, uint32_t kmin, uint32_t ccap)
{
    ZkTrainLayout L;
    const size_t a = 255;
    L.stride = (ccap + ZKE_LDM_SLACK + 255u) & ~255u; L.segs_cap = ccap / kmin + 1;
    L.hpos = 0;
    L.freq = ((size_t)n * 4 + a) & ~a;
    L.content = L.freq + (((size_t)(nk + 1) << f) * 4);
    L.segs = L.content + (size_t)nk * L.stride;
    L.out = L.segs + (((size_t)nk * L.segs_cap * 4 + a) & ~a);
    L.hist = L.out + 256;
    L.end = L.hist + (((size_t)ZKT_H_WORDS * 4 + a) & ~a);
    return L;
}
// E = max(1, min(content_cap / k, N / (10 k))) epochs of N / E positions each
ZK_HD uint32_t zkt_epochs(uint32_t n, uint32_t k, uint32_t ccap)
{
    const uint32_t a = ccap / k, b = (uint32_t)((uint64_t)n / (10ull * k)), e = a < b ? a : b;
    return e ? e : 1;
}

struct ZkTrainSrc {
    const uint8_t *src;         // the first sample's first byte
    const uint64_t *off;        // count + 1 prefix sums as the caller gave them (off[0] is position 0)
    uint32_t count, n, d, f;
};
__global__ __launch_bounds__(256) void zk_k_train_count(ZkTrainSrc a, uint32_t *hpos, uint32_t *freq)
{
    const uint64_t base = a.off[0];
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < a.n; p += (uint64_t)gridDim.x * 256) {
        // the sample that holds p ends at the first offset above it (empty samples share an offset; off[count] - base = n > p)
        uint32_t lo = 1, hi = a.count;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a.off[mid] - base > p) hi = mid; else lo = mid + 1; }
        uint32_t h = ZKT_NONE;
        if (p + a.d <= a.off[lo] - base) { h = zkt_hash(a.src + p, a.d, a.f); atomicAdd(&freq[h], 1u); }
        hpos[p] = h;
    }
}

struct ZkTrainSel {
    const uint8_t *src; const uint32_t *hpos;
    uint32_t n, d, f, ccap;     // ccap: the content's capacity
    uint32_t k[ZKT_CANDS_MAX];  // blockIdx.x's segment length
    uint32_t stride;            // bytes between the candidates' content buffers (>= ccap); candidate c's content ends at c * stride + ccap
    uint32_t segs_cap;          // entries between the candidates' segment lists (>= ccap / k)
};
// out[2 c] = segments taken, out[2 c + 1] = content bytes: the segments' in the order last taken ... first taken, or, when no segment
// scored above 0, the last min(n, ccap) bytes of the samples.  freq: candidate c's copy at c << f (modified).
__global__ __launch_bounds__(ZKT_SEL_THREADS) void zk_k_train_select(ZkTrainSel s, uint32_t *freq_all, uint8_t *content_all, uint32_t *segs_all, uint32_t *out)
{
    __shared__ uint64_t pre[ZKT_PER_LANE * ZKT_SEL_THREADS + 1];
    __shared__ uint64_t red[2][ZKT_SEL_THREADS];
    __shared__ uint32_t redp[ZKT_SEL_THREADS];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, k = s.k[c], w = k - s.d + 1, per = zkt_per_lane(k);
    uint32_t *freq = freq_all + ((size_t)c << s.f), *segs = segs_all + (size_t)c * s.segs_cap;
    uint8_t *content = content_all + (size_t)c * s.stride;
    const uint32_t E = zkt_epochs(s.n, k, s.ccap), esize = s.n / E;
    uint32_t left = s.ccap, nseg = 0;
    for (bool more = true; more && left >= k;) {
        more = false;
        for (uint32_t e = 0; e < E && left >= k; e++) {
            const uint64_t lo = (uint64_t)e * esize, hi = lo + esize;
            uint64_t best = 0; uint32_t bpos = 0;
            for (uint64_t t0 = lo; t0 + k <= hi; t0 += ZKT_TILE) {
                // exclusive prefix sums of the values of positions t0 ... (a position's value: freq at its hash; 0 without a d-mer, and
                // past the epoch, where no segment of it reaches)
                uint64_t v[ZKT_PER_LANE], sum = 0;
#pragma unroll
                for (uint32_t j = 0; j < ZKT_PER_LANE; j++) {
                    const uint64_t q = t0 + (uint64_t)tid * per + j;
                    const uint32_t h = j < per && q < hi ? s.hpos[q] : ZKT_NONE;
                    v[j] = h != ZKT_NONE ? freq[h] : 0u;
                    sum += v[j];
                }
                uint32_t cur = 0;
                red[0][tid] = sum;
                __syncthreads();
                for (uint32_t st = 1; st < ZKT_SEL_THREADS; st <<= 1) {
                    red[cur ^ 1][tid] = red[cur][tid] + (tid >= st ? red[cur][tid - st] : 0);
                    cur ^= 1;
                    __syncthreads();
                }
                uint64_t run = red[cur][tid] - sum;
#pragma unroll
                for (uint32_t j = 0; j < ZKT_PER_LANE; j++) if (j < per) { pre[tid * per + j] = run; run += v[j]; }
                if (tid == ZKT_SEL_THREADS - 1) pre[per * ZKT_SEL_THREADS] = run;
                __syncthreads();
                for (uint32_t j = tid; j < ZKT_TILE && t0 + j + k <= hi; j += ZKT_SEL_THREADS) {
                    const uint64_t sc = pre[j + w] - pre[j];
                    if (sc > best) { best = sc; bpos = (uint32_t)(t0 + j); }          // (a lane's starts ascend: the lowest position stays on ties)
                }
                __syncthreads();
            }
            red[0][tid] = best; redp[tid] = bpos;
            __syncthreads();
            for (uint32_t st = ZKT_SEL_THREADS / 2; st; st >>= 1) {
                if (tid < st && (red[0][tid + st] > red[0][tid] || (red[0][tid + st] == red[0][tid] && redp[tid + st] < redp[tid]))) { red[0][tid] = red[0][tid + st]; redp[tid] = redp[tid + st]; }
                __syncthreads();
            }
            best = red[0][0]; bpos = redp[0];
            __syncthreads();
            if (best == 0) continue;
            // taken: its bytes in front of what the content holds (the first segment lies last), freq cleared at its d-mers
            for (uint32_t i = tid; i < k; i += ZKT_SEL_THREADS) content[left - k + i] = s.src[(uint64_t)bpos + i];
            for (uint32_t i = tid; i < w; i += ZKT_SEL_THREADS) { const uint32_t h = s.hpos[(uint64_t)bpos + i]; if (h != ZKT_NONE) freq[h] = 0; }
            if (tid == 0) segs[nseg] = bpos;
            nseg++; left -= k; more = true;
            __syncthreads();
        }
    }
    uint32_t bytes = s.ccap - left;
    if (!nseg) {
        bytes = s.n < s.ccap ? s.n : s.ccap;
        for (uint32_t i = tid; i < bytes; i += ZKT_SEL_THREADS) content[s.ccap - bytes + i] = s.src[(uint64_t)s.n - bytes + i];
    }
    if (tid == 0) { out[2 * c] = nseg; out[2 * c + 1] = bytes; }
}

// the samples first, first + j, first + 2 j, ... behind one another: workgroup b copies sample b * j to dst + sub_off[b] (sub_off: the
// prefix sums of the chosen samples' sizes, made on the host)
__global__ __launch_bounds__(256) void zk_k_train_gather(const uint8_t *src, const uint64_t *off, uint32_t j, const uint64_t *sub_off, uint8_t *dst)
{
    const uint64_t from = off[(uint64_t)blockIdx.x * j] - off[0], n = sub_off[blockIdx.x + 1] - sub_off[blockIdx.x];
    uint8_t *to = dst + sub_off[blockIdx.x];
    for (uint64_t i = threadIdx.x; i < n; i += 256) to[i] = src[from + i];
}

// hist[ZKT_H_WORDS] (cleared by the caller): 256 literal values | 36 literal-length codes | 53 match-length codes | 32 offset codes of all
// blocks.  32-bit counters: everything counted is at most one per sample byte, and the samples total less than 2^32.
__global__ __launch_bounds__(256) void zk_k_train_stats(const ZkEncBlock *blocks, uint32_t nb, const uint64_t *seqs, const uint8_t *lits, uint32_t *hist)
{
    __shared__ uint32_t h[ZKT_H_WORDS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < ZKT_H_WORDS; i += 256) h[i] = 0;
    __syncthreads();
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const ZkEncBlock &blk = blocks[b];
        const uint8_t *lt = lits + blk.lit_base;
        for (uint32_t i = tid; i < blk.nlit; i += 256) atomicAdd(&h[lt[i]], 1u);
        const uint64_t *sq = seqs + blk.seq_base;
        for (uint32_t i = tid; i < blk.nseq; i += 256) {
            const uint64_t e = sq[i];                                // ll | ml << 16 | Offset_Value << 32 (zk_enc_device.h)
            const uint32_t ll = (uint32_t)e & 0xFFFF, ml = (uint32_t)(e >> 16) & 0xFFFF, ob = (uint32_t)(e >> 32);
            atomicAdd(&h[ZKT_H_LL + zke_ll_code(ll)], 1u);
            atomicAdd(&h[ZKT_H_ML + zke_ml_code(ml - 3)], 1u);
            atomicAdd(&h[ZKT_H_OF + zk_highbit(ob | 1u)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < ZKT_H_WORDS; i += 256) if (h[i]) atomicAdd(&hist[i], h[i]);
}

// zk_train.hip -- zk_train_dictionary[_dev]: a zstd dictionary trained on the device (include/zeekstd_amd.h).
//   1. zk_k_train_count    d-mer frequencies of the samples (zk_train.h)
//   2. zk_k_train_select   a workgroup per candidate segment length, each on its own copy of the frequencies: a candidate content each
//   3. the choice          the samples encoded against every candidate content with the encoder's own frame-list route (the content as the
//                          prefix: byte for byte what a raw-content zk_cdict of it gives), the smallest total wins; once more without a
//                          dictionary for the report
//                          Samples above 64 MiB in all: every j-th sample, the smallest j that brings them under, gathered behind one
//                          another (zk_k_train_gather); step 4 runs on the same samples
//   4. zk_k_train_stats    the encode stages up to and including the matcher once more with the winning content as the prefix
//                          (zk_enc_args::matched), its literals and sequences counted into one set of histograms, from which the host
//                          writes the header (zk_train_host.h).  Not with ZK_TRAIN_RAW_CONTENT.
// All scratch is the encoder's (zk_engine::Enc::train, train_src): a submitted decode batch is not touched.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "../../include/zeekstd_amd.h"
#include "zk_engine.h"
#include "zk_train.h"
#include "zk_train_host.h"

constexpr uint32_t ZKT_STATS_WGS_MAX = 1024;
constexpr uint64_t ZKT_TRIAL_BYTES = 64ull << 20;        // samples above this are tried and measured on every j-th sample (ZK_CHOICE_TRAIN_TRIAL_KIB)
static void zk_launch_train_count(hipStream_t st, const ZkTrainSrc &a, uint32_t *hpos, uint32_t *freq)
{
    const uint64_t wgs = ((uint64_t)a.n + 255) / 256;
    hipLaunchKernelGGL(zk_k_train_count, dim3((uint32_t)(wgs < ZKT_COUNT_WGS_MAX ? wgs : ZKT_COUNT_WGS_MAX)), dim3(256), 0, st, a, hpos, freq);
}
static void zk_launch_train_select(hipStream_t st, const ZkTrainSel &s, uint32_t nk, uint32_t *freq_all, uint8_t *content_all, uint32_t *segs_all, uint32_t *out)
{
    hipLaunchKernelGGL(zk_k_train_select, dim3(nk), dim3(ZKT_SEL_THREADS), 0, st, s, freq_all, content_all, segs_all, out);
}

namespace {
struct ZkTrainSetup {
    uint32_t d, f, nk, k[ZKT_CANDS_MAX], ccap, flags, dict_id;
    int level;
};
// the checks that need no offsets; 0, ZK_ERR_ARGUMENT or ZK_ERR_FRAME_INDEX_TOO_LARGE
int zk_train_setup(const zk_train_params *p, uint32_t count, const void *dict_out, size_t cap, const size_t *written, ZkTrainSetup &s)
{
    static const zk_train_params defaults = {0, 0, 0, 0, 0, 0};
    if (!p) p = &defaults;
    if (count == 0 || cap < 1024 || !dict_out || !written) return ZK_ERR_ARGUMENT;
    if (count > ZK_SEEKABLE_MAX_FRAMES) return ZK_ERR_FRAME_INDEX_TOO_LARGE;         // (a sample is a frame of the trial encodes)
    s.d = p->d ? p->d : 8; s.f = p->f ? p->f : 20; s.level = p->level ? p->level : 1; s.flags = p->flags;
    if ((s.d != 6 && s.d != 8) || s.f < 10 || s.f > 24 || (p->flags & ~(uint32_t)ZK_TRAIN_RAW_CONTENT)) return ZK_ERR_ARGUMENT;
    s.dict_id = p->dict_id;
    s.nk = 0;
    if (p->k) {
        if (p->k < ZKT_K_MIN || p->k > ZKT_K_MAX || p->k > cap / 4) return ZK_ERR_ARGUMENT;
        s.k[s.nk++] = p->k;
    } else for (uint32_t k = 64; k <= 512; k *= 2) if (k <= cap / 4) s.k[s.nk++] = k;
    // (the matcher reaches the last 2^27 - 1 bytes of a dictionary's content: more is never made)
    const size_t ccap = cap - ZKT_HEADER_RESERVE;
    s.ccap = (uint32_t)(ccap < ZKE_LDM_MAX_OFF ? ccap : ZKE_LDM_MAX_OFF);
    return 0;
}
// the list: non-decreasing, no sample above a frame's largest size, below 2^32 bytes in all, at least 8 samples of d bytes
int zk_train_list_check(const uint64_t *off, uint32_t count, uint32_t d, uint64_t *n_out)
{
    uint32_t usable = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > ZK_SEEKABLE_MAX_FRAME_SIZE) return ZK_ERR_ARGUMENT;
        usable += off[i + 1] - off[i] >= d;
    }
    const uint64_t n = off[count] - off[0];
    if (n >> 32 || usable < 8) return ZK_ERR_ARGUMENT;
    *n_out = n;
    return 0;
}

// the samples the candidates are tried on: every j-th, for the smallest j whose samples total at most `limit` (j = count, the first sample
// alone, when none does); 1 = all of them
uint32_t zk_train_trial_stride(const uint64_t *off, uint32_t count, uint64_t limit)
{
    if (off[count] - off[0] <= limit) return 1;
    for (uint32_t j = 2; j < count; j++) {
        uint64_t sum = 0;
        for (uint64_t i = 0; i < count && sum <= limit; i += j) sum += off[i + 1] - off[i];
        if (sum <= limit) return j;
    }
    return count;
}

// d_samples / d_off: on the device; off: the same offsets on the host, checked.  Everything runs on st.
int zk_train_run(zk_engine *e, const void *d_samples, const void *d_off, const uint64_t *off, uint32_t count, uint64_t n64, const ZkTrainSetup &s,
                 uint8_t *dict_out, size_t *written, zk_train_report *report, hipStream_t st)
{
    const uint32_t n = (uint32_t)n64, nk = s.nk;
    const size_t fsize = (size_t)1 << s.f;
    const ZkTrainLayout L = zkt_layout(n, s.f, nk, s.k[0], s.ccap);
    // the trial set: all samples, or every j-th behind one another with offsets of their own
    const uint32_t j = zk_train_trial_stride(off, count, e->enc.train_trial_bytes ? e->enc.train_trial_bytes : ZKT_TRIAL_BYTES);
    const uint32_t tcount = (count + j - 1) / j;
    std::vector<uint64_t> sub;
    if (j > 1) {
        sub.resize((size_t)tcount + 1);
        sub[0] = 0;
        for (uint32_t i = 0; i < tcount; i++) sub[i + 1] = sub[i] + (off[(size_t)i * j + 1] - off[(size_t)i * j]);
    }
    const uint64_t tn = j > 1 ? sub[tcount] : n64;
    const uint64_t bound = zk_compress_bound_list(tn, tcount, 0);
    const size_t sub_off_b = j > 1 ? (((size_t)tcount + 1) * 8 + 255) & ~(size_t)255 : 0, sub_src_b = j > 1 ? ((size_t)tn + 64 + 255) & ~(size_t)255 : 0;
    int rc;
    if ((rc = zk_devbuf_reserve(e, e->enc.train, L.end + sub_off_b + sub_src_b + (size_t)bound + 64))) return rc;
    uint8_t *base = (uint8_t *)e->enc.train.p;
    uint32_t *hpos = (uint32_t *)(base + L.hpos), *freq = (uint32_t *)(base + L.freq), *segs = (uint32_t *)(base + L.segs), *out = (uint32_t *)(base + L.out);
    uint32_t *d_hist = (uint32_t *)(base + L.hist);
    uint8_t *content = base + L.content;
    uint64_t *d_sub_off = (uint64_t *)(base + L.end);
    uint8_t *d_sub_src = base + L.end + sub_off_b, *dst = d_sub_src + sub_src_b;
    zk_profile_begin(e);
    ZK_HIP(hipMemsetAsync(freq, 0, fsize * 4, st));
    ZK_HIP(hipMemsetAsync(content, 0, (size_t)nk * L.stride, st));
    const ZkTrainSrc src{(const uint8_t *)d_samples + off[0], (const uint64_t *)d_off, count, n, s.d, s.f};
    { zk_kernel_timer t(e, ZK_K_TRAIN_COUNT, st); zk_launch_train_count(st, src, hpos, freq); }
    for (uint32_t c = 0; c < nk; c++) ZK_HIP(hipMemcpyAsync(freq + (c + 1) * fsize, freq, fsize * 4, hipMemcpyDeviceToDevice, st));
    ZkTrainSel sel{src.src, hpos, n, s.d, s.f, s.ccap, {0, 0, 0, 0}, L.stride, L.segs_cap};
    for (uint32_t c = 0; c < nk; c++) sel.k[c] = s.k[c];
    { zk_kernel_timer t(e, ZK_K_TRAIN_SELECT, st); zk_launch_train_select(st, sel, nk, freq + fsize, content, segs, out); }
    const void *t_src = d_samples, *t_off = d_off;
    if (j > 1) {
        ZK_HIP(hipMemcpyAsync(d_sub_off, sub.data(), ((size_t)tcount + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(zk_k_train_gather, dim3(tcount), dim3(256), 0, st, src.src, src.off, j, d_sub_off, d_sub_src);
        t_src = d_sub_src; t_off = d_sub_off;
    }
    uint32_t res[2 * ZKT_CANDS_MAX];
    ZK_HIP(hipMemcpyAsync(res, out, 2 * nk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_HIP(hipGetLastError());
    zk_profile_collect(e);
    // the choice: existing code, called with per-kernel timing off (its own begin / collect would clear the times above)
    uint64_t with[ZKT_CANDS_MAX], without = 0;
    uint32_t win = 0;
    {
        zk_profiling_off quiet(e);
        for (uint32_t c = 0; c < nk; c++) {
            const uint32_t bytes = res[2 * c + 1];
            if ((rc = zk_encode_frame_list_dev(e, t_src, t_off, tcount, s.level, 0, content + (size_t)c * L.stride + (s.ccap - bytes), bytes, nullptr,
                                               dst, bound, nullptr, nullptr, &with[c], st))) return rc;
            if (with[c] < with[win]) win = c;           // (ascending k: a tie stays with the smaller)
        }
        if (report && (rc = zk_encode_frame_list_dev(e, t_src, t_off, tcount, s.level, 0, nullptr, 0, nullptr, dst, bound, nullptr, nullptr, &without, st))) return rc;
    }
    const uint32_t bytes = res[2 * win + 1];
    const uint8_t *chosen = content + (size_t)win * L.stride + (s.ccap - bytes);
    uint8_t head[ZKT_HEADER_RESERVE];
    size_t hb = 0;
    std::vector<uint8_t> host((size_t)bytes);
    if (!(s.flags & ZK_TRAIN_RAW_CONTENT)) {
        // the tables: what the matcher makes of the trial samples against the chosen content
        uint32_t hist[ZKT_H_WORDS];
        ZkEncMatched m;
        {
            zk_profiling_off quiet(e);
            if ((rc = zk_encode_frame_list_matched(e, t_src, t_off, tcount, s.level, chosen, bytes, dst, bound, &m, st))) return rc;
        }
        ZK_HIP(hipMemsetAsync(d_hist, 0, sizeof hist, st));
        if (m.nb) {
            zk_kernel_timer t(e, ZK_K_TRAIN_STATS, st);
            hipLaunchKernelGGL(zk_k_train_stats, dim3(m.nb < ZKT_STATS_WGS_MAX ? m.nb : ZKT_STATS_WGS_MAX), dim3(256), 0, st, m.blocks, m.nb, m.seqs, m.lits, d_hist);
        }
        ZK_HIP(hipMemcpyAsync(hist, d_hist, sizeof hist, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(host.data(), chosen, bytes, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipGetLastError());
        zk_profile_collect(e);
        uint64_t h64[ZKT_H_WORDS];
        for (uint32_t i = 0; i < ZKT_H_WORDS; i++) h64[i] = hist[i];
        const uint32_t id = s.dict_id ? s.dict_id : zkt_dict_id(host.data(), bytes);
        hb = zkt_write_header(h64, h64 + ZKT_H_LL, h64 + ZKT_H_ML, h64 + ZKT_H_OF, id, head, sizeof head);
        if (!hb) return -(int)ZK_E_GENERIC;
    } else {
        ZK_HIP(hipMemcpyAsync(host.data(), chosen, bytes, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
    }
    // (the header takes less than its reserve: the content moves up to it)
    memcpy(dict_out, head, hb);
    memcpy(dict_out + hb, host.data(), bytes);
    *written = hb + bytes;
    if (report) *report = zk_train_report{s.k[win], res[2 * win], bytes, (uint32_t)hb, n64, with[win], without};
    return 0;
}
}  // namespace

extern "C" int zk_train_dictionary_dev(zk_engine *e, const void *d_samples, const void *d_off, uint32_t count, const zk_train_params *p,
                                       uint8_t *dict_out, size_t cap, size_t *written, zk_train_report *report, void *stream)
{
    ZkTrainSetup s;
    if (!e || !d_off) return ZK_ERR_ARGUMENT;
    if (const int rc = zk_train_setup(p, count, dict_out, cap, written, s)) return rc;
    ZK_HIP(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    std::vector<uint64_t> off((size_t)count + 1);
    ZK_HIP(hipMemcpyAsync(off.data(), d_off, off.size() * 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    uint64_t n = 0;
    if (const int rc = zk_train_list_check(off.data(), count, s.d, &n)) return rc;
    if (!d_samples) return ZK_ERR_ARGUMENT;
    return zk_train_run(e, d_samples, d_off, off.data(), count, n, s, dict_out, written, report, st);
}

extern "C" int zk_train_dictionary(zk_engine *e, const uint8_t *samples, const uint64_t *off, uint32_t count, const zk_train_params *p,
                                   uint8_t *dict_out, size_t cap, size_t *written, zk_train_report *report)
{
    ZkTrainSetup s;
    if (!e || !off) return ZK_ERR_ARGUMENT;
    if (const int rc = zk_train_setup(p, count, dict_out, cap, written, s)) return rc;
    uint64_t n = 0;
    if (const int rc = zk_train_list_check(off, count, s.d, &n)) return rc;
    if (!samples) return ZK_ERR_ARGUMENT;
    ZK_HIP(hipSetDevice(e->device));
    // the samples and their offsets, counted from the first sample, go up once; from there on it is the device entry point's path
    const size_t off_b = ((size_t)count + 1) * 8;
    if (const int rc = zk_devbuf_reserve(e, e->enc.train_src, (size_t)n + 64 + off_b)) return rc;
    uint8_t *d_samples = (uint8_t *)e->enc.train_src.p;
    uint64_t *d_off = (uint64_t *)(d_samples + (((size_t)n + 63) & ~(size_t)63));
    std::vector<uint64_t> rel((size_t)count + 1);
    for (uint32_t i = 0; i <= count; i++) rel[i] = off[i] - off[0];
    ZK_HIP(hipMemcpyAsync(d_samples, samples + off[0], (size_t)n, hipMemcpyHostToDevice, e->stream));
    ZK_HIP(hipMemcpyAsync(d_off, rel.data(), off_b, hipMemcpyHostToDevice, e->stream));
    ZK_HIP(hipStreamSynchronize(e->stream));
    return zk_train_run(e, d_samples, d_off, rel.data(), count, n, s, dict_out, written, report, e->stream);
}

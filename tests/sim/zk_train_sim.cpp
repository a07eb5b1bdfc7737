// zk_train_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels that select a trained dictionary's content (zeekstd_amd/csrc/zk_train.h, the very source hipcc compiles for gfx950) on
// the CPU, one workgroup at a time, under the fiber emulator of hip_wg_emu.h, with the launchers' grids and the scratch layout of
// zk_train_run (zk_train.hip).  tests/test_sim_train.py compares what they leave -- every position's hash, the counters, the segments taken
// and the content -- with the numpy model of tests/helpers/train_model.py; tests/sim/train_san.cpp runs the same under AddressSanitizer +
// UBSan.  Every buffer a kernel sees is a heap allocation of EXACTLY the size the engine gives it, filled with a poison pattern first.
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_train.h"
#include <memory>

template <class T> static std::unique_ptr<T[]> zkt_exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

// buf: the caller's buffer, off[count + 1] as given (the samples are buf[off[0], off[count])); ks[nk] ascending.  Outputs: hpos_out[n],
// freq_out[1 << f] (as counted), segs_out[nk * segs_cap], content_out[nk * ccap] (a candidate's content ends at the end of its row),
// out[2 nk].  Returns 0; -2: a candidate wrote into the slack behind its content.
extern "C" int zk_train_sim(const uint8_t *buf, const uint64_t *off_in, uint32_t count, uint32_t d, uint32_t f, const uint32_t *ks, uint32_t nk, uint32_t ccap,
                            int descending, uint32_t *hpos_out, uint32_t *freq_out, uint32_t *segs_out, uint32_t segs_cap, uint8_t *content_out, uint32_t *out)
{
    const uint32_t n = (uint32_t)(off_in[count] - off_in[0]);
    const size_t fsize = (size_t)1 << f;
    // exact copies: the samples alone (nothing readable behind the last one), the offsets
    const auto src = zkt_exact<uint8_t>(n);
    memcpy(src.get(), buf + off_in[0], n);
    const auto off = zkt_exact<uint64_t>((size_t)count + 1);
    memcpy(off.get(), off_in, ((size_t)count + 1) * 8);
    // the layout zk_train_run reserves (zkt_layout, shared): every array of exactly the bytes it has there
    const ZkTrainLayout L = zkt_layout(n, f, nk, ks[0], ccap);
    const uint32_t stride = L.stride;
    if (segs_cap != L.segs_cap || L.content - L.freq != (nk + 1) * fsize * 4 || L.segs - L.content != (size_t)nk * stride) return -3;
    const auto hpos = zkt_exact<uint32_t>(n), freq = zkt_exact<uint32_t>((nk + 1) * fsize), segs = zkt_exact<uint32_t>((size_t)nk * segs_cap), res = zkt_exact<uint32_t>(2 * nk);
    const auto content = zkt_exact<uint8_t>((size_t)nk * stride);
    for (uint32_t i = 0; i < n; i++) hpos[i] = 0xA5A5A5A5u;
    for (size_t i = 0; i < (nk + 1) * fsize; i++) freq[i] = 0xA5A5A5A5u;
    for (size_t i = 0; i < (size_t)nk * segs_cap; i++) segs[i] = 0xA5A5A5A5u;
    // "hipMemsetAsync(freq, 0, fsize * 4)", "hipMemsetAsync(content, 0, cont_b)"
    memset(freq.get(), 0, fsize * 4);
    memset(content.get(), 0, (size_t)nk * stride);
    emu_set_lane_order(descending != 0);
    // zk_launch_train_count: "wgs = (n + 255) / 256", "dim3(wgs < ZKT_COUNT_WGS_MAX ? wgs : ZKT_COUNT_WGS_MAX), dim3(256)"
    const ZkTrainSrc a{src.get(), off.get(), count, n, d, f};
    const uint64_t wgs = ((uint64_t)n + 255) / 256;
    const uint32_t gx = (uint32_t)(wgs < ZKT_COUNT_WGS_MAX ? wgs : ZKT_COUNT_WGS_MAX);
    for (uint32_t b = 0; b < gx; b++) emu_run_workgroup(256, b, [&]() { zk_k_train_count(a, hpos.get(), freq.get()); }, gx);
    memcpy(hpos_out, hpos.get(), (size_t)n * 4);
    memcpy(freq_out, freq.get(), fsize * 4);
    // "hipMemcpyAsync(freq + (c + 1) * fsize, freq, ...)" per candidate, then "zk_k_train_select, dim3(nk), dim3(ZKT_SEL_THREADS)" on freq + fsize
    for (uint32_t c = 0; c < nk; c++) memcpy(freq.get() + (c + 1) * fsize, freq.get(), fsize * 4);
    ZkTrainSel s{src.get(), hpos.get(), n, d, f, ccap, {0, 0, 0, 0}, stride, segs_cap};
    for (uint32_t c = 0; c < nk; c++) s.k[c] = ks[c];
    for (uint32_t c = 0; c < nk; c++)
        emu_run_workgroup(ZKT_SEL_THREADS, c, [&]() { zk_k_train_select(s, freq.get() + fsize, content.get(), segs.get(), res.get()); }, nk);
    emu_set_lane_order(false);
    int rc = 0;
    for (uint32_t c = 0; c < nk; c++) {
        memcpy(content_out + (size_t)c * ccap, content.get() + (size_t)c * stride, ccap);
        for (uint32_t i = ccap; i < stride; i++) if (content[(size_t)c * stride + i]) rc = -2;
    }
    memcpy(segs_out, segs.get(), (size_t)nk * segs_cap * 4);
    memcpy(out, res.get(), 2 * nk * 4);
    return rc;
}

// zk_k_train_stats over nb blocks with the launcher's grid ("dim3(m.nb < ZKT_STATS_WGS_MAX ? ...)" = wgs here): nseq / nlit / seq_base /
// lit_base per block, the packed sequences and the literals in exact-size copies.  hist_out[ZKT_H_WORDS].
extern "C" int zk_train_sim_stats(const uint32_t *nseq, const uint32_t *nlit, const uint64_t *seq_base, const uint64_t *lit_base, uint32_t nb,
                                  const uint64_t *seqs_in, uint64_t nseqs, const uint8_t *lits_in, uint64_t nlits, uint32_t wgs, int descending, uint32_t *hist_out)
{
    const auto blocks = zkt_exact<ZkEncBlock>(nb);
    memset(blocks.get(), 0, (size_t)nb * sizeof(ZkEncBlock));
    for (uint32_t b = 0; b < nb; b++) { blocks[b].nseq = nseq[b]; blocks[b].nlit = nlit[b]; blocks[b].seq_base = seq_base[b]; blocks[b].lit_base = lit_base[b]; }
    const auto seqs = zkt_exact<uint64_t>(nseqs);
    memcpy(seqs.get(), seqs_in, nseqs * 8);
    const auto lits = zkt_exact<uint8_t>(nlits);
    memcpy(lits.get(), lits_in, nlits);
    const auto hist = zkt_exact<uint32_t>(ZKT_H_WORDS);
    memset(hist.get(), 0, ZKT_H_WORDS * 4);
    emu_set_lane_order(descending != 0);
    for (uint32_t b = 0; b < wgs; b++) emu_run_workgroup(256, b, [&]() { zk_k_train_stats(blocks.get(), nb, seqs.get(), lits.get(), hist.get()); }, wgs);
    emu_set_lane_order(false);
    memcpy(hist_out, hist.get(), ZKT_H_WORDS * 4);
    return 0;
}
// zk_k_train_gather, a workgroup per chosen sample; dst_out[sub_off[m]]
extern "C" int zk_train_sim_gather(const uint8_t *buf, const uint64_t *off_in, uint32_t count, uint32_t j, const uint64_t *sub_off_in, uint32_t m, uint8_t *dst_out)
{
    const uint32_t n = (uint32_t)(off_in[count] - off_in[0]);
    const auto src = zkt_exact<uint8_t>(n);
    memcpy(src.get(), buf + off_in[0], n);
    const auto off = zkt_exact<uint64_t>((size_t)count + 1), sub = zkt_exact<uint64_t>((size_t)m + 1);
    memcpy(off.get(), off_in, ((size_t)count + 1) * 8);
    memcpy(sub.get(), sub_off_in, ((size_t)m + 1) * 8);
    const auto dst = zkt_exact<uint8_t>((size_t)sub_off_in[m]);
    memset(dst.get(), 0xA5, (size_t)sub_off_in[m]);
    for (uint32_t b = 0; b < m; b++) emu_run_workgroup(256, b, [&]() { zk_k_train_gather(src.get(), off.get(), j, sub.get(), dst.get()); }, m);
    memcpy(dst_out, dst.get(), (size_t)sub_off_in[m]);
    return 0;
}

// zk_cdc_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels that find content-defined frame boundaries (zeekstd_amd/csrc/zk_cdc.h, the very source hipcc compiles for gfx950) on the
// CPU, one workgroup at a time, under the fiber emulator of hip_wg_emu.h, with the launchers' grids, the slices and the scratch layout of
// zk_cdc_pass (zk_cdc.hip).  tests/test_sim_cdc.py compares what they leave -- the candidate bitmap and the offsets -- with the numpy model
// of tests/helpers/cdc_model.py; tests/sim/cdc_san.cpp runs the same under AddressSanitizer + UBSan.  Every buffer a kernel sees is a heap
// allocation of EXACTLY the size the engine gives it, filled with a poison pattern first; the source is an exact copy that starts
// `misalign` bytes into its allocation and ends with it.
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_cdc.h"
#include <memory>

template <class T> static std::unique_ptr<T[]> zkc_exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

// src[n] (n > 0); slice_bytes: what ZK_CHOICE_CDC_SLICE_KIB gives (0 = the default, 64 MiB).  Outputs: bitmap_out[(n + 7) / 8] (position p
// is bit p & 7 of byte p >> 3), off_out[off_cap + 1], *count_out (the cuts behind off[0], also those without room).  off_out may be null: a
// counting pass.  Returns 0; -2: the chain did not end at n; -3: a tile's bitmap words behind the slice's end are not zero.
extern "C" int zk_cdc_sim(const uint8_t *src_in, uint64_t n, uint32_t min, uint32_t bits, uint32_t max, uint64_t slice_bytes, uint32_t misalign, int descending,
                          uint8_t *bitmap_out, uint64_t *off_out, uint64_t off_cap, uint64_t *count_out)
{
    const auto block = zkc_exact<uint8_t>((size_t)n + misalign);
    memset(block.get(), 0xEE, misalign);
    uint8_t *src = block.get() + misalign;
    memcpy(src, src_in, (size_t)n);
    // zk_cdc_pass: "slice = n < slice_max ? n : slice_max", the layout of one slice
    const uint64_t slice_max = slice_bytes ? slice_bytes : 64ull << 20, slice = n < slice_max ? n : slice_max;
    const ZkCdcLayout L = zkc_layout(slice, min, bits);
    if (L.counts - L.bitmap != (size_t)L.tiles * ZKC_THREADS * 16 || L.bases - L.counts != (size_t)L.tiles * 8 || L.end - L.list != (size_t)slice * 4) return -4;
    const auto bitmap = zkc_exact<uint4>((size_t)L.tiles * ZKC_THREADS);
    const auto counts = zkc_exact<uint64_t>(L.tiles), bases = zkc_exact<uint64_t>((size_t)L.tiles + 1);
    const auto list = zkc_exact<uint32_t>((size_t)slice);
    if (L.rows - L.runs < (size_t)L.g.nseg * sizeof(ZkCdcRun) || L.runs - L.meta != (size_t)L.g.nseg * sizeof(ZkCdcSegMeta) || L.list - L.rows != (size_t)L.g.nseg * L.g.row * 8) return -4;
    const auto rows = zkc_exact<uint64_t>((size_t)L.g.nseg * L.g.row);
    const auto meta = zkc_exact<ZkCdcSegMeta>(L.g.nseg);
    const auto runs = zkc_exact<ZkCdcRun>(L.g.nseg);
    uint64_t nruns = 0xA5A5A5A5A5A5A5A5ull;
    for (size_t i = 0; i < (size_t)L.g.nseg * L.g.row; i++) rows[i] = 0xA5A5A5A5A5A5A5A5ull;
    const auto off = zkc_exact<uint64_t>(off_out ? (size_t)off_cap + 1 : 0);
    memset(bitmap.get(), 0xA5, (size_t)L.tiles * ZKC_THREADS * 16);
    for (size_t i = 0; i < slice; i++) list[i] = 0xA5A5A5A5u;
    for (size_t i = 0; off_out && i <= off_cap; i++) off[i] = 0xA5A5A5A5A5A5A5A5ull;
    // "hipMemsetAsync(state, 0, ...)", "hipMemsetAsync(d_off, 0, 8)"
    ZkCdcState state{0, 0};
    if (off_out) off[0] = 0;
    emu_set_lane_order(descending != 0);
    int rc = 0;
    for (uint64_t s0 = 0; s0 < n; s0 += slice) {
        const uint64_t len = n - s0 < slice ? n - s0 : slice;
        const uint32_t tiles = zkc_tiles(len);
        const ZkCdcSlice a{src, 0, s0, len, bits};
        for (uint32_t t = 0; t < tiles; t++) emu_run_workgroup(ZKC_THREADS, t, [&]() { zk_k_cdc_mark(a, bitmap.get(), counts.get()); }, tiles);
        // zk_k_scan64 (zk_encode.hip), restated: the exclusive scan, the total behind it
        bases[0] = 0;
        for (uint32_t t = 0; t < tiles; t++) bases[t + 1] = bases[t] + counts[t];
        for (uint32_t t = 0; t < tiles; t++) emu_run_workgroup(ZKC_THREADS, t, [&]() { zk_k_cdc_emit(bitmap.get(), bases.get(), list.get()); }, tiles);
        // "nseg == 1 ? zk_k_cdc_select : zk_k_cdc_spec (dim3(nseg)), zk_k_cdc_fix, zk_k_cdc_copy (dim3(nseg))"
        const uint32_t nseg = (uint32_t)((len + L.g.seg - 1) / L.g.seg);
        const ZkCdcSel sel{n, s0, s0 + len, min, max, off_cap, L.g.seg, nseg, L.g.row};
        uint64_t *d_off = off_out ? off.get() : nullptr;
        if (nseg == 1) emu_run_workgroup(ZKC_SEL_THREADS, 0, [&]() { zk_k_cdc_select(sel, list.get(), bases.get() + tiles, &state, d_off); }, 1);
        else {
            for (uint32_t k = 0; k < nseg; k++) emu_run_workgroup(ZKC_SEL_THREADS, k, [&]() { zk_k_cdc_spec(sel, list.get(), bases.get() + tiles, rows.get(), meta.get()); }, nseg);
            emu_run_workgroup(ZKC_SEL_THREADS, 0, [&]() { zk_k_cdc_fix(sel, list.get(), bases.get() + tiles, rows.get(), meta.get(), &state, d_off, runs.get(), &nruns); }, 1);
            for (uint32_t k = 0; k < nseg; k++) emu_run_workgroup(ZKC_THREADS, k, [&]() { zk_k_cdc_copy(sel, rows.get(), runs.get(), &nruns, d_off); }, nseg);
        }
        const uint8_t *bm = (const uint8_t *)bitmap.get();
        memcpy(bitmap_out + s0 / 8, bm, (size_t)((len + 7) / 8));
        for (size_t i = (size_t)((len + 7) / 8); i < (size_t)tiles * ZKC_THREADS * 16; i++) if (bm[i]) rc = -3;
    }
    emu_set_lane_order(false);
    if (state.cut != n) rc = -2;
    *count_out = state.count;
    if (off_out) memcpy(off_out, off.get(), ((size_t)off_cap + 1) * 8);
    return rc;
}

// zk_compact_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels that remove frames from an archive (zeekstd_amd/csrc/zk_compact.h, the very source hipcc compiles for gfx950) on the CPU
// under the emulator of hip_wg_emu.h, with the launchers' grids, the scratch layout and the steps of zk_compact.hip: the plan functions of
// zk_compact.h decide here what they decide in the engine.  tests/test_sim_compact.py compares what the kernels leave -- remap, the offsets,
// every byte of the destination -- with the model of tests/helpers/compact_model.py; tests/sim/compact_san.cpp runs the same under
// AddressSanitizer + UBSan.  Every buffer a kernel sees is a heap allocation of EXACTLY the size the engine gives it, filled with a poison
// pattern first: the source is a copy that starts `misalign` bytes into its allocation and ends with the archive's last byte; a destination
// of its own ends with the last byte written; a staged step's scratch is exactly the step.
//   No kernel of zk_compact.h has a barrier or a wave collective, so their lanes run one after the other (zkd_flat), in ascending or
// descending order of lanes AND workgroups.  The index (zk_dedup_index_compact_dev) sits on the harness of zk_dedup_index_sim.cpp.
#include "zk_dedup_index_sim.cpp"
#include "../../zeekstd_amd/csrc/zk_compact.h"

static_assert(ZKC_THREADS == ZKD_THREADS, "zkd_flat runs workgroups of ZKD_THREADS lanes");

// the plan functions, for literal expectations
extern "C" int zkc_sim_step_direct(uint64_t removed_before_step, uint64_t step_bytes) { return zkc_step_direct(removed_before_step, step_bytes) ? 1 : 0; }
extern "C" uint64_t zkc_sim_step_bytes(uint64_t slice) { return zkc_step_bytes(slice); }
extern "C" uint64_t zkc_sim_nsteps(uint64_t moved, uint64_t step) { return zkc_nsteps(moved, step); }
extern "C" uint64_t zkc_sim_step_begin(uint64_t k, uint64_t step) { return zkc_step_begin(k, step); }
extern "C" uint64_t zkc_sim_step_end(uint64_t k, uint64_t step, uint64_t moved) { return zkc_step_end(k, step, moved); }
extern "C" uint64_t zkc_sim_stage_bytes(uint64_t moved, uint64_t step) { return zkc_stage_bytes(moved, step); }
extern "C" uint32_t zkc_sim_move_grid(uint64_t bytes) { return zkc_move_grid(bytes); }
extern "C" uint32_t zkc_sim_tile(void) { return ZKC_TILE; }

// "zk_mark_frames_dev": live (n_frames bytes) marked with ids; returns 0, or -100 (ZK_ERR_ARGUMENT's place) with live untouched
extern "C" int zk_compact_sim_mark(const uint32_t *ids_in, uint32_t count, uint32_t n_frames, uint8_t *live_io, int descending)
{
    if (count == 0) return 0;
    const bool desc = descending != 0;
    const auto ids = zkd_exact<uint32_t>(count), err = zkd_exact<uint32_t>(1, 0);
    const auto live = zkd_exact<uint8_t>(n_frames);
    memcpy(ids.get(), ids_in, (size_t)count * 4);
    memcpy(live.get(), live_io, n_frames);
    emu_set_lane_order(desc);
    zkd_flat(zkc_blocks(count), desc, [&] { zk_k_cmp_check_ids(ids.get(), count, n_frames, err.get()); });
    if (err[0] == 0) zkd_flat(zkc_blocks(count), desc, [&] { zk_k_cmp_mark(ids.get(), count, live.get()); });
    emu_set_lane_order(false);
    if (err[0]) return -100;
    memcpy(live_io, live.get(), n_frames);
    return 0;
}

// "zk_remap_ids_dev": out (count) = remap[ids]; returns 0, or -100 with out untouched
extern "C" int zk_compact_sim_remap_ids(const uint32_t *remap_in, uint32_t n_frames, const uint32_t *ids_in, uint32_t count, uint32_t *out_io, int descending)
{
    if (count == 0) return 0;
    const bool desc = descending != 0;
    const auto remap = zkd_exact<uint32_t>(n_frames), ids = zkd_exact<uint32_t>(count), out = zkd_exact<uint32_t>(count), err = zkd_exact<uint32_t>(1, 0);
    memcpy(remap.get(), remap_in, (size_t)n_frames * 4);
    memcpy(ids.get(), ids_in, (size_t)count * 4);
    emu_set_lane_order(desc);
    zkd_flat(zkc_blocks(count), desc, [&] { zk_k_cmp_remap_ids(remap.get(), n_frames, ids.get(), count, out.get(), err.get()); });
    emu_set_lane_order(false);
    if (err[0]) return -100;
    memcpy(out_io, out.get(), (size_t)count * 4);
    return 0;
}

// "zk_compact_archive_dev".  comp_in[c_end]: the archive's buffer up to its last byte, c_end = c_off[n] (the bytes before c_off[0] belong to
// nobody); slice_bytes: what ZK_CHOICE_COMPACT_SLICE_KIB gives (0 = the default).  Outputs: remap_out (n), c_out / d_out (n + 1; n_kept + 1
// written), *n_kept, *written, and buf_out[c_end]: in place the whole buffer as the call leaves it; out of place the destination's bytes
// [0, written), the rest 0.  *steps_out / *staged_out: the in-place steps, and how many of them went through scratch.
// Returns 0; -100: refused for its offsets; -3: the layout is not what the harness allocates; -5: a kernel wrote outside its output
extern "C" int zk_compact_sim(const uint8_t *comp_in, uint32_t misalign, const uint64_t *c_off_in, const uint64_t *d_off_in, uint32_t n, const uint8_t *live_in,
                              int in_place, uint64_t slice_bytes, int descending, uint32_t *remap_out, uint64_t *c_out, uint64_t *d_out, uint32_t *n_kept_out,
                              uint64_t *written_out, uint8_t *buf_out, uint32_t *steps_out, uint32_t *staged_out)
{
    if (n == 0) return -1;
    const uint64_t c_end = c_off_in[n];
    const auto block = zkd_exact<uint8_t>((size_t)c_end + misalign, 0xEE);
    uint8_t *comp = block.get() + misalign;
    if (c_end) memcpy(comp, comp_in, (size_t)c_end);
    const ZkCmpLayout L = zkc_layout(n);
    const size_t a = 8 * ((size_t)n + 2);
    if (L.pk - L.fk != a || L.fc - L.pk != a || L.pc - L.fc != a || L.fd - L.pc != a || L.pd - L.fd != a || L.co - L.pd != a || L.dof - L.co != a || L.rsrc - L.dof != a ||
        L.rdst - L.rsrc != a || L.remap - L.rdst != a || L.words - L.remap < (size_t)4 * n || L.end - L.words != 8 * ZKC_W_WORDS) return -3;
    const auto c_off = zkd_exact<uint64_t>((size_t)n + 1), d_off = zkd_exact<uint64_t>((size_t)n + 1);
    const auto live = zkd_exact<uint8_t>(n);
    const auto fk = zkd_exact<uint64_t>((size_t)n + 1), fc = zkd_exact<uint64_t>((size_t)n + 1), fd = zkd_exact<uint64_t>((size_t)n + 1);
    const auto pk = zkd_exact<uint64_t>((size_t)n + 2), pc = zkd_exact<uint64_t>((size_t)n + 2), pd = zkd_exact<uint64_t>((size_t)n + 2);
    const auto co = zkd_exact<uint64_t>((size_t)n + 1), dof = zkd_exact<uint64_t>((size_t)n + 1), rsrc = zkd_exact<uint64_t>((size_t)n + 2), rdst = zkd_exact<uint64_t>((size_t)n + 2);
    const auto remap = zkd_exact<uint32_t>(n);
    const auto words = zkd_exact<uint64_t>(ZKC_W_WORDS, 0);          // "hipMemsetAsync(words, 0, ...)"
    memcpy(c_off.get(), c_off_in, ((size_t)n + 1) * 8);
    memcpy(d_off.get(), d_off_in, ((size_t)n + 1) * 8);
    memcpy(live.get(), live_in, n);
    const bool desc = descending != 0;
    emu_set_lane_order(desc);
    const uint64_t step = zkc_step_bytes(slice_bytes);
    const uint32_t max_steps = !in_place ? 0 : (uint32_t)(c_end / step + 2);
    const auto gaps = zkd_exact<uint64_t>(max_steps);
    const uint32_t grid = zkc_blocks((uint64_t)n + 1);
    zkd_flat(grid, desc, [&] { zk_k_cmp_flags(c_off.get(), d_off.get(), live.get(), n, fk.get(), fc.get(), fd.get(), (uint32_t *)words.get()); });
    // zk_k_scan64 (zk_encode.hip), restated, three times: the exclusive scan of n + 1 values, the total behind it
    const auto scan = [&](const uint64_t *in, uint64_t *out) { out[0] = 0; for (uint32_t i = 0; i <= n; i++) out[i + 1] = out[i] + in[i]; };
    scan(fk.get(), pk.get()); scan(fc.get(), pc.get()); scan(fd.get(), pd.get());
    zkd_flat(grid, desc, [&] { zk_k_cmp_emit(c_off.get(), d_off.get(), n, fk.get(), pk.get(), pc.get(), pd.get(), remap.get(), co.get(), dof.get(), rsrc.get(), rdst.get(), words.get()); });
    if (in_place) zkd_flat(zkc_blocks(max_steps), desc, [&] { zk_k_cmp_step_gaps(rsrc.get(), rdst.get(), words.get(), step, max_steps, gaps.get()); });
    int rc = 0;
    uint32_t steps = 0, staged = 0;
    const uint32_t nk = (uint32_t)words[ZKC_W_KEPT], nruns = (uint32_t)words[ZKC_W_RUNS];
    const uint64_t wr = words[ZKC_W_WRITTEN];
    if ((uint32_t)words[ZKC_W_ERR] || words[ZKC_W_END] > c_end) rc = -100;
    memset(buf_out, 0, (size_t)c_end);
    if (rc == 0) {
        for (uint32_t k = nk + 1; k <= n; k++) if (co[k] != 0xA5A5A5A5A5A5A5A5ull || dof[k] != 0xA5A5A5A5A5A5A5A5ull) rc = -5;
        for (uint32_t r = nruns + 1; r < n + 2; r++) if (rdst[r] != 0xA5A5A5A5A5A5A5A5ull) rc = -5;
        const uint64_t lo = in_place ? words[ZKC_W_FIRST_REMOVED] : words[ZKC_W_BEGIN], moved = wr > lo ? wr - lo : 0;
        if (!in_place) {
            // a destination of exactly `written` bytes; what lies before c_off[0] must stay as it is
            const auto dst = zkd_exact<uint8_t>((size_t)wr, 0xA5);
            if (nruns && moved)
                zkd_flat(zkc_move_grid(wr - lo), desc, [&] { zk_k_cmp_move(comp, dst.get(), 0, rsrc.get(), rdst.get(), nruns, lo, wr); });
            for (uint64_t p = 0; p < lo && p < wr; p++) if (dst[p] != 0xA5) rc = -5;
            memcpy(buf_out, dst.get(), (size_t)wr);
        } else {
            const uint64_t nsteps = zkc_nsteps(moved, step);
            for (uint64_t k = 0; k < nsteps && nruns; k++) {
                const uint64_t x = lo + zkc_step_begin(k, step), z = lo + zkc_step_end(k, step, moved);
                steps++;
                if (zkc_step_direct(k < max_steps ? gaps[k] : 0, z - x))
                    zkd_flat(zkc_move_grid(z - x), desc, [&] { zk_k_cmp_move(comp, comp, 0, rsrc.get(), rdst.get(), nruns, x, z); });
                else {
                    if (z - x > zkc_stage_bytes(moved, step)) rc = -3;
                    const auto stage = zkd_exact<uint8_t>((size_t)(z - x));      // (exactly the step: the engine's scratch holds the longest)
                    zkd_flat(zkc_move_grid(z - x), desc, [&] { zk_k_cmp_move(comp, stage.get(), x, rsrc.get(), rdst.get(), nruns, x, z); });
                    memcpy(comp + x, stage.get(), (size_t)(z - x));              // "hipMemcpyAsync(dst + a, stage, z - a)"
                    staged++;
                }
            }
            if (c_end) memcpy(buf_out, comp, (size_t)c_end);
        }
        for (uint32_t m = 0; m < misalign; m++) if (block[m] != 0xEE) rc = -5;
        memcpy(remap_out, remap.get(), (size_t)n * 4);
        memcpy(c_out, co.get(), ((size_t)nk + 1) * 8);
        memcpy(d_out, dof.get(), ((size_t)nk + 1) * 8);
    }
    emu_set_lane_order(false);
    *n_kept_out = rc ? 0 : nk;
    *written_out = rc ? 0 : wr;
    *steps_out = steps;
    *staged_out = staged;
    return rc;
}

// "zk_dedup_index_compact_dev" on the index of zk_dedup_index_sim.cpp: remap checked, the kept keys and lengths moved, the table rebuilt.
// Returns 0, or -100 with the index as it was
extern "C" int zkx_sim_compact(void *h, const uint32_t *remap_in, uint32_t n, int descending)
{
    ZkxSimIndex *x = (ZkxSimIndex *)h;
    if (n != x->m) return -100;
    if (n == 0) return 0;
    const bool desc = descending != 0;
    const auto remap = zkd_exact<uint32_t>(n), err = zkd_exact<uint32_t>(1, 0);
    const auto flags = zkd_exact<uint64_t>((size_t)n + 1), pos = zkd_exact<uint64_t>((size_t)n + 2);
    memcpy(remap.get(), remap_in, (size_t)n * 4);
    emu_set_lane_order(desc);
    zkd_flat(zkc_blocks((uint64_t)n + 1), desc, [&] { zk_k_cmp_remap_flags(remap.get(), n, flags.get()); });
    pos[0] = 0;
    for (uint32_t i = 0; i <= n; i++) pos[i + 1] = pos[i] + flags[i];
    zkd_flat(zkc_blocks(n), desc, [&] { zk_k_cmp_remap_check(remap.get(), n, pos.get(), err.get()); });
    int rc = err[0] ? -100 : 0;
    if (rc == 0) {
        const uint32_t nk = (uint32_t)pos[n];
        auto keys = zkd_exact<uint64_t>(nk);                                     // (exactly the kept frames: a place at or above n_kept is a report)
        auto lens = zkd_exact<uint32_t>(nk);
        zkd_flat(zkc_blocks(n), desc, [&] { zk_k_cmp_take(remap.get(), n, x->keys.get(), x->lens.get(), keys.get(), lens.get()); });
        x->keys = std::move(keys); x->lens = std::move(lens);
        x->m = nk;
        zkx_sim_rebuild(x, nk, desc);
    }
    emu_set_lane_order(false);
    return rc;
}

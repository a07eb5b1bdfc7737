// zk_view_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels of zk_read_view_ranges_dev (zeekstd_amd/csrc/zk_view.h, the very source hipcc compiles for gfx950) on the CPU under the
// emulator of hip_wg_emu.h, with the launchers' grids and the engine's pass loop (zk_view.hip): the plan functions of zk_view.h decide here what
// they decide in the engine.  The harness plays the decoder: every pass it fills a scratch of EXACTLY the pass's bytes with the frames' bytes by
// the plan's uids / uoff (0xEE for a frame that "fails"), and hands the kernels the frames' error codes.  tests/test_sim_view_ranges.py compares
// what the kernels leave -- every byte of the poisoned destination, the statuses, the return value, the frames decoded -- with the model of
// tests/helpers/view_model.py; tests/sim/view_san.cpp runs the same under AddressSanitizer + UBSan.  Every array a kernel sees is a heap
// allocation of exactly the entries zkv_sizes gives it, poisoned first; the destination starts `misalign` bytes into its allocation and ends
// with its last byte.
//   No kernel of zk_view.h has a barrier or a wave collective, so their lanes run one after the other (zkv_flat), in ascending or descending
// order of lanes AND workgroups.  zk_k_scan64 (zk_encode.hip) and zk_k_range_compact (zk_ranges.hip) are restated in plain C++.
#include "hip_wg_emu.h"
static inline unsigned long long emu_atomic_min(unsigned long long *p, unsigned long long v) { const unsigned long long old = *p; if (v < old) *p = v; return old; }
#include "../../zeekstd_amd/csrc/zk_view.h"
#include <memory>

template <class T> static std::unique_ptr<T[]> zkv_exact(size_t n, int fill = 0xA5)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    memset(p.get(), fill, (n ? n : 1) * sizeof(T));
    return p;
}
static void zkv_flat(uint32_t grid, bool descending, const std::function<void()> &body)
{
    EmuWG &g = g_emu;
    g.lanes.assign(ZKV_THREADS, EmuLane());
    g.grid_x = grid; g.grid_y = 1; g.block_y = 0;
    for (uint32_t bi = 0; bi < grid; bi++) {
        g.block = descending ? grid - 1 - bi : bi;
        for (uint32_t i = 0; i < ZKV_THREADS; i++) {
            const uint32_t t = descending ? ZKV_THREADS - 1 - i : i;
            g.lanes[t].tid = t; g.cur = t;
            body();
        }
    }
    g.block = 0; g.grid_x = 1;
}
// zk_k_scan64: the exclusive scan of n values, the total behind it
static void zkv_scan64(const uint64_t *in, uint32_t n, uint64_t *out)
{
    uint64_t s = 0;
    for (uint32_t i = 0; i < n; i++) { out[i] = s; s += in[i]; }
    out[n] = s;
}
// zk_k_range_compact: the frames whose coverage is not 0 and that are not empty, ascending; slot[f] for every f < n; uoff, words[0..1]
static void zkv_range_compact(const uint64_t *d_off, uint32_t n, const uint32_t *cover, uint32_t *slot, uint32_t *ids, uint64_t *uoff, uint64_t *words)
{
    uint32_t cv = 0, s = 0;
    uint64_t b = 0;
    for (uint32_t f = 0; f < n; f++) {
        cv += cover[f];
        slot[f] = s;
        const uint64_t sz = d_off[f + 1] - d_off[f];
        if (cv != 0 && sz != 0) { ids[s] = f; uoff[s] = b; s++; b += sz; }
    }
    uoff[s] = b; words[0] = s; words[1] = b;
}

// the plan functions, for literal expectations
extern "C" uint64_t zkv_sim_chunks(uint64_t len, uint64_t dst) { return zkv_chunks(len, (uintptr_t)dst); }
extern "C" uint64_t zkv_sim_chunk_begin(uint64_t k, uint64_t dst) { return zkv_chunk_begin(k, (uintptr_t)dst); }
extern "C" uint64_t zkv_sim_chunk_end(uint64_t k, uint64_t dst, uint64_t len) { return zkv_chunk_end(k, (uintptr_t)dst, len); }
extern "C" int32_t zkv_sim_check(uint64_t v0, uint64_t vend, uint64_t off, uint64_t len, uint64_t dst_cap, uint64_t dst_off) { return zkv_check(v0, vend, off, len, dst_cap, dst_off); }
extern "C" uint32_t zkv_sim_chunk_wgs(uint32_t count, uint64_t dst_cap) { return zkv_chunk_wgs(count, dst_cap); }

// "zk_read_view_ranges_dev".  data: the frames' decoded bytes back to back by d_off (d_off[0] == 0); dst_io[size]: the destination, poisoned by
// the caller, dst_cap <= size; misalign: where the destination starts in its allocation (mod 16 is what matters); pass_bytes: what
// ZK_CHOICE_RANGE_PASS_MIB gives (0 = 1 GiB); frame_err[n_frames]: ZSTD_ErrorCode of a frame that fails; status_io[count].
// out2: [0] frames decoded, [1] passes.  Returns the call's return value (-2003: the view was refused, dst_io and status_io untouched);
// -5: a kernel wrote where it must not
extern "C" int zk_view_sim(const uint8_t *data, const uint64_t *d_off_in, uint32_t n_frames, const uint32_t *ids_in, const uint64_t *voff_in, uint32_t vcount,
                           const uint64_t *offs_in, const uint64_t *lens_in, const uint64_t *dst_off_in, uint32_t count, uint8_t *dst_io, uint64_t dst_cap, uint64_t size,
                           uint32_t misalign, uint64_t pass_bytes_max, const int32_t *frame_err, int descending, int32_t *status_io, uint64_t *out2)
{
    out2[0] = 0; out2[1] = 0;
    if (count == 0) return 0;
    const bool desc = descending != 0;
    const ZkViewSizes S = zkv_sizes(count, vcount, n_frames);
    const auto d_off = zkv_exact<uint64_t>((size_t)n_frames + 1), voff = zkv_exact<uint64_t>((size_t)vcount + 1);
    const auto ids = zkv_exact<uint32_t>(vcount);
    const auto offs = zkv_exact<uint64_t>(count), lens = zkv_exact<uint64_t>(count), given = zkv_exact<uint64_t>(count);
    memcpy(d_off.get(), d_off_in, ((size_t)n_frames + 1) * 8);
    memcpy(voff.get(), voff_in, ((size_t)vcount + 1) * 8);
    if (vcount) memcpy(ids.get(), ids_in, (size_t)vcount * 4);
    memcpy(offs.get(), offs_in, (size_t)count * 8);
    memcpy(lens.get(), lens_in, (size_t)count * 8);
    if (dst_off_in) memcpy(given.get(), dst_off_in, (size_t)count * 8);
    const auto block = zkv_exact<uint8_t>((size_t)size + misalign, 0xEE);
    uint8_t *dst = block.get() + misalign;
    memcpy(dst, dst_io, (size_t)size);
    const auto eff = zkv_exact<uint64_t>(S.eff), cnt = zkv_exact<uint64_t>(S.cnt), packed = zkv_exact<uint64_t>(S.packed), coff = zkv_exact<uint64_t>(S.coff);
    const auto efirst = zkv_exact<uint32_t>(S.efirst), elast = zkv_exact<uint32_t>(S.elast);
    const auto status = zkv_exact<int32_t>(S.status), fstat = zkv_exact<int32_t>(S.fstat);
    const auto ecover = zkv_exact<uint32_t>(S.ecover, 0), seg = zkv_exact<uint32_t>(S.seg, 0), super = zkv_exact<uint32_t>(S.super, 0), fcover = zkv_exact<uint32_t>(S.fcover, 0);
    const auto ebase = zkv_exact<uint32_t>(S.ebase), slot = zkv_exact<uint32_t>(S.slot), uids = zkv_exact<uint32_t>(S.uids);
    const auto uoff = zkv_exact<uint64_t>(S.uoff), words = zkv_exact<uint64_t>(ZKV_W_WORDS);
    const auto out_status = zkv_exact<int32_t>(count);
    memcpy(out_status.get(), status_io, (size_t)count * 4);
    words[ZKV_W_VIEW_ERR] = 0; words[ZKV_W_FIRST_ERR] = ~0ull;
    uint32_t *err = (uint32_t *)(words.get() + ZKV_W_VIEW_ERR);
    const uint64_t *dst_off = dst_off_in ? given.get() : packed.get();

    emu_set_lane_order(desc);
    // launch_view_plan
    if (vcount) zkv_flat(zkv_blocks(vcount), desc, [&] { zk_k_view_check(d_off.get(), n_frames, ids.get(), voff.get(), vcount, err); });
    if (!dst_off_in) {
        zkv_flat(zkv_blocks(count), desc, [&] { zk_k_view_lens(voff.get(), vcount, offs.get(), lens.get(), count, eff.get()); });
        zkv_scan64(eff.get(), count, packed.get());
    }
    zkv_flat(zkv_blocks(count), desc, [&] {
        zk_k_view_plan(voff.get(), vcount, offs.get(), lens.get(), dst_off, count, dst_cap, (uintptr_t)dst, efirst.get(), elast.get(), status.get(), ecover.get(), seg.get(),
                       super.get(), cnt.get());
    });
    zkv_scan64(cnt.get(), count, coff.get());
    const uint32_t nseg = zkv_nseg(vcount);
    zkv_flat(zkv_blocks(nseg), desc, [&] { zk_k_view_bases(seg.get(), super.get(), nseg, ebase.get()); });
    if (vcount) zkv_flat(zkv_blocks(vcount), desc, [&] { zk_k_view_mark(ids.get(), voff.get(), vcount, ecover.get(), ebase.get(), err, fcover.get()); });
    zkv_range_compact(d_off.get(), n_frames, fcover.get(), slot.get(), uids.get(), uoff.get(), words.get());
    int rc = 0;
    if (words[ZKV_W_VIEW_ERR] != 0) rc = -2003;
    else {
        const uint32_t nt = (uint32_t)words[ZKV_W_FRAMES];
        const uint64_t bytes = words[ZKV_W_BYTES];
        const uint64_t cap = pass_bytes_max ? pass_bytes_max : 1ull << 30;
        bool any_failed = false;
        const uint32_t small_wgs = zkv_small_wgs(count), grid = small_wgs + zkv_chunk_wgs(count, dst_cap);
        for (uint32_t a = 0; a < nt;) {
            uint32_t b = nt;
            uint64_t pass_bytes = bytes;
            if (a != 0 || bytes > cap) {
                b = a + 1;
                while (b < nt && uoff[b + 1] - uoff[a] <= cap) b++;
                pass_bytes = uoff[b] - uoff[a];
            }
            // "zk_decode_enqueue": frames uids[a .. b) at scratch + uoff[s] - uoff[a], their codes in fstat[s]
            const auto scratch = zkv_exact<uint8_t>((size_t)pass_bytes, 0xEE);
            for (uint32_t s = a; s < b; s++) {
                const uint32_t f = uids[s];
                fstat[s] = frame_err ? frame_err[f] : 0;
                if (fstat[s]) any_failed = true;
                else memcpy(scratch.get() + (uoff[s] - uoff[a]), data + d_off[f], (size_t)(d_off[f + 1] - d_off[f]));
            }
            zkv_flat(grid, desc, [&] {
                zk_k_view_gather(scratch.get(), dst, ids.get(), voff.get(), vcount, offs.get(), lens.get(), dst_off, efirst.get(), coff.get(), count, slot.get(), uoff.get(),
                                 a, b, small_wgs);
            });
            out2[0] += b - a; out2[1]++;
            a = b;
        }
        zkv_flat(zkv_blocks(count), desc, [&] {
            zk_k_view_status(ids.get(), voff.get(), count, efirst.get(), elast.get(), slot.get(), fstat.get(), any_failed ? 1 : 0, nullptr, status.get(), out_status.get(),
                             (unsigned long long *)(words.get() + ZKV_W_FIRST_ERR));
        });
        if (words[ZKV_W_FIRST_ERR] != ~0ull) rc = -(int)(uint32_t)(words[ZKV_W_FIRST_ERR] & 0xFFFFFFFFu);
    }
    emu_set_lane_order(false);
    for (uint32_t m = 0; m < misalign; m++) if (block[m] != 0xEE) rc = -5;
    memcpy(dst_io, dst, (size_t)size);
    memcpy(status_io, out_status.get(), (size_t)count * 4);
    return rc;
}

// zk_dedup_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels that find duplicate frames (zeekstd_amd/csrc/zk_dedup.h, the very source hipcc compiles for gfx950) on the CPU under the
// emulator of hip_wg_emu.h, with the launchers' grids, the rounds and the scratch layout of zk_dedup_core, and the gather with the slices
// of zk_dedup_encode (zk_dedup.hip).  tests/test_sim_dedup.py compares what they leave -- ref, uniq, ids, the gathered bytes -- with the
// model of tests/helpers/dedup_model.py; tests/sim/dedup_san.cpp runs the same under AddressSanitizer + UBSan.  Every buffer a kernel sees
// is a heap allocation of EXACTLY the size the engine gives it, filled with a poison pattern first; the source is an exact copy that
// starts `misalign` bytes into its allocation and ends with it.
//   The frames' hashes are zk_k_dedup_hash's, or an INPUT: the map has to be right for any key function -- the tests also hand in hashes
// that collide on purpose.
//   No kernel of zk_dedup.h has a barrier or a wave collective -- a lane never waits for another -- so their lanes run one after the other
// without fibers (zkd_flat, over the emulator's threadIdx / blockIdx / gridDim and atomics), in ascending or descending order of lanes AND
// workgroups: the result must not depend on who reaches an atomic first.
#define ZKD_PEEK(p) (*(const volatile uint32_t *)(p))
#include "hip_wg_emu.h"
#include "../../zeekstd_amd/csrc/zk_dedup.h"
#include <memory>

template <class T> static std::unique_ptr<T[]> zkd_exact(size_t n, int fill = 0xA5)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    memset(p.get(), fill, (n ? n : 1) * sizeof(T));
    return p;
}
static void zkd_flat(uint32_t grid, bool descending, const std::function<void()> &body, uint32_t grid_y = 1)
{
    EmuWG &g = g_emu;
    g.lanes.assign(ZKD_THREADS, EmuLane());
    g.grid_x = grid; g.grid_y = grid_y;
    for (uint64_t bi = 0; bi < (uint64_t)grid * grid_y; bi++) {
        const uint64_t b = descending ? (uint64_t)grid * grid_y - 1 - bi : bi;
        g.block = (uint32_t)(b % grid); g.block_y = (uint32_t)(b / grid);
        for (uint32_t i = 0; i < ZKD_THREADS; i++) {
            const uint32_t t = descending ? ZKD_THREADS - 1 - i : i;
            g.lanes[t].tid = t; g.cur = t;
            body();
        }
    }
}

// src_in[nbytes]: the bytes off_in[0] .. off_in[count] name (count > 0, the list checked by the caller); hash_in[count], or null: the kernel's.  key_bits: what
// ZK_CHOICE_DEDUP_KEY_BITS gives.  Outputs: ref / ids (count), uniq (count; n_unique written), *rounds_out.  gather_out (may be null): the
// unique frames back to back, gathered in slices of slice_bytes (0 = 1 GiB), *gather_slices_out how many.  hash_out (may be null): the hashes used.
// Returns 0; -2: a round settled nothing; -4: the layout is not what the harness allocates; -5: a kernel wrote behind its output
extern "C" int zk_dedup_sim(const uint8_t *src_in, uint64_t nbytes, uint32_t misalign, const uint64_t *off_in, uint32_t count, const uint64_t *hash_in,
                            uint32_t key_bits, int descending, uint32_t *ref_out, uint32_t *uniq_out, uint32_t *ids_out, uint32_t *n_unique_out,
                            uint32_t *rounds_out, uint8_t *gather_out, uint64_t slice_bytes, uint32_t *gather_slices_out, uint64_t *hash_out)
{
    if (count == 0 || off_in[count] - off_in[0] != nbytes) return -1;
    const auto block = zkd_exact<uint8_t>((size_t)nbytes + misalign, 0xEE);
    uint8_t *src = block.get() + misalign;
    if (nbytes) memcpy(src, src_in, (size_t)nbytes);
    const ZkDedupLayout L = zkd_layout(count);
    const size_t q = ((size_t)4 * count + 15) & ~(size_t)15;
    if (L.flags - L.hash != (size_t)8 * count || L.pos - L.flags != (size_t)8 * (count + 1) || L.ref - L.pos < (size_t)8 * (count + 2) || L.slot - L.ref != q ||
        L.cnt - L.ids != q || L.table - L.cnt != 4 * ZKD_CNT_WORDS || L.end - L.table != (size_t)4 * zkd_slots(count)) return -4;
    const auto off = zkd_exact<uint64_t>((size_t)count + 1), hash = zkd_exact<uint64_t>(count), flags = zkd_exact<uint64_t>((size_t)count + 1), pos = zkd_exact<uint64_t>((size_t)count + 2);
    const auto ref = zkd_exact<uint32_t>(count), slot = zkd_exact<uint32_t>(count), list0 = zkd_exact<uint32_t>(count), list1 = zkd_exact<uint32_t>(count);
    const auto longl = zkd_exact<uint32_t>(count), differ = zkd_exact<uint32_t>(count), uniq = zkd_exact<uint32_t>(count), ids = zkd_exact<uint32_t>(count);
    const auto cnt = zkd_exact<uint32_t>(ZKD_CNT_WORDS), table = zkd_exact<uint32_t>(zkd_slots(count));
    memcpy(off.get(), off_in, ((size_t)count + 1) * 8);
    uint64_t max_frame = 0;
    for (uint32_t i = 0; i < count; i++) if (off[i + 1] - off[i] > max_frame) max_frame = off[i + 1] - off[i];
    const bool desc = descending != 0;
    emu_set_lane_order(desc);
    if (hash_in) memcpy(hash.get(), hash_in, (size_t)count * 8);
    else {
        // "hipMemsetAsync(S.hash, 0, count * 8)", "dim3(count < ZKD_GRID_MAX ? count : ZKD_GRID_MAX, zkd_pieces(max_frame))"
        memset(hash.get(), 0, (size_t)count * 8);
        zkd_flat(count < ZKD_GRID_MAX ? count : ZKD_GRID_MAX, desc, [&] { zk_k_dedup_hash(src, off.get(), off[0], count, (uint32_t *)hash.get()); }, zkd_pieces(max_frame));
    }
    // "hipMemsetAsync(S.ref, 0xFF, count * 4)"
    memset(ref.get(), 0xFF, (size_t)count * 4);
    const ZkDedupIn in{src, off.get(), off[0], hash.get(), key_bits};
    const uint32_t *list = nullptr;
    uint32_t *lists[2] = {list0.get(), list1.get()};
    uint32_t nopen = count, w = 0, rounds = 0;
    int rc = 0;
    while (nopen) {
        const uint32_t slots = zkd_slots(nopen), blocks = zkd_blocks(nopen);
        const ZkDedupRound r{list, nopen, slots - 1};
        uint32_t *next = lists[w];
        memset(table.get(), 0xFF, (size_t)slots * 4);
        memset(cnt.get(), 0, ZKD_CNT_WORDS * 4);
        zkd_flat(blocks, desc, [&] { zk_k_dedup_insert(in, r, table.get(), slot.get()); });
        zkd_flat(blocks, desc, [&] { zk_k_dedup_verify(in, r, table.get(), slot.get(), ref.get(), next, longl.get(), differ.get(), cnt.get()); });
        if (const uint32_t nlong = cnt[ZKD_CNT_LONG]) {
            // "dim3 grid(nlong < ZKD_GRID_MAX ? nlong : ZKD_GRID_MAX, zkd_pieces(max_frame))"
            const uint32_t gx = nlong < ZKD_GRID_MAX ? nlong : ZKD_GRID_MAX, gy = zkd_pieces(max_frame);
            zkd_flat(gx, desc, [&] { zk_k_dedup_verify_long(in, table.get(), slot.get(), longl.get(), nlong, differ.get()); }, gy);
            zkd_flat(zkd_blocks(nlong), desc, [&] { zk_k_dedup_settle_long(table.get(), slot.get(), longl.get(), nlong, differ.get(), ref.get(), next, cnt.get()); });
        }
        rounds++;
        if (cnt[ZKD_CNT_NEXT] >= nopen) { rc = -2; break; }
        nopen = cnt[ZKD_CNT_NEXT]; list = next; w ^= 1;
    }
    uint32_t nu = 0;
    if (rc == 0) {
        zkd_flat(zkd_blocks((uint64_t)count + 1), desc, [&] { zk_k_dedup_flags(ref.get(), count, flags.get()); });
        // zk_k_scan64 (zk_encode.hip), restated: the exclusive scan of count + 1 values, the total behind it
        pos[0] = 0;
        for (uint32_t i = 0; i <= count; i++) pos[i + 1] = pos[i] + flags[i];
        zkd_flat(zkd_blocks(count), desc, [&] { zk_k_dedup_emit(ref.get(), count, pos.get(), uniq.get(), ids.get()); });
        nu = (uint32_t)pos[count];
        for (uint32_t k = nu; k < count; k++) if (uniq[k] != 0xA5A5A5A5u) rc = -5;
    }
    uint32_t nslices = 0;
    if (rc == 0 && gather_out) {
        // zk_dedup_encode: the slices, each gathered into a buffer of exactly its bytes
        const uint64_t slice_max = slice_bytes ? slice_bytes : 1ull << 30;
        const auto len_of = [&](uint32_t k) { return off[uniq[k] + 1] - off[uniq[k]]; };
        uint64_t done = 0;
        for (uint32_t k0 = 0; k0 < nu; nslices++) {
            const uint32_t k1 = zkd_slice_end(k0, nu, slice_max, len_of), m = k1 - k0;
            const auto goff = zkd_exact<uint64_t>((size_t)m + 1);
            goff[0] = 0;
            for (uint32_t k = 0; k < m; k++) goff[k + 1] = goff[k] + len_of(k0 + k);
            const auto dst = zkd_exact<uint8_t>((size_t)goff[m]);
            const uint32_t gx = m < ZKD_GRID_MAX ? m : ZKD_GRID_MAX, gy = zkd_pieces(max_frame);
            zkd_flat(gx, desc, [&] { zk_k_dedup_gather(src, off.get(), off[0], uniq.get() + k0, m, goff.get(), dst.get()); }, gy);
            memcpy(gather_out + done, dst.get(), (size_t)goff[m]);
            done += goff[m];
            k0 = k1;
        }
    }
    emu_set_lane_order(false);
    if (hash_out) memcpy(hash_out, hash.get(), (size_t)count * 8);
    memcpy(ref_out, ref.get(), (size_t)count * 4);
    memcpy(ids_out, ids.get(), (size_t)count * 4);
    memcpy(uniq_out, uniq.get(), (size_t)count * 4);
    *n_unique_out = nu;
    *rounds_out = rounds;
    if (gather_slices_out) *gather_slices_out = nslices;
    return rc;
}

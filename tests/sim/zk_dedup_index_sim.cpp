// zk_dedup_index_sim.cpp -- TEST HARNESS (never shipped, never linked into libzeekstd_amd.so).
// Runs the kernels of the dedup index (zeekstd_amd/csrc/zk_dedup_index.h, the very source hipcc compiles for gfx950) on the CPU under the
// emulator of hip_wg_emu.h, with the launchers' grids, the rounds, the passes and the scratch layout of zk_dedup_index.hip, behind the
// in-call map of zk_dedup_sim.cpp.  The harness hands over the candidates' decoded bytes in place of the decode: every pass gets a heap
// allocation of EXACTLY its bytes, the archive frames of its pairs copied to their places.  Every other buffer a kernel sees is exact too,
// and poisoned first.  tests/test_sim_dedup_index.py compares ids and fresh with the model of tests/helpers/dedup_against_model.py;
// tests/sim/dedup_index_san.cpp runs the same under AddressSanitizer + UBSan.
//   No kernel of zk_dedup_index.h has a barrier or a wave collective, so their lanes run one after the other (zkd_flat), in ascending or
// descending order of lanes AND workgroups.
#include "zk_dedup_sim.cpp"
#include "../../zeekstd_amd/csrc/zk_dedup_index.h"

// the index as zk_dedup_index.hip keeps it: keys / lens of exactly m entries, a table of exactly `slots` words
struct ZkxSimIndex {
    uint32_t bits = 0, m = 0, slots = 0;
    std::unique_ptr<uint64_t[]> keys;
    std::unique_ptr<uint32_t[]> lens, table;
};
// "zkx_rebuild"
static void zkx_sim_rebuild(ZkxSimIndex *x, uint32_t frames, bool desc)
{
    x->slots = zkx_slots(frames);
    x->table = zkd_exact<uint32_t>(x->slots, 0xFF);
    if (frames) zkd_flat(zkd_blocks(frames), desc, [&] { zk_k_dxi_insert(x->keys.get(), x->lens.get(), x->bits, 0u, frames, x->table.get(), x->slots - 1); });
}
// "zkx_reserve" (exact: room for total frames, the first m kept) -- the keys / lens of the n new frames are written by the caller -- then "zkx_commit"
static void zkx_sim_room(ZkxSimIndex *x, uint32_t total)
{
    auto keys = zkd_exact<uint64_t>(total);
    auto lens = zkd_exact<uint32_t>(total);
    if (x->m) { memcpy(keys.get(), x->keys.get(), (size_t)x->m * 8); memcpy(lens.get(), x->lens.get(), (size_t)x->m * 4); }
    x->keys = std::move(keys); x->lens = std::move(lens);
}
static void zkx_sim_commit(ZkxSimIndex *x, uint32_t n, bool desc)
{
    const uint32_t total = x->m + n;
    if (zkx_slots(total) > x->slots) zkx_sim_rebuild(x, total, desc);
    else if (n) zkd_flat(zkd_blocks(n), desc, [&] { zk_k_dxi_insert(x->keys.get(), x->lens.get(), x->bits, x->m, n, x->table.get(), x->slots - 1); });
    x->m = total;
}

extern "C" void *zkx_sim_create(uint32_t bits)
{
    ZkxSimIndex *x = new ZkxSimIndex();
    x->bits = bits;
    zkx_sim_room(x, 0);
    zkx_sim_rebuild(x, 0, false);
    return x;
}
extern "C" void zkx_sim_free(void *h) { delete (ZkxSimIndex *)h; }
extern "C" uint32_t zkx_sim_count(void *h) { return ((ZkxSimIndex *)h)->m; }
extern "C" uint32_t zkx_sim_slots(void *h) { return ((ZkxSimIndex *)h)->slots; }
extern "C" int zkx_sim_add(void *h, const uint64_t *keys, const uint32_t *lens, uint32_t n, int descending)
{
    ZkxSimIndex *x = (ZkxSimIndex *)h;
    emu_set_lane_order(descending != 0);
    zkx_sim_room(x, x->m + n);
    if (n) { memcpy(x->keys.get() + x->m, keys, (size_t)n * 8); memcpy(x->lens.get() + x->m, lens, (size_t)n * 4); }
    zkx_sim_commit(x, n, descending != 0);
    emu_set_lane_order(false);
    return 0;
}
extern "C" int zkx_sim_truncate(void *h, uint32_t count, int descending)
{
    ZkxSimIndex *x = (ZkxSimIndex *)h;
    if (count > x->m) return -1;
    emu_set_lane_order(descending != 0);
    x->m = count;
    zkx_sim_room(x, count);
    zkx_sim_rebuild(x, count, descending != 0);
    emu_set_lane_order(false);
    return 0;
}
extern "C" int zkx_sim_export(void *h, uint32_t first, uint32_t count, uint64_t *keys_out, uint32_t *lens_out)
{
    ZkxSimIndex *x = (ZkxSimIndex *)h;
    if ((uint64_t)first + count > x->m) return -1;
    memcpy(keys_out, x->keys.get() + first, (size_t)count * 8);
    memcpy(lens_out, x->lens.get() + first, (size_t)count * 4);
    return 0;
}
// every frame's slot: the table holds each id < m exactly once and nothing else
extern "C" int zkx_sim_table_ok(void *h)
{
    ZkxSimIndex *x = (ZkxSimIndex *)h;
    if (x->slots < 64 || (x->slots & (x->slots - 1)) || x->slots < 2ull * x->m) return 0;
    std::vector<uint32_t> seen(x->m, 0);
    for (uint32_t s = 0; s < x->slots; s++) {
        const uint32_t id = x->table[s];
        if (id == ZKD_EMPTY) continue;
        if (id >= x->m || seen[id]++) return 0;
    }
    for (uint32_t id = 0; id < x->m; id++) if (!seen[id]) return 0;
    return 1;
}

// The list (as zk_dedup_sim takes it) against the archive: arch[arch_off[s] .. arch_off[s + 1]) the DECODED bytes of archive frame s < n_frames
// (n_frames >= the index's m).  hash_in: the list frames' hashes in zk_k_dedup_hash's place, or null.  key_bits: the in-call map's.  pass_bytes:
// what ZK_CHOICE_DEDUP_PASS_KIB gives (0 = 1 GiB).  take != 0: the fresh frames' keys and lengths are added to the index behind the map, as
// zk_encode_dedup_against_dev does.  Outputs: ids (count), fresh (count; n_fresh written), the rounds, the passes, the largest pass in bytes.
// Returns 0; -1 arguments; -3 the layout is not what the harness allocates; -5 a kernel wrote behind its output; -6 a round made no way;
// otherwise zk_dedup_sim's code
extern "C" int zkx_sim_against(void *h, const uint8_t *arch, const uint64_t *arch_off_in, uint32_t n_frames, const uint8_t *src_in, uint64_t nbytes, uint32_t misalign,
                               const uint64_t *off_in, uint32_t count, const uint64_t *hash_in, uint32_t key_bits, int descending, uint64_t pass_bytes, int take,
                               uint32_t *ids_out, uint32_t *fresh_out, uint32_t *n_fresh_out, uint32_t *rounds_out, uint32_t *passes_out, uint64_t *largest_pass_out)
{
    ZkxSimIndex *x = (ZkxSimIndex *)h;
    if (count == 0 || n_frames < x->m) return -1;
    // the in-call map: "zk_dedup_map_dev"
    std::vector<uint32_t> ref(count), uniq(count), ids_in(count);
    std::vector<uint64_t> hash(count);
    uint32_t nu = 0, in_rounds = 0;
    if (const int rc = zk_dedup_sim(src_in, nbytes, misalign, off_in, count, hash_in, key_bits, descending, ref.data(), uniq.data(), ids_in.data(), &nu, &in_rounds, nullptr, 0,
                                    nullptr, hash.data())) return rc;
    const auto block = zkd_exact<uint8_t>((size_t)nbytes + misalign, 0xEE);
    uint8_t *src = block.get() + misalign;
    if (nbytes) memcpy(src, src_in, (size_t)nbytes);
    const ZkDxLayout L = zkx_layout(count);
    const size_t q = ((size_t)4 * count + 15) & ~(size_t)15;
    if (L.pos - L.flags != (size_t)8 * (count + 1) || L.poff - L.pos != (size_t)8 * (count + 2) || L.cand - L.poff < (size_t)8 * (2 * (size_t)count + 2) || L.out - L.cand != q ||
        L.cs - L.fresh != q || L.end - L.ds != q) return -3;
    const auto off = zkd_exact<uint64_t>((size_t)count + 1), arch_off = zkd_exact<uint64_t>((size_t)n_frames + 1), d_hash = zkd_exact<uint64_t>(count);
    const auto d_uniq = zkd_exact<uint32_t>(nu), d_ids_in = zkd_exact<uint32_t>(count);
    const auto flags = zkd_exact<uint64_t>((size_t)count + 1), pos = zkd_exact<uint64_t>((size_t)count + 2), d_poff = zkd_exact<uint64_t>(2 * (size_t)count + 2);
    const auto cand = zkd_exact<uint32_t>(count), out = zkd_exact<uint32_t>(count), list = zkd_exact<uint32_t>(count), d_pid = zkd_exact<uint32_t>(count);
    const auto d_pk = zkd_exact<uint32_t>(count), differ = zkd_exact<uint32_t>(count), ids = zkd_exact<uint32_t>(count), fresh = zkd_exact<uint32_t>(count);
    memcpy(off.get(), off_in, ((size_t)count + 1) * 8);
    memcpy(arch_off.get(), arch_off_in, ((size_t)n_frames + 1) * 8);
    memcpy(d_hash.get(), hash.data(), (size_t)count * 8);
    memcpy(d_uniq.get(), uniq.data(), (size_t)nu * 4);
    memcpy(d_ids_in.get(), ids_in.data(), (size_t)count * 4);
    uint64_t max_frame = 0;
    for (uint32_t i = 0; i < count; i++) if (off[i + 1] - off[i] > max_frame) max_frame = off[i + 1] - off[i];
    const bool desc = descending != 0;
    emu_set_lane_order(desc);
    const ZkDxIndex xi{x->keys.get(), x->lens.get(), x->table.get(), x->m, x->slots - 1, x->bits};
    const uint64_t pass_max = pass_bytes ? pass_bytes : ZKX_PASS_BYTES;
    // "hipMemsetAsync(D.cand, 0xFF, nu * 4)"
    memset(cand.get(), 0xFF, (size_t)nu * 4);
    std::vector<uint32_t> open, next, pid, pk;
    std::vector<uint64_t> poff;
    uint32_t nopen = nu, rounds = 0, passes = 0;
    uint64_t largest = 0;
    int rc = 0;
    for (uint32_t round = 0; nopen && rc == 0; round++) {
        if (round) memcpy(list.get(), open.data(), (size_t)nopen * 4);
        zkd_flat(zkd_blocks(nopen), desc, [&] { zk_k_dxi_lookup(xi, arch_off.get(), d_hash.get(), off.get(), d_uniq.get(), round ? list.get() : nullptr, nopen, cand.get(), out.get()); });
        rounds++;
        pid.clear(); pk.clear();
        for (uint32_t t = 0; t < nopen; t++) {
            const uint32_t k = round ? open[t] : t;
            if (out[t] == ZKX_FRESH || off[uniq[k] + 1] == off[uniq[k]]) continue;
            if (out[t] >= x->m) { rc = -6; break; }
            pid.push_back(out[t]); pk.push_back(k);
        }
        const uint32_t np = (uint32_t)pid.size();
        if (!np || rc) break;
        const auto len_of = [&](uint32_t p) { return off[uniq[pk[p]] + 1] - off[uniq[pk[p]]]; };
        std::vector<uint32_t> cut{0};
        poff.clear();
        while (cut.back() < np) {
            const uint32_t p0 = cut.back(), p1 = zkx_pass_end(p0, np, pass_max, len_of);
            uint64_t at = 0;
            for (uint32_t p = p0; p < p1; p++) { poff.push_back(at); at += len_of(p); }
            poff.push_back(at);
            cut.push_back(p1);
        }
        if (poff.size() > 2 * (size_t)count + 2) { rc = -3; break; }
        memcpy(d_pid.get(), pid.data(), (size_t)np * 4);
        memcpy(d_pk.get(), pk.data(), (size_t)np * 4);
        memcpy(d_poff.get(), poff.data(), poff.size() * 8);
        memset(differ.get(), 0, (size_t)np * 4);
        for (size_t s = 0; s + 1 < cut.size(); s++) {
            const uint32_t p0 = cut[s], n = cut[s + 1] - p0;
            const uint64_t *pass_off = d_poff.get() + p0 + s;
            const uint64_t bytes = poff[p0 + s + n];
            // in place of zk_decode_enqueue: the candidates' decoded bytes at their places, in an allocation of exactly the pass
            const auto dec = zkd_exact<uint8_t>((size_t)bytes, 0xDD);
            for (uint32_t p = 0; p < n; p++) {
                const uint32_t id = pid[p0 + p];
                if (arch_off[id + 1] - arch_off[id] != pass_off[p + 1] - pass_off[p]) { rc = -6; break; }
                memcpy(dec.get() + pass_off[p], arch + arch_off[id], (size_t)(arch_off[id + 1] - arch_off[id]));
            }
            if (rc) break;
            zkd_flat(n < ZKD_GRID_MAX ? n : ZKD_GRID_MAX, desc,
                     [&] { zk_k_dxi_compare(src, off.get(), off[0], d_uniq.get(), d_pk.get() + p0, pass_off, dec.get(), n, differ.get() + p0); }, zkd_pieces(max_frame));
            passes++;
            if (bytes > largest) largest = bytes;
        }
        next.clear();
        for (uint32_t p = 0; p < np; p++) if (differ[p]) next.push_back(pk[p]);
        open.swap(next);
        nopen = (uint32_t)open.size();
        if (rounds > x->m + 1) rc = -6;
    }
    uint32_t nf = 0;
    if (rc == 0) {
        zkd_flat(zkd_blocks((uint64_t)nu + 1), desc, [&] { zk_k_dxi_flags(cand.get(), nu, flags.get()); });
        pos[0] = 0;
        for (uint32_t k = 0; k <= nu; k++) pos[k + 1] = pos[k] + flags[k];
        zkd_flat(zkd_blocks(count), desc, [&] { zk_k_dxi_emit(d_ids_in.get(), d_uniq.get(), cand.get(), pos.get(), count, nu, x->m, ids.get(), fresh.get()); });
        nf = (uint32_t)pos[nu];
        for (uint32_t k = nf; k < count; k++) if (fresh[k] != 0xA5A5A5A5u) rc = -5;
    }
    if (rc == 0 && take) {
        // "zkx_reserve", zk_k_dxi_take, "zkx_commit"
        zkx_sim_room(x, x->m + nf);
        if (nf) zkd_flat(zkd_blocks(nf), desc, [&] { zk_k_dxi_take(d_hash.get(), off.get(), fresh.get(), nf, x->keys.get() + x->m, x->lens.get() + x->m); });
        zkx_sim_commit(x, nf, desc);
    }
    emu_set_lane_order(false);
    memcpy(ids_out, ids.get(), (size_t)count * 4);
    memcpy(fresh_out, fresh.get(), (size_t)count * 4);
    *n_fresh_out = nf;
    *rounds_out = rounds;
    *passes_out = passes;
    *largest_pass_out = largest;
    return rc;
}

// zk_dedup_index.h -- a frame list deduplicated against an archive that already exists: the kernels of zk_dedup_index_* and
// zk_dedup_against_dev / zk_encode_dedup_against_dev (included by zk_dedup_index.hip, which keeps their launchers; tests/sim/zk_dedup_index_sim.cpp
// runs the same source on the CPU under the workgroup emulator, against the model of tests/helpers/dedup_against_model.py).  It builds on
// zk_dedup.h: the frame key is zk_k_dedup_hash's 64 bits, cut by zkd_key, homed by zkd_home, compared by zkd_wg_differ.
// The rule (include/zeekstd_amd.h), for an archive of m frames:
//   ids[i]    the smallest archive frame s < m whose decoded bytes are frame i's, where one exists; otherwise m + the position in `fresh` of
//             the first list frame with frame i's bytes
//   fresh     those first list frames, ascending
// THE INDEX (lives from call to call, on the device): keys[m] the frames' full 64-bit hashes, lens[m] their lengths, and an open-addressing
// table of 32-bit archive ids.  Every frame has a slot of its own -- equal keys are not merged: the archive may hold duplicates --, taken by
// compare-and-swap on an empty slot, linear probing from zkd_home of the cut key.  The table has no key words: a slot's key is keys[id].  No
// slot is ever given back (truncate rebuilds), so all frames of one home lie in the run from the home to the first empty slot.
//   zk_k_dxi_insert     a lane per new frame: its id into the table
//   zk_k_dxi_take       keys / lens of the fresh frames of a call, from the hashes its in-call map made (zk_encode_dedup_against_dev)
//   zk_k_dxi_lens       lens from prefix sums (zk_dedup_index_add_archive_dev)
// THE LOOKUP, behind the in-call map of zk_dedup.h (ref, uniq, ids of the list alone), in ROUNDS over the unique frames still OPEN:
//   zk_k_dxi_lookup     a lane per open unique frame walks its probe chain to the first empty slot; among the slots whose cut key and length
//                       are the frame's (and whose archive entry has that length) it takes the smallest id above the one it tried last:
//                       its CANDIDATE.  None: the frame is FRESH
//   (the host makes the round's (frame, candidate) pairs and their places in the scratch; the candidates are decoded there, pass after pass)
//   zk_k_dxi_compare    a workgroup per pair and piece of ZKD_PIECE bytes: the decoded candidate against the source frame, zkd_wg_differ; no
//                       load leaves either frame.  A difference is an atomic OR into differ[pair]
//   equal: the frame is settled on its candidate.  Different: it is open again, with the candidate tried.  Candidates ascend, so the first
//   that is equal is the smallest.
//   zk_k_dxi_flags / (zk_k_scan64) / zk_k_dxi_emit      fresh, and ids for all frames of the list through the in-call ids
// Every write is a vector store or a vector atomic.  Plain C++ only: no barrier, and no lane waits for another.
#pragma once
#include "zk_dedup.h"

constexpr uint32_t ZKX_FRESH = 0xFFFFFFFEu;                 // cand[]: no archive frame (left) that could hold this content
constexpr uint64_t ZKX_PASS_BYTES = 1ull << 30;             // ZK_CHOICE_DEDUP_PASS_KIB's default

// slots for an index of `frames` frames: a power of two, at least twice as many and at least 64 (grown -- the table rebuilt from the keys --
// when an add would cross that)
ZK_HD uint32_t zkx_slots(uint32_t frames) { return zkd_slots(frames); }
// the pass that begins with the p0-th pair of a round ends before the returned one: whole candidates of at most pass_max decoded bytes in
// all, one at least.  len_of(p): the length of the p-th pair's frame
template <class LenOf> ZK_HD uint32_t zkx_pass_end(uint32_t p0, uint32_t np, uint64_t pass_max, LenOf len_of) { return zkd_slice_end(p0, np, pass_max, len_of); }
// The scratch of one call for `count` frames, in bytes from its start (the unique frames are at most count, a round's pairs at most as many,
// its passes at most as many as its pairs): flags[count + 1] | pos[count + 2] | poff[2 * count + 2] (the pairs' places, per pass from 0) |
// cand | out | list | pid | pk | differ | fstat | ids | fresh | cs | ds (count each; cs / ds: the fresh frames' sizes as the encoder leaves them,
// handed to the caller once the encode has succeeded)
struct ZkDxLayout { size_t flags, pos, poff, cand, out, list, pid, pk, differ, fstat, ids, fresh, cs, ds, end; };
ZK_HD ZkDxLayout zkx_layout(uint32_t count)
{
    ZkDxLayout L;
    const size_t c = count, q = (4 * c + 15) & ~(size_t)15;
    L.flags = 0;
    L.pos = L.flags + 8 * (c + 1);
    L.poff = L.pos + 8 * (c + 2);
    L.cand = (L.poff + 8 * (2 * c + 2) + 15) & ~(size_t)15;
    L.out = L.cand + q; L.list = L.out + q; L.pid = L.list + q; L.pk = L.pid + q; L.differ = L.pk + q; L.fstat = L.differ + q;
    L.ids = L.fstat + q; L.fresh = L.ids + q; L.cs = L.fresh + q; L.ds = L.cs + q; L.end = L.ds + q;
    return L;
}

// the index as the kernels see it: m frames, a table of mask + 1 slots, keys cut to `bits` bits
struct ZkDxIndex { const uint64_t *keys; const uint32_t *lens; const uint32_t *table; uint32_t m, mask, bits; };

// frames first .. first + n - 1 (their keys and lengths are in place) into the table
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_insert(const uint64_t *keys, const uint32_t *lens, uint32_t bits, uint32_t first, uint32_t n, uint32_t *table,
                                                               uint32_t mask)
{
    const uint32_t t = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (t >= n) return;
    const uint32_t id = first + t;
    uint32_t s = zkd_home(zkd_key(keys[id], lens[id], bits), mask);
    for (;;) {
        uint32_t old = ZKD_PEEK(table + s);
        if (old == ZKD_EMPTY) old = atomicCAS(table + s, ZKD_EMPTY, id);
        if (old == ZKD_EMPTY) break;                                             // taken (the table has more slots than frames: there is one)
        s = (s + 1) & mask;
    }
}

// keys_out[k] / lens_out[k]: of list frame fresh[k], k < n
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_take(const uint64_t *hash, const uint64_t *off, const uint32_t *fresh, uint32_t n, uint64_t *keys_out,
                                                             uint32_t *lens_out)
{
    const uint32_t k = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = fresh[k];
    keys_out[k] = hash[i];
    lens_out[k] = (uint32_t)(off[i + 1] - off[i]);
}
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_lens(const uint64_t *off, uint32_t n, uint32_t *lens_out)
{
    const uint32_t k = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (k < n) lens_out[k] = (uint32_t)(off[k + 1] - off[k]);
}

// The open unique frames: list[t] (list == nullptr: t), t < nopen, positions in uniq.  cand[k]: ZKD_EMPTY before the first round, the
// candidate tried last from then on; the new candidate (or ZKX_FRESH) goes there and to out[t].  arch_off: the archive's prefix sums of
// decoded sizes -- an index entry whose length is not the archive's is no candidate (its decoded frame would not lie where the pairs say)
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_lookup(ZkDxIndex x, const uint64_t *arch_off, const uint64_t *hash, const uint64_t *off, const uint32_t *uniq,
                                                               const uint32_t *list, uint32_t nopen, uint32_t *cand, uint32_t *out)
{
    const uint32_t t = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (t >= nopen) return;
    const uint32_t k = list ? list[t] : t, i = uniq[k], tried = cand[k];
    const uint64_t len = off[i + 1] - off[i], key = zkd_key(hash[i], len, x.bits);
    uint32_t best = ZKX_FRESH, s = zkd_home(key, x.mask);
    for (uint32_t n = 0; n <= x.mask; n++) {
        const uint32_t id = x.table[s];
        if (id == ZKD_EMPTY) break;
        if (id < x.m && id < best && (tried == ZKD_EMPTY || id > tried) && x.lens[id] == len && zkd_key(x.keys[id], len, x.bits) == key &&
            arch_off[id + 1] - arch_off[id] == len) best = id;
        s = (s + 1) & x.mask;
    }
    cand[k] = best;
    out[t] = best;
}

// Pair p < np of a pass: unique frame pk[p] against its decoded candidate at dec + poff[p] (poff[0] = 0).  Workgroup (p, y) takes the pieces
// y, y + gridDim.y, ... of the frame
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_compare(const uint8_t *src, const uint64_t *off, uint64_t base, const uint32_t *uniq, const uint32_t *pk,
                                                                const uint64_t *poff, const uint8_t *dec, uint32_t np, uint32_t *differ)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t i = uniq[pk[p]];
        const uint64_t len = off[i + 1] - off[i];
        const uint8_t *x = src + (off[i] - base), *y = dec + poff[p];
        bool d = false;
        for (uint64_t p0 = (uint64_t)blockIdx.y * ZKD_PIECE; p0 < len; p0 += (uint64_t)gridDim.y * ZKD_PIECE)
            d |= zkd_wg_differ(x + p0, y + p0, (uint32_t)(len - p0 < ZKD_PIECE ? len - p0 : ZKD_PIECE), tid);
        if (d) atomicOr(differ + p, 1u);
    }
}

// flags[k] = unique frame k is fresh; flags[nu] = 0, so that the scan of nu + 1 values leaves pos[nu] = n_fresh
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_flags(const uint32_t *cand, uint32_t nu, uint64_t *flags)
{
    const uint32_t k = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (k <= nu) flags[k] = k < nu && cand[k] == ZKX_FRESH;
}
// ids_in: the in-call ids (frame i has the bytes of unique frame ids_in[i]); pos: the exclusive scan of the flags.  ids_out / fresh_out may be null
__global__ __launch_bounds__(ZKD_THREADS) void zk_k_dxi_emit(const uint32_t *ids_in, const uint32_t *uniq, const uint32_t *cand, const uint64_t *pos, uint32_t count,
                                                             uint32_t nu, uint32_t m, uint32_t *ids_out, uint32_t *fresh_out)
{
    const uint32_t i = blockIdx.x * ZKD_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t k = ids_in[i], c = cand[k];
    if (ids_out) ids_out[i] = c == ZKX_FRESH ? m + (uint32_t)pos[k] : c;
    if (fresh_out && i < nu && cand[i] == ZKX_FRESH) fresh_out[pos[i]] = uniq[i];
}

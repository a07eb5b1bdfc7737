// zk_sim_dict.cpp -- TEST INFRASTRUCTURE: the decoder's lane code (zk_device.h) run on the CPU against a zstd dictionary, the way the
// kernels run it: frame walk with the dictionary's ID and block entry (zk_dict.h) -> Huffman literals -> sequence decode -> execution
// with the dictionary's content below the frame and its repeat offsets as the first history.  The block entry of the dictionary sits
// behind the batch's last block and its "content" behind the compressed bytes, in one buffer (the engine keeps it in a buffer of its
// own and states the distance).  The executor here is the plain byte loop: the tile machinery is tests/sim/zk_sim.cpp's subject.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../zeekstd_amd/csrc/zk_dict.h"

static const uint32_t LLV[36] = ZK_LL_TABLE;
static const uint32_t MLV[53] = ZK_ML_TABLE;

// dict / dict_len: the dictionary's bytes (nullptr: none).  status[count]: 0 or the ZSTD_ErrorCode of a frame.  Returns 0, or -30 for a
// dictionary zk_dict_parse refuses.
extern "C" int zk_sim_dict_decode(const uint8_t *comp_in, uint64_t comp_len, const uint64_t *c_off, const uint64_t *d_off, uint32_t count,
                                  const uint8_t *dict, uint64_t dict_len, uint8_t *dst, int32_t *status)
{
    ZkDictLayout L;
    if (zk_dict_parse(dict, dict ? dict_len : 0, L) != ZK_OK) return -(int)ZK_E_DICT_CORRUPTED;
    const bool have = dict && dict_len;
    std::vector<uint8_t> img;
    ZkBlock dblk;
    if (have && L.formatted) zk_dict_block(dict, L, img, dblk);
    else memset(&dblk, 0, sizeof dblk);
    std::vector<uint8_t> buf(comp_in, comp_in + comp_len);
    buf.resize((comp_len + 15) & ~(uint64_t)7, 0);
    const uint64_t img_at = buf.size();
    buf.insert(buf.end(), img.begin(), img.end());
    buf.resize(buf.size() + 16, 0);
    const uint8_t *comp = buf.data();
    const uint8_t *content = have ? dict + L.content_off : nullptr;
    const uint64_t plen = have ? dict_len - L.content_off : 0;

    std::vector<ZkFrameInfo> infos(count);
    std::vector<ZkFrameBase> bases(count);
    uint64_t nb = 0, ns = 0, nl = 0;
    const bool tables = have && L.formatted;
    ZkDictWalk dw; dw.on = have ? 1u : 0u; dw.id = L.id; dw.def = tables ? 0u : ZK_DEF_NONE;                 // (counting: "a table is in force", whichever)
    for (uint32_t f = 0; f < count; f++) {
        ZkFrameInfo fi;
        zk_walk_frame(comp, c_off[f], c_off[f + 1], d_off[f + 1] - d_off[f], f, nullptr, nullptr, fi, dw);
        if (fi.status != ZK_OK) { fi.n_blocks = 0; fi.n_seq = 0; fi.lit_bytes = 0; }
        infos[f] = fi;
        bases[f].block_base = nb; bases[f].seq_base = ns; bases[f].lit_base = nl;
        nb += fi.n_blocks; ns += fi.n_seq; nl += fi.lit_bytes;
    }
    if (tables) dw.def = (uint32_t)nb;                                 // the dictionary's block entry: behind the last block
    std::vector<ZkBlock> blocks(nb + 1);
    std::vector<ZkSeqP> seqs(ns + 1);
    std::vector<uint8_t> lit(nl + 64);
    if (tables) {
        dblk.src = img_at;
        dblk.huf_def = dblk.tab_def[0] = dblk.tab_def[1] = dblk.tab_def[2] = (uint32_t)nb;
        blocks[nb] = dblk;
    }
    for (uint32_t f = 0; f < count; f++) {
        if (infos[f].status != ZK_OK) continue;
        ZkFrameInfo fi;
        zk_walk_frame(comp, c_off[f], c_off[f + 1], d_off[f + 1] - d_off[f], f, &bases[f], blocks.data(), fi, dw);
    }
    // literals: zk_k_huf's steps, a stream at a time
    std::vector<uint16_t> tab(2048);
    for (uint64_t bi = 0; bi < nb; bi++) {
        ZkBlock &b = blocks[bi];
        if (!(b.type == 2 && b.lit_type >= 2 && b.status == ZK_OK)) continue;
        const ZkBlock &def = blocks[b.huf_def];
        ZkHufHdr hd; ZkHufTmp tmp;
        uint32_t mb = 0, nsym = 0;
        const uint32_t r = zk_huf_read_weights(comp + def.src + def.lit_off, def.lit_comp, &hd, &tmp, &nsym, &mb);
        bool ok = r != 0;
        if (ok) {
            zk_huf_fill_table(tab.data(), &hd, nsym, mb);
            const uint8_t *pay = comp + b.src + b.lit_off;
            uint32_t size = b.lit_comp;
            if (b.lit_type == 2) { pay += r; size -= r; }
            uint8_t *d = lit.data() + b.lit_base;
            const uint32_t regen = b.lit_regen;
            if (b.lit_streams == 1) ok = zk_huf_decode_stream(tab.data(), mb, pay, size, d, regen);
            else if (size < 6) ok = false;
            else {
                const uint32_t s1 = zk_rd16(pay), s2 = zk_rd16(pay + 2), s3 = zk_rd16(pay + 4), q = (regen + 3) / 4;
                if (6 + s1 + s2 + s3 > size || 3 * q > regen) ok = false;
                else {
                    const uint32_t s4 = size - 6 - s1 - s2 - s3;
                    for (uint32_t s = 0; s < 4 && ok; s++) {
                        const uint32_t start = 6 + (s > 0 ? s1 : 0) + (s > 1 ? s2 : 0) + (s > 2 ? s3 : 0);
                        ok = zk_huf_decode_stream(tab.data(), mb, pay + start, s == 0 ? s1 : s == 1 ? s2 : s == 2 ? s3 : s4, d + s * q, s == 3 ? regen - 3 * q : q);
                    }
                }
            }
        }
        if (!ok) b.status = ZK_E_CORRUPTION;
    }
    // sequences: zk_k_fse's lane (tables of the block in force, the dictionary's entry among them)
    ZkSeqTables16 *T = new ZkSeqTables16;
    for (uint64_t bi = 0; bi < nb; bi++) {
        ZkBlock b = blocks[bi];
        if (b.type != 2 || b.nseq == 0 || b.status != ZK_OK) continue;
        zk_decode_sequences<ZkRevU, ZkCells16>(comp, blocks.data(), b, T, seqs.data() + b.seq_base, LLV, MLV);
        blocks[bi].out_size = b.out_size; blocks[bi].status = b.status;
        for (int k = 0; k < 3; k++) blocks[bi].rep_out[k] = b.rep_out[k];
    }
    delete T;
    // execution: zk_k_exec's rules (offsets bounded by availability with a prefix, by the window without), byte by byte
    for (uint32_t f = 0; f < count; f++) {
        uint32_t err = infos[f].status;
        uint8_t *out = dst + d_off[f];
        const uint64_t d_size = d_off[f + 1] - d_off[f];
        uint64_t pos = 0;
        uint32_t rep[3] = {plen ? L.rep[0] : 1u, plen ? L.rep[1] : 4u, plen ? L.rep[2] : 8u};
        const uint32_t block_max = infos[f].window < ZK_BLOCK_MAX ? infos[f].window : ZK_BLOCK_MAX;
        for (uint32_t bk = 0; bk < infos[f].n_blocks && err == ZK_OK; bk++) {
            const ZkBlock &b = blocks[bases[f].block_base + bk];
            if (b.status != ZK_OK) { err = b.status; break; }
            if (pos + b.out_size > d_size || b.out_size > block_max) { err = ZK_E_CORRUPTION; break; }
            uint8_t *bout = out + pos;
            if (b.type == 0) memcpy(bout, comp + b.src, b.bsize);
            else if (b.type == 1) memset(bout, comp[b.src], b.bsize);
            else {
                const uint8_t *l = b.lit_type >= 2 ? lit.data() + b.lit_base : comp + b.src + b.lit_off;
                const ZkSeqP *sq = seqs.data() + b.seq_base;
                uint32_t o = 0, li = 0;
                for (uint32_t i = 0; i < b.nseq && err == ZK_OK; i++) {
                    const ZkSeq q = zk_seq_unpack(i ? sq[i - 1] : 0, sq[i], i == 0);
                    const uint32_t off = zk_rep_resolve(q.off, rep), ms = q.out_end - q.ml;
                    if (off == 0 || (plen ? pos + ms + plen < off : (pos + ms < off || off > infos[f].window)) || q.ml > q.out_end) { err = ZK_E_CORRUPTION; break; }
                    for (; o < ms; o++, li++) bout[o] = b.lit_type == 1 ? l[0] : l[li];
                    for (; o < q.out_end; o++) {
                        const int64_t src = (int64_t)pos + o - off;
                        bout[o] = src < 0 ? content[plen + src] : out[src];
                    }
                }
                for (; err == ZK_OK && o < b.out_size; o++, li++) bout[o] = b.lit_type == 1 ? l[0] : l[li];
                const uint32_t r0 = zk_rep_resolve(b.rep_out[0], rep), r1 = zk_rep_resolve(b.rep_out[1], rep), r2 = zk_rep_resolve(b.rep_out[2], rep);
                rep[0] = r0; rep[1] = r1; rep[2] = r2;
            }
            pos += b.out_size;
        }
        if (err == ZK_OK && pos != d_size) err = ZK_E_CORRUPTION;
        status[f] = (int32_t)err;
    }
    return 0;
}

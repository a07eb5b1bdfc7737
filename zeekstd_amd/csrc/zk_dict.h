// zk_dict.h -- zstd dictionaries (RFC 8878 section 5) for the decoder: parsing and validation on the host, and the form in which a
// dictionary's entropy tables reach the kernels.
//
// A formatted dictionary is  magic 0xEC30A437 | Dictionary_ID | Huffman tree description | FSE descriptions OF, ML, LL | three
// repeat offsets (4 bytes each, little endian) | content.  Anything else is a raw-content dictionary: ID 0, no tables, repeat
// offsets 1 / 4 / 8, every byte content.  The descriptions are read with the lane code's own parsers (zk_huf_read_weights,
// zk_fse_read_ncount): what creation accepts is exactly what the kernels can build tables from.
//
// HOW THE KERNELS SEE THE TABLES.  Every kernel names "the table in force" by the index of the block whose header carries its
// description (ZkBlock::huf_def / tab_def[3]) and reads it at comp + blocks[index].src.  A dictionary is therefore handed to
// them as one more BLOCK: the entry behind the batch's last block (index = the batch's block count, which no real block has)
// describes a block whose "content" is the dictionary's entropy section, re-ordered into a block's order -- tree description,
// then LL, OF, ML (each FSE description ends on a byte boundary, so they can be moved as bytes) -- and a frame's walk starts
// with huf_def / tab_def[] set to that index.  No kernel tests for a dictionary: table setup follows the index as for any
// Treeless / Repeat_Mode block, and blocks of different frames that repeat the dictionary's tables carry the same key, so the
// shared-table kernels serve them with one copy per workgroup.
#pragma once
#include <vector>
#include "zk_device.h"

constexpr uint32_t ZK_DICT_MAGIC = 0xEC30A437u;

struct ZkDictLayout {
    bool formatted;
    uint32_t id;
    uint32_t huf_off, huf_len;                       // tree description
    uint32_t of_off, of_len, ml_off, ml_len, ll_off, ll_len;
    uint32_t rep[3];
    size_t content_off;                              // first byte of Content (0 for raw content)
};

// 0, or ZK_E_DICT_CORRUPTED (what ZSTD_loadDEntropy refuses: a truncated or invalid entropy section, a repeat offset that is 0
// or larger than the content)
static inline uint32_t zk_dict_parse(const uint8_t *d, size_t len, ZkDictLayout &L)
{
    L = ZkDictLayout{};
    L.rep[0] = 1; L.rep[1] = 4; L.rep[2] = 8;
    if (len < 8 || zk_rd32(d) != ZK_DICT_MAGIC) return ZK_OK;          // raw content
    L.formatted = true;
    L.id = zk_rd32(d + 4);
    size_t p = 8;
    const auto left = [&]() { return (uint32_t)(len - p < 0x10000u ? len - p : 0x10000u); };
    {
        ZkHufHdr hd; ZkHufTmp tmp;
        uint32_t n = 0, mb = 0;
        const uint32_t r = zk_huf_read_weights(d + p, left(), &hd, &tmp, &n, &mb);
        if (!r) return ZK_E_DICT_CORRUPTED;
        // HUF_readStats: a Huffman tree's deepest leaves come in pairs, so the symbols of weight 1 are two at least and even in number.
        // The lane code builds a table from other weights too (weights 2, 2 decode like 1, 1); libzstd does not load such a dictionary.
        uint32_t ones = 0;
        for (uint32_t i = 0; i < n; i++) ones += hd.weights[i] == 1;
        if (ones < 2 || (ones & 1)) return ZK_E_DICT_CORRUPTED;
        L.huf_off = (uint32_t)p; L.huf_len = r; p += r;
    }
    const int order[3] = {ZK_TAB_OF, ZK_TAB_ML, ZK_TAB_LL};
    for (int k = 0; k < 3; k++) {
        const int t = order[k];
        int16_t norm[64];
        uint32_t nsym = 0, al = 0;
        if (p >= len) return ZK_E_DICT_CORRUPTED;
        const uint32_t r = zk_fse_read_ncount(d + p, left(), zk_tab_maxsym(t), zk_tab_maxal(t), norm, &nsym, &al);
        if (!r) return ZK_E_DICT_CORRUPTED;
        // the table must build (zk_seq_table_setup does the same per block)
        uint32_t cells[512]; uint16_t next[64];
        if (!zk_fse_build<ZkCells32>(cells, norm, nsym, al, next, nullptr)) return ZK_E_DICT_CORRUPTED;
        uint32_t &off = t == ZK_TAB_OF ? L.of_off : t == ZK_TAB_ML ? L.ml_off : L.ll_off;
        uint32_t &ln = t == ZK_TAB_OF ? L.of_len : t == ZK_TAB_ML ? L.ml_len : L.ll_len;
        off = (uint32_t)p; ln = r; p += r;
    }
    if (len - p < 12) return ZK_E_DICT_CORRUPTED;
    const size_t content = len - p - 12;
    for (int i = 0; i < 3; i++) {
        L.rep[i] = zk_rd32(d + p + 4 * i);
        if (L.rep[i] == 0 || L.rep[i] > content) return ZK_E_DICT_CORRUPTED;
    }
    L.content_off = p + 12;
    return ZK_OK;
}

// The dictionary's entropy section as the content of a block (see above): img = tree description | LL | OF | ML descriptions
// (+ ZK_DEV_COMP_PADDING zero bytes), blk = the block entry that goes with it.  The caller sets blk.src (where img lies, relative
// to the batch's compressed buffer) and blk.huf_def / tab_def[] (the entry's own index).
static inline void zk_dict_block(const uint8_t *d, const ZkDictLayout &L, std::vector<uint8_t> &img, ZkBlock &blk)
{
    img.clear();
    img.insert(img.end(), d + L.huf_off, d + L.huf_off + L.huf_len);
    img.insert(img.end(), d + L.ll_off, d + L.ll_off + L.ll_len);
    img.insert(img.end(), d + L.of_off, d + L.of_off + L.of_len);
    img.insert(img.end(), d + L.ml_off, d + L.ml_off + L.ml_len);
    const uint32_t n = (uint32_t)img.size();
    img.insert(img.end(), ZK_DEV_COMP_PADDING, 0);
    memset(&blk, 0, sizeof blk);
    blk.bsize = n;
    blk.type = 2; blk.lit_type = 2; blk.lit_streams = 1;
    blk.seq_modes = 0xA8;                            // FSE_Compressed_Mode for LL, OF and ML
    blk.lit_off = 0; blk.lit_comp = L.huf_len;
    blk.seq_off = L.huf_len - 1;                     // the descriptions start one byte behind "the modes byte"
    blk.huf_def = blk.tab_def[0] = blk.tab_def[1] = blk.tab_def[2] = 0xFFFFFFFFu;
    blk.status = ZK_OK;
}

struct zk_dict {
    std::vector<uint8_t> bytes;
    ZkDictLayout L;
};

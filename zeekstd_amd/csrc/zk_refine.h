// zk_refine.h -- the ENTRY walk of zk_refine_entries (include/zeekstd_amd.h): where the frames of a seek-table entry begin.
//
// A seek-table entry may be any chain of Zstandard frames and skippable frames (seekable_format.md: an archive consists of "Zstandard
// compressed frames and skippable frames"; the reference feeds ZSTD_decompressStream from the entry's first byte and libzstd walks
// through whatever frames follow, lib/src/decode.rs:206-267).  zk_split_entry finds their first bytes: one lane per entry, a chain of
// dependent loads like zk_walk_frame -- a frame header, then block header to block header (3 bytes + content; a raw or RLE block needs
// its header only), the 4-byte checksum where the header's flag says so; a skippable frame by its size field.  It judges nothing it
// does not need for the next hop: every piece it emits is walked by zk_walk_frame afterwards, and that verdict is the entry's.
//
// ZK_HD like everything in zk_device.h: tests/sim/ runs the same lane code on the CPU (tests/test_refine_entries.py,
// tests/sim/entry_split_fuzz.cpp).
#pragma once
#include "zk_device.h"

// Why the walk stopped before the entry's last byte (ZkSplit::stop); 0: it did not -- the entry is a whole number of frames.
// The codes are what zk_walk_frame says of the piece that begins where the walk stopped (a trailing piece that begins with neither magic
// is `srcSize_wrong` for the ENTRY -- its size does not match its frames -- unless it is the entry's first frame: zk_refine_verdict).
struct ZkSplit {
    uint32_t n;         // pieces: the complete frames, plus one for whatever is left where the walk stopped (never 0)
    uint32_t stop;      // ZK_OK, or the reason as a ZSTD_ErrorCode
};

// comp[c_begin, c_end) is the entry (the caller has checked c_begin <= c_end <= the buffer's size); every read stays below c_end.
// starts == nullptr: count only; else starts[0 .. n) receive the pieces' first bytes (absolute offsets).
// Every hop advances by at least 3 bytes (a block header), a frame by at least 8, so the walk ends after at most (c_end - c_begin) / 3 hops.
ZK_HD ZkSplit zk_split_entry(const uint8_t *comp, uint64_t c_begin, uint64_t c_end, uint64_t *starts)
{
    ZkSplit s; s.n = 0; s.stop = ZK_OK;
    uint64_t p = c_begin;                                   // first byte of the frame at hand
    for (;;) {
        if (s.n == 0xFFFFFFFFu) { s.stop = ZK_E_GENERIC; return s; }     // (an entry of more than 2^32 - 2 frames: beyond every table)
        if (starts) starts[s.n] = p;
        s.n++;
        const uint64_t left = c_end - p;
        if (left < 4) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }        // (an empty entry too: it holds no frame)
        const uint8_t *f = comp + p;
        const uint32_t magic = zk_rd32(f);
        uint64_t q;                                         // bytes of this frame
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            if (left < 8) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }
            q = 8ull + zk_rd32(f + 4);
            if (q > left) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }
        } else if (magic == 0xFD2FB528u) {
            if (left < 6) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }
            const uint32_t fhd = f[4];
            const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, cks = (fhd >> 2) & 1, did = fhd & 3;
            q = 5ull + (single ? 0u : 1u) + (did == 3 ? 4u : did) + (fcs_flag == 0 ? single : (1u << fcs_flag));
            if (q > left) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }
            for (;;) {
                if (q + 3 > left) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }
                const uint32_t bh = zk_rd24(f + q);
                const uint32_t last = bh & 1, type = (bh >> 1) & 3, bsize = bh >> 3;
                if (type == 3) { s.stop = ZK_E_CORRUPTION; return s; }
                q += 3ull + (type == 1 ? 1u : bsize);
                if (q > left) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; }
                if (last) break;
            }
            if (cks) { q += 4; if (q > left) { s.stop = ZK_E_SRC_SIZE_WRONG; return s; } }
        } else { s.stop = ZK_E_PREFIX_UNKNOWN; return s; }
        p += q;
        if (p == c_end) return s;
    }
}

// The entry's verdict from its pieces' own (zk_walk_frame + the sequence walks, as -ZSTD_ErrorCode or 0): the first piece that fails
// decides.  j: that piece's index in the entry, code: its positive ZSTD_ErrorCode.  A piece behind a complete frame that begins with
// neither magic is the ENTRY's srcSize_wrong ("the entry's size does not match its frames": today's verdict for such an entry).
ZK_HD uint32_t zk_refine_verdict(uint32_t j, uint32_t code)
{
    return (j > 0 && code == ZK_E_PREFIX_UNKNOWN) ? (uint32_t)ZK_E_SRC_SIZE_WRONG : code;
}

// zk_ranges.h -- the arithmetic of a byte-range read (zk_read_ranges*, include/zeekstd_amd.h): which frames a range
// [off, off + len) of the decompressed stream touches and which bytes of each it wants.  Host + device: the plan kernels of
// zk_ranges.hip, the host-pointer entry point and tests/test_ranges_plan.py (which compiles this file with g++) run the same code.
// Everything is 64-bit: d_off, offsets, lengths and sums may pass 2^32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZKR_HD __host__ __device__ __forceinline__
#else
#define ZKR_HD static inline
#endif

// per-range codes (what d_range_status receives; the values of include/zeekstd_amd.h)
#define ZKR_OK 0
#define ZKR_E_OFFSET_OUT_OF_RANGE (-1001)   /* ZK_ERR_OFFSET_OUT_OF_RANGE: off + len leaves the decompressed stream (or overflows) */
#define ZKR_E_DST_TOO_SMALL (-70)           /* dstSize_tooSmall: dst_off + len leaves the destination (or overflows) */

// The frame an offset belongs to: the LAST f with d_off[f] <= off, i.e. np.searchsorted(d_off, off, "right") - 1 over the n + 1
// prefix sums.  That is the reference's edge rule (SeekTable::frame_index_decomp, lib/src/seek_table.rs:579-596; set_offset,
// decode.rs:402-417): an offset on a frame boundary belongs to the frame that STARTS there, and of several frames that start
// there -- empty ones in front of a non-empty one -- the last, so empty frames are skipped.  off == d_off[n] gives n (no frame:
// only an empty range may start there).  d_off[0] <= off is the caller's to ensure (d_off[0] == 0 for every seek table).
ZKR_HD uint32_t zkr_frame_of(const uint64_t *d_off, uint32_t n_frames, uint64_t off)
{
    uint32_t lo = 0, hi = n_frames + 1;             // invariant: d_off[lo] <= off; hi == n + 1 or d_off[hi] > off
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (d_off[mid] <= off) lo = mid; else hi = mid;
    }
    return lo;
}

// Validation of one range against the stream (total = d_off[n_frames]) and its destination.
ZKR_HD int32_t zkr_check_src(uint64_t total, uint64_t off, uint64_t len)
{
    return (off > total || len > total - off) ? ZKR_E_OFFSET_OUT_OF_RANGE : ZKR_OK;
}
ZKR_HD int32_t zkr_check_dst(uint64_t dst_cap, uint64_t dst_off, uint64_t len)
{
    return (dst_off > dst_cap || len > dst_cap - dst_off) ? ZKR_E_DST_TOO_SMALL : ZKR_OK;
}
ZKR_HD int32_t zkr_check(uint64_t total, uint64_t off, uint64_t len, uint64_t dst_cap, uint64_t dst_off)
{
    const int32_t s = zkr_check_src(total, off, len);
    return s ? s : zkr_check_dst(dst_cap, dst_off, len);
}

// First and last frame of a valid range with len > 0 (both non-empty by the edge rule; frames between them may be empty and
// are then not touched).  Returns 0 for a range that touches nothing (len == 0).
ZKR_HD int zkr_span(const uint64_t *d_off, uint32_t n_frames, uint64_t off, uint64_t len, uint32_t *first, uint32_t *last)
{
    if (len == 0) return 0;
    *first = zkr_frame_of(d_off, n_frames, off);
    *last = zkr_frame_of(d_off, n_frames, off + (len - 1));
    return 1;
}

// The piece of range [off, off + len) that lies in frame f: bytes [*at, *at + *n) of the frame, which land *dst_at bytes into the
// range's destination.  n == 0: the frame holds nothing of the range (an empty frame, or one outside the span).
ZKR_HD void zkr_piece(const uint64_t *d_off, uint32_t f, uint64_t off, uint64_t len, uint64_t *at, uint64_t *n, uint64_t *dst_at)
{
    const uint64_t fb = d_off[f], fe = d_off[f + 1], end = off + len;
    const uint64_t lo = off > fb ? off : fb, hi = end < fe ? end : fe;
    if (hi <= lo) { *at = 0; *n = 0; *dst_at = 0; return; }
    *at = lo - fb; *n = hi - lo; *dst_at = lo - off;
}

// A range cut to the window [wlo, whi) of decompressed coordinates that one decode pass holds (whi > wlo): bytes
// [*lo, *lo + *n) of the stream, *lo - off bytes into the range's destination.
ZKR_HD void zkr_clip(uint64_t off, uint64_t len, uint64_t wlo, uint64_t whi, uint64_t *lo, uint64_t *n)
{
    const uint64_t end = off + len;
    const uint64_t a = off > wlo ? off : wlo, b = end < whi ? end : whi;
    *lo = a; *n = b > a ? b - a : 0;
}

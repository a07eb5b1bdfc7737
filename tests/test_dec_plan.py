"""What a decode decides from the shape of its batch (zeekstd_amd/csrc/zk_dec_plan.h: the checksum follower, the executor in segments on the
device path and on the host-pointer small path) compiled with g++ and pinned at its edges.  The expectations are literal: read off the
conditions as they stood in zk_engine.hip (zk_follow_wanted, zk_seg_wanted) and zk_engine_host.hip (zk_decode_small).  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 131072                  # ZK_SEG_BYTES
K = 512 << 10               # ZK_FOLLOW_MIN_FRAME_BYTES

CLIENT = r"""
#include "zk_dec_plan.h"
static ZkDecShape shape(int xxh, int exec_seg, int seg_kib, int profiling, uint32_t count, uint64_t out_bytes, uint64_t max_frame, uint64_t nblocks,
                        int has_prefix, int alone, int follow)
{
    return ZkDecShape{xxh, exec_seg, seg_kib, profiling != 0, count, out_bytes, max_frame, nblocks, has_prefix != 0, alone != 0, follow != 0};
}
static int plan_out(const ZkSegPlan &p, uint32_t *seg_bytes, uint32_t *max_segs) { *seg_bytes = p.seg_bytes; *max_segs = p.max_segs; return p.on; }
extern "C" {
uint32_t t_seg_bytes(void) { return ZK_SEG_BYTES; }
uint64_t t_follow_min(void) { return ZK_FOLLOW_MIN_FRAME_BYTES; }
int t_scan_index(int k)
{
    const int v[8] = {ZK_SCAN_BLOCKS, ZK_SCAN_SEQS, ZK_SCAN_LITS, ZK_SCAN_OWN_TABLES, ZK_SCAN_OUT_BYTES, ZK_SCAN_MAX_FRAME, ZK_SCAN_CHECKSUMMED, ZK_SCAN_WORDS};
    return v[k];
}
int t_follow(int xxh, int profiling, uint32_t count, uint64_t out_bytes, int alone) { return zk_follow_wanted(shape(xxh, 0, 0, profiling, count, out_bytes, 0, 0, 0, alone, 0)); }
int t_seg_dev(int exec_seg, int seg_kib, uint32_t count, uint64_t out_bytes, uint64_t max_frame, uint64_t nblocks, int has_prefix, int follow, uint32_t *seg_bytes, uint32_t *max_segs)
{
    return plan_out(zk_seg_plan_dev(shape(0, exec_seg, seg_kib, 0, count, out_bytes, max_frame, nblocks, has_prefix, 0, follow)), seg_bytes, max_segs);
}
int t_seg_small(int exec_seg, int seg_kib, uint32_t count, uint64_t out_bytes, uint64_t max_frame, uint64_t nblocks, int has_prefix, uint32_t *seg_bytes, uint32_t *max_segs)
{
    return plan_out(zk_seg_plan_small(shape(0, exec_seg, seg_kib, 0, count, out_bytes, max_frame, nblocks, has_prefix, 1, 0)), seg_bytes, max_segs);
}
int t_small_wants_blocks(int exec_seg, int seg_kib, uint32_t count, uint64_t out_bytes, uint64_t max_frame, int has_prefix)
{
    return zk_small_wants_blocks(shape(0, exec_seg, seg_kib, 0, count, out_bytes, max_frame, 0, has_prefix, 1, 0));
}
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("dec_plan")
    src = d / "client.cpp"
    src.write_text(CLIENT)
    so = d / "libdec_plan.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "zeekstd_amd", "csrc"), "-o", str(so), str(src)])
    l = C.CDLL(str(so))
    l.t_seg_bytes.restype = C.c_uint32
    l.t_follow_min.restype = C.c_uint64
    l.t_follow.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_int]
    l.t_seg_dev.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    l.t_seg_small.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    l.t_small_wants_blocks.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int]
    return l


def follow(l, count, out_bytes, alone=True, xxh=0, profiling=False):
    return bool(l.t_follow(xxh, int(profiling), count, out_bytes, int(alone)))


def seg_dev(l, count=4, out_bytes=None, max_frame=4 * S, nblocks=100, exec_seg=0, seg_kib=0, prefix=False, follow=False):
    """-> (segments?, segment bytes, segments per frame at most); a handful of 512 KiB frames unless told otherwise"""
    sb, ms = C.c_uint32(), C.c_uint32()
    on = l.t_seg_dev(exec_seg, seg_kib, count, count * 4 * S if out_bytes is None else out_bytes, max_frame, nblocks, int(prefix), int(follow), C.byref(sb), C.byref(ms))
    return bool(on), sb.value, ms.value


def seg_small(l, count, out_bytes, max_frame, nblocks=0, exec_seg=0, seg_kib=0, prefix=False):
    sb, ms = C.c_uint32(), C.c_uint32()
    on = l.t_seg_small(exec_seg, seg_kib, count, out_bytes, max_frame, nblocks, int(prefix), C.byref(sb), C.byref(ms))
    return bool(on), sb.value, ms.value


def test_constants_and_scan_words(plan):
    assert plan.t_seg_bytes() == S and plan.t_follow_min() == K
    # blocks, sequences, literals, blocks with own tables, output bytes, longest frame, frames with a checksum; words read back
    assert [plan.t_scan_index(k) for k in range(8)] == [0, 1, 2, 4, 5, 7, 8, 9]


def test_follower(plan):
    big = 1 << 40
    assert not follow(plan, 4, big, profiling=True)
    assert not follow(plan, 4, big, xxh=4, profiling=True)
    for xxh in (1, 2, 3, 5):
        assert not follow(plan, 4, big, xxh=xxh)
    assert follow(plan, 1, 0, xxh=4) and follow(plan, 500, 3, alone=True, xxh=4) and follow(plan, 5000, 3, alone=False, xxh=4)
    assert not follow(plan, 4, 4 * K - 1) and follow(plan, 4, 4 * K)
    assert not follow(plan, 1, K - 1) and follow(plan, 1, K)
    for alone in (True, False):
        assert follow(plan, 64, big, alone)
    assert not follow(plan, 65, big, alone=True) and follow(plan, 65, big, alone=False)
    assert not follow(plan, 1023, big, alone=True) and follow(plan, 1023, big, alone=False)
    assert follow(plan, 1024, big, alone=True) and not follow(plan, 1024, big, alone=False)


def test_segments_on_the_device_path(plan):
    assert seg_dev(plan) == (True, S, 9)
    assert not seg_dev(plan, prefix=True)[0] and not seg_dev(plan, prefix=True, exec_seg=2)[0]
    assert not seg_dev(plan, count=0, out_bytes=0)[0] and not seg_dev(plan, count=0, out_bytes=0, exec_seg=2)[0]
    assert not seg_dev(plan, nblocks=0)[0] and not seg_dev(plan, nblocks=0, exec_seg=2)[0]
    # pinned: never, by shape, wherever it may
    assert not seg_dev(plan, exec_seg=1)[0]
    assert seg_dev(plan, count=100, exec_seg=0)[0] is False and seg_dev(plan, count=100, exec_seg=2) == (True, S, 9)
    assert seg_dev(plan, out_bytes=0, exec_seg=2)[0]
    # not beside the checksum follower at 16 frames or fewer
    assert not seg_dev(plan, count=16, follow=True)[0] and seg_dev(plan, count=17, follow=True)[0]
    assert seg_dev(plan, count=16, follow=False)[0] and not seg_dev(plan, count=1, follow=True)[0]
    assert seg_dev(plan, count=32)[0] and not seg_dev(plan, count=33)[0]
    assert not seg_dev(plan, count=5, out_bytes=5 * 4 * S - 1)[0] and seg_dev(plan, count=5, out_bytes=5 * 4 * S)[0]
    # segments per frame: 2 * ceil(max_frame / seg_bytes) + 1, at most 65535 (a grid's rows)
    assert seg_dev(plan, max_frame=2 << 20) == (True, S, 33)
    assert seg_dev(plan, max_frame=(2 << 20) + 1, seg_kib=48) == (True, 48 << 10, 2 * 43 + 1)
    for exec_seg in (0, 2):
        assert seg_dev(plan, max_frame=32767 * 1024, seg_kib=1, exec_seg=exec_seg) == (True, 1024, 65535)
        assert not seg_dev(plan, max_frame=32767 * 1024 + 1, seg_kib=1, exec_seg=exec_seg)[0]         # 65537


def test_segments_on_the_small_path(plan):
    # long frames: the batch averages four segments' worth per frame
    assert not seg_small(plan, 2, 2 * 4 * S - 1, 4 * S)[0]
    assert seg_small(plan, 2, 2 * 4 * S, 4 * S + 5) == (True, S, 11)
    assert seg_small(plan, 1, 2 << 20, 2 << 20) == (True, S, 33)
    assert seg_small(plan, 1, 2 << 20, 2 << 20, seg_kib=16) == (True, 16384, 257)
    # ... beside the follower too, and beyond 32 frames: where the two paths disagree
    assert seg_small(plan, 40, 40 * 4 * S, 4 * S)[0]
    # short frames: 32 KiB up to one segment, with six blocks per frame to deal out; 4 KiB per segment
    assert not seg_small(plan, 1, 32767, 32767, nblocks=6)[0]
    assert seg_small(plan, 1, 32768, 32768, nblocks=6) == (True, 4096, 17)
    assert seg_small(plan, 1, S, S, nblocks=6) == (True, 4096, 65)
    assert not seg_small(plan, 1, S + 1, S + 1, nblocks=6)[0]
    # ... count * max_segs <= 256 (an odd number per frame: 33 at 64 KiB; 3 at one segment of 128 KiB)
    assert seg_small(plan, 7, 7 * 65536, 65536, nblocks=42) == (True, 4096, 33)        # 231
    assert not seg_small(plan, 8, 8 * 65536, 65536, nblocks=48)[0]                     # 264
    assert seg_small(plan, 85, 85 * S, S, nblocks=6 * 85, seg_kib=128) == (True, S, 3)       # 255
    assert not seg_small(plan, 86, 86 * S, S, nblocks=6 * 86, seg_kib=128)[0]                # 258
    # ... the host's block count
    assert not seg_small(plan, 3, 3 * 65536, 65536, nblocks=17)[0] and seg_small(plan, 3, 3 * 65536, 65536, nblocks=18)[0]
    assert not seg_small(plan, 3, 3 * 65536, 65536, nblocks=0)[0]                      # a frame the host's walk refused
    assert seg_small(plan, 3, 3 * 65536, 65536, nblocks=18, seg_kib=8) == (True, 8192, 17)
    # it is asked for only where the verdict hangs on it
    wants = plan.t_small_wants_blocks
    assert wants(0, 0, 3, 3 * 65536, 65536, 0) == 1 and wants(2, 0, 3, 3 * 65536, 65536, 0) == 0
    assert wants(0, 0, 1, 2 << 20, 2 << 20, 0) == 0 and wants(0, 0, 1, 1000, 1000, 0) == 0
    # pinned
    assert seg_small(plan, 3, 3 * 65536, 65536, nblocks=0, exec_seg=2) == (True, 4096, 33)
    assert seg_small(plan, 1, 1000, 1000, exec_seg=2) == (True, 4096, 3)
    assert not seg_small(plan, 1, 2 << 20, 2 << 20, exec_seg=1)[0] and not seg_small(plan, 3, 3 * 65536, 65536, nblocks=18, exec_seg=1)[0]
    assert not seg_small(plan, 1, 2 << 20, 2 << 20, prefix=True)[0] and not seg_small(plan, 1, 2 << 20, 2 << 20, prefix=True, exec_seg=2)[0]
    assert seg_small(plan, 1, 32767 * 1024, 32767 * 1024, seg_kib=1) == (True, 1024, 65535)
    assert not seg_small(plan, 1, 32767 * 1024 + 1, 32767 * 1024 + 1, seg_kib=1, exec_seg=2)[0]

"""What a decode decides from the shape of its batch (zeekstd_amd/csrc/zk_dec_plan.h: the checksum follower, the executor in segments on the
device path and on the host-pointer small path; which kernel, template instance and grid unit the entropy stage, the executor and the
checksum passes launch) compiled with g++ and pinned at its edges.  The expectations are literal: read off the conditions as they
stood in zk_engine.hip (zk_follow_wanted, zk_seg_wanted), zk_engine_host.hip (zk_decode_small) and the launchers of zk_decode.hip
(zk_launch_fse, zk_launch_fse_rest, zk_entropy_fused_wanted, zk_launch_exec, zk_launch_exec_seg, zk_launch_xxh64, zk_launch_xxh64_follow).  No GPU."""
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
    ZkKernelChoice k;
    k.xxh = xxh; k.exec_seg = exec_seg; k.seg_kib = seg_kib;
    return ZkDecShape{k, profiling != 0, count, out_bytes, max_frame, nblocks, has_prefix != 0, alone != 0, follow != 0};
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
int t_lanes(int which) { return which ? ZK_HUF_BLOCKS : ZK_FSEP_LANES; }
void t_entropy(uint32_t nblocks, uint32_t n_own, uint32_t frames, int fse_own, int fse_shared, int entropy, int rest_always, int no_fusion, int *out)
{
    ZkKernelChoice k;
    k.fse_own = fse_own; k.fse_shared = fse_shared; k.entropy = entropy;
    const ZkEntropyPlan p = zk_entropy_plan(nblocks, n_own, frames, k, rest_always != 0, no_fusion != 0);
    out[0] = p.fused; out[1] = p.quads; out[2] = p.shared; out[3] = p.rest;
}
void t_exec(uint32_t count, uint64_t nseq, uint64_t out_bytes, int has_prefix, int follow, int exec_lanes, int exec_ring, int exec_resident, int *out)
{
    ZkKernelChoice k;
    k.exec_lanes = exec_lanes; k.exec_ring = exec_ring; k.exec_resident = exec_resident;
    const ZkExecPlan p = zk_exec_plan(count, nseq, out_bytes, has_prefix != 0, follow != 0, k);
    out[0] = p.lanes; out[1] = p.ring; out[2] = (int)p.lds_pad;
}
void t_exec_seg(uint32_t count, uint32_t max_segs, uint64_t nseq, uint64_t out_bytes, int exec_lanes, int exec_ring, int seg_fill, int *out)
{
    ZkKernelChoice k;
    k.exec_lanes = exec_lanes; k.exec_ring = exec_ring; k.seg_fill = seg_fill;
    const ZkExecSegPlan p = zk_exec_seg_plan(count, max_segs, nseq, out_bytes, k);
    out[0] = p.lanes; out[1] = p.ring; out[2] = p.fill_lanes; out[3] = p.fill_lds;
}
// which: 0 the decoder's pass (zk_xxh_plan), 1 the encoder's (zk_xxh_plan_enc), 2 the conditions themselves with wide_from / beside given
void t_xxh(int which, uint32_t count, int xxh, int skip, uint32_t wide_from, int beside, int *out)
{
    ZkKernelChoice k;
    k.xxh = xxh;
    const ZkXxhPlan p = which == 0 ? zk_xxh_plan(count, k, skip != 0) : which == 1 ? zk_xxh_plan_enc(count, k) : zk_xxh_plan_from(count, k, skip != 0, wide_from, beside != 0);
    out[0] = p.kernel; out[1] = (int)p.frames_per_wg;
}
void t_xxh_follow(uint32_t count, int *out) { const ZkXxhFollowPlan p = zk_xxh_follow_plan(count); out[0] = p.follow1; out[1] = (int)p.grid; }
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
    l.t_entropy.argtypes = [C.c_uint32] * 3 + [C.c_int] * 5 + [C.c_void_p]
    l.t_exec.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_int] * 5 + [C.c_void_p]
    l.t_exec_seg.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_int] * 3 + [C.c_void_p]
    l.t_xxh.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    l.t_xxh_follow.argtypes = [C.c_uint32, C.c_void_p]
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


# ---- which kernels a stage launches
NONE, LANE_56x8, QUAD_16x1, QUAD_56x4 = 0, 1, 2, 3          # ZkFseRest
FRAME, WIDE, LEAN, FED4 = 0, 1, 2, 3                        # ZkXxhKernel


def entropy(l, nblocks, n_own=0, frames=1, fse_own=0, fse_shared=0, entropy=0, rest_always=False, no_fusion=False):
    """-> (fused, quads: blocks per workgroup of the all-quads kernel, shared: 1 predef / 2 fed / 3 sets, rest)"""
    out = (C.c_int * 4)()
    l.t_entropy(nblocks, n_own, frames, fse_own, fse_shared, entropy, int(rest_always), int(no_fusion), out)
    return bool(out[0]), out[1], out[2], out[3]


def execp(l, count, dense=False, prefix=False, follow=False, lanes=0, ring=0, resident=0, nseq=None, out_bytes=None):
    """-> (lanes, ring, LDS pad); dense: 101 sequences per 1000 bytes of output, otherwise 100"""
    out = (C.c_int * 3)()
    l.t_exec(count, (101 if dense else 100) if nseq is None else nseq, 1000 if out_bytes is None else out_bytes, int(prefix), int(follow), lanes, ring, resident, out)
    return tuple(out)


def segp(l, count, max_segs, dense=False, lanes=0, ring=0, fill=0):
    """-> (lanes, ring, fill pass lanes, fill pass in LDS)"""
    out = (C.c_int * 4)()
    l.t_exec_seg(count, max_segs, 101 if dense else 100, 1000, lanes, ring, fill, out)
    return out[0], out[1], out[2], bool(out[3])


def xxh(l, which, count, xxh=0, skip=False, wide_from=0, beside=False):
    """-> (kernel, frames per workgroup)"""
    out = (C.c_int * 2)()
    l.t_xxh(which, count, xxh, int(skip), wide_from, int(beside), out)
    return tuple(out)


def test_entropy_small_batches_and_shared_kernels(plan):
    assert plan.t_lanes(0) == 64 and plan.t_lanes(1) == 16
    assert entropy(plan, 0) == entropy(plan, 0, 5, 5, entropy=2, rest_always=True) == (False, 0, 0, NONE)
    # every block a quad of lanes up to 4096 blocks, in 8-block workgroups up to 2048; nothing behind them
    assert entropy(plan, 1) == entropy(plan, 2048) == entropy(plan, 2048, n_own=5, frames=5, rest_always=True) == (False, 8, 0, NONE)
    assert entropy(plan, 2049) == entropy(plan, 4096) == entropy(plan, 4096, n_own=9, frames=9) == (False, 16, 0, NONE)
    assert entropy(plan, 4097) == (False, 0, 1, NONE)
    # ... unless a sequence kernel is pinned
    assert entropy(plan, 100, fse_own=1) == entropy(plan, 100, fse_own=2) == entropy(plan, 100, fse_shared=1) == (False, 0, 1, NONE)
    assert entropy(plan, 100, fse_shared=3) == (False, 0, 3, NONE)
    assert entropy(plan, 100, fse_shared=2, no_fusion=True) == (False, 0, 2, NONE)
    # frames of fewer than 64 blocks: zk_k_fse_sets
    assert entropy(plan, 6399, frames=100) == (False, 0, 3, NONE) and entropy(plan, 6400, frames=100) == (False, 0, 1, NONE)
    assert entropy(plan, 6399, frames=0) == (False, 0, 1, NONE)
    # 1536 workgroups of 64 blocks: zk_k_fse_predef_fed, and with it the fused kernel
    assert entropy(plan, 98240, frames=1000) == (False, 0, 1, NONE)
    assert entropy(plan, 98241, frames=1000) == (True, 0, 2, NONE) and entropy(plan, 98241, frames=1000, no_fusion=True) == (False, 0, 2, NONE)
    assert entropy(plan, 98241, frames=1536) == (False, 0, 3, NONE)            # 98241 < 64 * 1536: sets come first
    # a pinned shared-table kernel wins over shape
    assert entropy(plan, 98241, frames=1000, fse_shared=1) == (False, 0, 1, NONE)
    assert entropy(plan, 98241, frames=1000, fse_shared=3) == (False, 0, 3, NONE)
    assert entropy(plan, 6399, frames=100, fse_shared=1) == (False, 0, 1, NONE)
    assert entropy(plan, 6399, frames=100, fse_shared=2, no_fusion=True) == (False, 0, 2, NONE)
    assert entropy(plan, 5000, fse_shared=2, no_fusion=True) == (False, 0, 2, NONE)


def test_entropy_rest_pass(plan):
    # (frames = 0: no fused kernel, zk_k_fse_predef in front)
    assert entropy(plan, 20000, n_own=0, frames=0) == (False, 0, 1, NONE)
    assert entropy(plan, 20000, n_own=0, frames=0, rest_always=True) == (False, 0, 1, QUAD_16x1)
    assert entropy(plan, 20000, n_own=1, frames=0) == (False, 0, 1, QUAD_16x1)
    assert entropy(plan, 20000, n_own=12288, frames=0) == (False, 0, 1, QUAD_16x1)
    assert entropy(plan, 20000, n_own=12289, frames=0) == (False, 0, 1, QUAD_56x4)
    assert entropy(plan, 20000, n_own=1, frames=0, fse_own=1) == entropy(plan, 20000, n_own=12289, frames=0, fse_own=1) == (False, 0, 1, LANE_56x8)
    assert entropy(plan, 20000, n_own=0, frames=0, fse_own=1, rest_always=True) == (False, 0, 1, LANE_56x8)
    assert entropy(plan, 20000, n_own=1, frames=0, fse_own=2) == (False, 0, 1, QUAD_56x4)
    assert entropy(plan, 20000, n_own=0, frames=0, fse_own=1) == entropy(plan, 20000, n_own=0, frames=0, fse_own=2) == (False, 0, 1, NONE)
    # behind the pinned kernels and the fused one alike
    assert entropy(plan, 100, n_own=1, frames=1, fse_own=1) == (False, 0, 1, LANE_56x8) and entropy(plan, 100, n_own=3, frames=3, fse_own=1) == (False, 0, 3, LANE_56x8)
    assert entropy(plan, 98241, n_own=1000, frames=1000) == (True, 0, 2, QUAD_16x1)
    assert entropy(plan, 98241, n_own=1000, frames=1000, no_fusion=True) == (False, 0, 2, QUAD_16x1)


def test_entropy_fused(plan):
    big = dict(n_own=1000, frames=1000)
    assert entropy(plan, 98241, **big) == (True, 0, 2, QUAD_16x1)
    assert entropy(plan, 98241, n_own=1001, frames=1000) == (False, 0, 2, QUAD_16x1)          # a frame defines more than one set of tables
    assert entropy(plan, 98241, entropy=1, **big) == (False, 0, 2, QUAD_16x1)
    assert entropy(plan, 98241, fse_own=1, **big) == (False, 0, 2, LANE_56x8) and entropy(plan, 98241, fse_own=2, **big) == (False, 0, 2, QUAD_56x4)
    assert entropy(plan, 98241, fse_own=1, entropy=2, **big) == (False, 0, 2, LANE_56x8)
    # by shape exactly where the shared pick is zk_k_fse_predef_fed; a pinned fed kernel counts
    assert entropy(plan, 98240, **big) == (False, 0, 1, QUAD_16x1)
    assert entropy(plan, 98241, n_own=1536, frames=1536) == (False, 0, 3, QUAD_16x1)
    assert entropy(plan, 100, n_own=4, frames=4) == (False, 8, 0, NONE)
    assert entropy(plan, 100, n_own=4, frames=4, fse_shared=2) == (True, 0, 2, QUAD_16x1)
    assert entropy(plan, 98241, fse_shared=1, **big) == (False, 0, 1, QUAD_16x1) and entropy(plan, 98241, fse_shared=3, **big) == (False, 0, 3, QUAD_16x1)
    # entropy = 2: whatever the size, with fse_shared 0 or 2 (quads then names what the fused kernel replaced, and the rest pass follows it)
    assert entropy(plan, 100, n_own=4, frames=4, entropy=2) == (True, 8, 0, QUAD_16x1)
    assert entropy(plan, 100, n_own=0, frames=4, entropy=2) == (True, 8, 0, NONE)
    assert entropy(plan, 3000, n_own=4, frames=4, entropy=2) == (True, 16, 0, QUAD_16x1)
    assert entropy(plan, 5000, n_own=4, frames=4, entropy=2) == (True, 0, 1, QUAD_16x1)
    assert entropy(plan, 100, n_own=4, frames=4, entropy=2, fse_shared=2) == (True, 0, 2, QUAD_16x1)
    assert entropy(plan, 100, n_own=4, frames=4, entropy=2, fse_shared=1) == (False, 0, 1, QUAD_16x1)
    assert entropy(plan, 100, n_own=4, frames=4, entropy=2, fse_shared=3) == (False, 0, 3, QUAD_16x1)
    assert entropy(plan, 100, n_own=5, frames=4, entropy=2) == (False, 8, 0, NONE)
    # never with per-kernel timing or on one queue
    assert entropy(plan, 100, n_own=4, frames=4, entropy=2, no_fusion=True) == (False, 8, 0, NONE)
    assert entropy(plan, 98241, no_fusion=True, **big) == (False, 0, 2, QUAD_16x1)


def test_executor_one_workgroup_per_frame(plan):
    # tile width by batch size and density
    for dense in (False, True):
        assert execp(plan, 1, dense) == execp(plan, 255, dense) == (1024, 2, 0)
        assert execp(plan, 256, dense) == execp(plan, 1023, dense) == (512, 2, 0)
    assert execp(plan, 1024, dense=False) == (256, 2, 0) and execp(plan, 1024, dense=True) == (512, 2, 0)
    # dense: more than a sequence per 10 output bytes
    assert execp(plan, 1024, nseq=100, out_bytes=1000) == (256, 2, 0) and execp(plan, 1024, nseq=100, out_bytes=999) == (512, 2, 0)
    assert execp(plan, 1024, nseq=0, out_bytes=0) == (256, 2, 0) and execp(plan, 1024, nseq=1, out_bytes=0) == (512, 2, 0)
    # pinned tiles, without and with a prefix (which has no 128-lane instance)
    for count in (1, 5000):
        assert [execp(plan, count, lanes=n)[0] for n in (128, 256, 512, 1024)] == [128, 256, 512, 1024]
        assert [execp(plan, count, lanes=n, prefix=True)[0] for n in (128, 256, 512, 1024)] == [256, 256, 512, 1024]
    assert execp(plan, 255, prefix=True) == (1024, 2, 0) and execp(plan, 256, prefix=True) == (512, 2, 0) and execp(plan, 1024, prefix=True) == (256, 2, 0)
    assert execp(plan, 1024, dense=True, prefix=True) == (512, 2, 0)
    # a ring of 4 T records: 256-lane tiles only -- dense batches from 1024 frames (where 256 lanes are a pin), or pinned
    assert execp(plan, 1024, dense=True, lanes=256) == (256, 4, 0) and execp(plan, 1023, dense=True, lanes=256) == (256, 2, 0)
    assert execp(plan, 1024, dense=False, lanes=256) == (256, 2, 0)
    assert execp(plan, 1024, dense=True, lanes=256, ring=1) == (256, 2, 0)
    assert execp(plan, 1024, ring=2) == execp(plan, 1, lanes=256, ring=2) == (256, 4, 0)
    assert execp(plan, 1024, ring=1) == (256, 2, 0)
    assert execp(plan, 500, ring=2) == (512, 2, 0) and execp(plan, 5, ring=2) == (1024, 2, 0) and execp(plan, 5, lanes=128, ring=2) == (128, 2, 0)
    assert execp(plan, 1024, ring=2, prefix=True) == execp(plan, 1024, dense=True, lanes=256, prefix=True) == (256, 2, 0)
    # 2560 bytes of LDS asked for and not used: 256-lane tiles at four workgroups per CU, which the checksum follower wants unless told otherwise
    assert execp(plan, 1024, resident=4) == execp(plan, 1024, follow=True) == execp(plan, 1024, follow=True, resident=4) == (256, 2, 2560)
    assert execp(plan, 1024, resident=5) == execp(plan, 1024, follow=True, resident=5) == (256, 2, 0)
    assert execp(plan, 1024, ring=2, follow=True) == (256, 4, 2560)
    assert execp(plan, 1024, prefix=True, follow=True) == execp(plan, 5, lanes=128, prefix=True, resident=4) == (256, 2, 2560)
    assert execp(plan, 5, lanes=128, follow=True) == execp(plan, 5, lanes=128, resident=4) == (128, 2, 0)
    assert execp(plan, 500, follow=True) == execp(plan, 500, resident=4) == (512, 2, 0)
    assert execp(plan, 5, follow=True) == execp(plan, 5, resident=4, prefix=True) == (1024, 2, 0)
    assert execp(plan, 1024, dense=True, follow=True) == (512, 2, 0)


def test_executor_in_segments(plan):
    # a segment is a workgroup: 1024-lane tiles below 1024 of them
    assert segp(plan, 31, 33) == (1024, 2, 1024, True) and segp(plan, 32, 32) == (256, 2, 1024, True)
    assert segp(plan, 1, 1023) == (1024, 2, 1024, True) and segp(plan, 1, 1024) == (256, 2, 1024, True)
    # exec_lanes: 256 and 1024 are honoured, 128 and 512 have no instance here
    assert segp(plan, 1, 10, lanes=256)[0] == 256 and segp(plan, 100, 50, lanes=1024)[0] == 1024
    for n in (128, 512):
        assert segp(plan, 31, 33, lanes=n)[0] == 1024 and segp(plan, 32, 32, lanes=n)[0] == 256
    # the ring: 4 T at 256 lanes on dense streams, or pinned
    assert segp(plan, 32, 32, dense=True) == (256, 4, 1024, True) and segp(plan, 32, 32, dense=False) == (256, 2, 1024, True)
    assert segp(plan, 32, 32, dense=False, ring=2) == (256, 4, 1024, True) and segp(plan, 32, 32, dense=True, ring=1) == (256, 2, 1024, True)
    assert segp(plan, 1, 10, dense=True, lanes=256) == (256, 4, 1024, True)
    assert segp(plan, 31, 33, dense=True) == segp(plan, 31, 33, ring=2) == segp(plan, 100, 50, dense=True, ring=2, lanes=1024) == (1024, 2, 1024, True)
    # the fill pass: through memory in 256-lane workgroups from 512 frames, the segment's holes in LDS below
    assert segp(plan, 511, 3) == (256, 2, 1024, True) and segp(plan, 512, 3) == (256, 2, 256, False)
    for count in (4, 600):
        assert segp(plan, count, 3, fill=1)[2:] == (1024, False)
        assert segp(plan, count, 3, fill=2)[2:] == (256, False)
        assert segp(plan, count, 3, fill=3)[2:] == (1024, True)


def test_checksum_passes(plan):
    # xxh 0..5 x skip x beside, below and from wide_from
    small = {False: [(FRAME, 1), (FRAME, 1), (WIDE, 16), (LEAN, 16), (FED4, 4), (FED4, 4)],
             True: [(FED4, 4), (FED4, 4), (WIDE, 16), (FED4, 4), (FED4, 4), (FED4, 4)]}
    large = {(False, False): [(FED4, 4), (FRAME, 1), (WIDE, 16), (LEAN, 16), (FED4, 4), (FED4, 4)],
             (False, True): [(WIDE, 16), (FRAME, 1), (WIDE, 16), (LEAN, 16), (FED4, 4), (FED4, 4)],
             (True, False): [(FED4, 4), (FED4, 4), (WIDE, 16), (FED4, 4), (FED4, 4), (FED4, 4)],
             (True, True): [(WIDE, 16), (FED4, 4), (WIDE, 16), (FED4, 4), (FED4, 4), (FED4, 4)]}
    for wide_from in (1024, 512):
        for skip in (False, True):
            for beside in (False, True):
                assert [xxh(plan, 2, wide_from - 1, k, skip, wide_from, beside) for k in range(6)] == small[skip]
                assert [xxh(plan, 2, wide_from, k, skip, wide_from, beside) for k in range(6)] == large[skip, beside]
    # the decoder's pass (and zk_xxh64_frames_dev): from 1024 frames, never wide by shape; behind the follower always zk_k_xxh64_fed<4>
    for skip in (False, True):
        assert [xxh(plan, 0, 1023, k, skip) for k in range(6)] == small[skip] and [xxh(plan, 0, 1024, k, skip) for k in range(6)] == large[skip, False]
    assert xxh(plan, 0, 1) == xxh(plan, 0, 1023) == (FRAME, 1) and xxh(plan, 0, 1024) == (FED4, 4) and xxh(plan, 0, 1, skip=True) == (FED4, 4)
    # the encoder's: from 512 frames, sixteen frames per wave
    assert [xxh(plan, 1, 511, k) for k in range(6)] == small[False] and [xxh(plan, 1, 512, k) for k in range(6)] == large[False, True]
    assert xxh(plan, 1, 511) == (FRAME, 1) and xxh(plan, 1, 512) == xxh(plan, 1, 5000) == (WIDE, 16)


def test_checksum_follower(plan):
    def f(count):
        out = (C.c_int * 2)()
        plan.t_xxh_follow(count, out)
        return bool(out[0]), out[1]
    # a wave per frame up to 32 frames, in eights; beyond, eight waves per 128 frames
    assert f(1) == (True, 8) and f(8) == (True, 8) and f(9) == (True, 16) and f(25) == (True, 32) and f(32) == (True, 32)
    assert f(33) == (False, 8) and f(128) == (False, 8) and f(129) == (False, 16) and f(2048) == (False, 128)

"""What an encode decides from the shape of its call (zeekstd_amd/csrc/zk_enc_sched.h: the far history a call gets, the table entries and where
a list frame's table starts, the slices of whole frames, the size of the dense scratch and of the staged records, the grids of the far-history
kernels, the match-kernel instance) compiled with g++ and pinned at its edges.  The expectations are literal: read off the conditions as they
stood inline in zk_engine_enc.hip (zk_enc_stage_hist, zk_enc_far_history, zk_enc_match) and in the launchers of zk_encode.hip
(zk_launch_enc_ldm_build_frames, zk_launch_enc_ldm_build, zk_launch_enc_match), not computed by the header.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 57280                   # ZKE_WINDOW
SLACK = 4096 + 16           # ZKE_DENSE_SLACK
NONE, INFRAME, PREFIX = 0, 1, 2

CLIENT = r"""
#include "zk_enc_sched.h"
static ZkEncCut cut(const uint64_t *list, uint32_t count, uint64_t n, uint32_t fs) { return ZkEncCut{list, count, n, fs}; }
extern "C" {
uint32_t t_const(int k) { const uint32_t v[4] = {ZKE_WINDOW, ZKE_DENSE_SLACK, ZK_ENC_GRID_Y_MAX, zke_ldm_list_shared()}; return v[k]; }
void t_frame(const uint64_t *list, uint32_t count, uint64_t n, uint32_t fs, uint32_t hist, uint32_t f, uint64_t *out)
{
    out[0] = zk_enc_frame_src(cut(list, count, n, fs), f); out[1] = zk_enc_frame_bytes(cut(list, count, n, fs), f); out[2] = zk_enc_frame_rec(cut(list, count, n, fs), hist, f);
}
void t_far(const uint64_t *list, uint32_t count, uint64_t n, uint32_t fs, int level, uint64_t prefix_len, uint32_t hist, uint32_t nseg, uint64_t dense_slice, uint64_t *out)
{
    const ZkEncFarPlan p = zk_enc_far_plan(cut(list, count, n, fs), level, prefix_len, hist, nseg, dense_slice);
    const uint64_t v[18] = {(uint64_t)p.kind, p.ldm.inframe, p.ldm.frame_size, p.ldm.n_total, p.ldm.log, p.ldm.dlog, p.ldm.plen, p.ldm.u0, p.ldm.nlf, p.lf_bytes, p.entries,
                            p.table_bytes, p.build_gx, p.slice_cap, p.dense_span, p.cand_words, p.poff_words,
                            (uint64_t)(p.ldm.pfx || p.ldm.table || p.ldm.dense || p.ldm.lf)};
    for (int i = 0; i < 18; i++) out[i] = v[i];
}
void t_list_frames(const uint64_t *list, uint32_t count, uint64_t n, uint32_t fs, int level, uint32_t nlf, uint64_t *out)
{
    ZkEncLdmFrame lf[16];
    zk_enc_far_list_frames(cut(list, count, n, fs), level, 0, lf);
    for (uint32_t k = 0; k < nlf; k++) { out[4 * k] = lf[k].start; out[4 * k + 1] = lf[k].tbase; out[4 * k + 2] = lf[k].size; out[4 * k + 3] = lf[k].pad; }
}
void t_stage(const uint64_t *list, uint32_t count, uint64_t n, uint32_t fs, uint32_t hist, int dict, uint64_t dict_slice, uint64_t *out)
{
    const ZkEncStagePlan p = zk_enc_stage_plan(cut(list, count, n, fs), hist, dict != 0, dict_slice);
    out[0] = p.rec_total; out[1] = p.slice_cap; out[2] = p.stage_bytes;
}
void t_slice(const uint64_t *list, uint32_t count, uint64_t n, uint32_t fs, uint32_t hist, uint64_t rec_total, uint64_t slice_cap, uint32_t nseg, uint32_t f0, uint32_t s0, uint32_t *out)
{
    const ZkEncSlice s = zk_enc_slice_end(cut(list, count, n, fs), hist, rec_total, slice_cap, nseg, f0, s0);
    out[0] = s.f1; out[1] = s.s1;
}
uint32_t t_gx_frames(uint32_t bytes) { return zk_enc_ldm_frames_gx(bytes); }
uint32_t t_gy_frames(uint32_t nframes, uint32_t f0) { return zk_enc_ldm_frames_gy(nframes, f0); }
uint32_t t_gx_prefix(uint64_t bytes) { return zk_enc_ldm_prefix_gx(bytes); }
int t_match(int level, int table, int dense) { return zk_enc_match_kernel(level, table != 0, dense != 0); }
// the table's row k: "enumerator|instance|takes ldm"; null behind the last
const char *t_match_row(int k)
{
#define ROW(name, kernel, takes_ldm) #name "|" #kernel "|" #takes_ldm,
    static const char *const rows[] = {ZK_ENC_MATCH_KERNELS(ROW) nullptr};
#undef ROW
    return rows[k];
}
}
"""


@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    d = tmp_path_factory.mktemp("enc_sched")
    src = d / "client.cpp"
    src.write_text(CLIENT)
    so = d / "libenc_sched.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "zeekstd_amd", "csrc"), "-o", str(so), str(src)])
    l = C.CDLL(str(so))
    u32, u64, i, p = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
    cut = [p, u32, u64, u32]
    l.t_const.restype = u32
    l.t_const.argtypes = [i]
    l.t_frame.argtypes = cut + [u32, u32, p]
    l.t_far.argtypes = cut + [i, u64, u32, u32, u64, p]
    l.t_list_frames.argtypes = cut + [i, u32, p]
    l.t_stage.argtypes = cut + [u32, i, u64, p]
    l.t_slice.argtypes = cut + [u32, u64, u64, u32, u32, u32, p]
    for f, a in ((l.t_gx_frames, [u32]), (l.t_gy_frames, [u32, u32]), (l.t_gx_prefix, [u64])):
        f.restype, f.argtypes = u32, a
    l.t_match.argtypes = [i, i, i]
    l.t_match_row.restype = C.c_char_p
    l.t_match_row.argtypes = [i]
    return l


def _cut(sizes=None, n=0, fs=0, base=0):
    """-> (keep-alive, the four arguments of a cut): a list of frame sizes (offsets from `base`), or the uniform cut of n bytes"""
    if sizes is None:
        return None, (None, max(1, -(-n // fs)), n, fs)
    off = [base]
    for s in sizes:
        off.append(off[-1] + s)
    arr = (C.c_uint64 * len(off))(*off)
    return arr, (C.cast(arr, C.c_void_p), len(sizes), off[-1] - base, max(max(sizes), 1))


FAR = ("kind", "inframe", "frame_size", "n_total", "log", "dlog", "plen", "u0", "nlf", "lf_bytes", "entries", "table_bytes", "build_gx", "slice_cap", "dense_span",
       "cand_words", "poff_words", "any_pointer")


def far(l, level, sizes=None, n=0, fs=0, prefix_len=0, hist=0, nseg=0, dense_slice=0, base=0):
    keep, c = _cut(sizes, n, fs, base)
    out = (C.c_uint64 * 18)()
    l.t_far(*c, level, prefix_len, hist, nseg, dense_slice, out)
    return dict(zip(FAR, out))


def slices(l, sizes=None, n=0, fs=0, hist=0, rec_total=None, slice_cap=0, nseg=0, base=0):
    """-> [(f0, f1, s0, s1)] of the whole call"""
    keep, c = _cut(sizes, n, fs, base)
    out, got, f0, s0 = (C.c_uint32 * 2)(), [], 0, 0
    while f0 < c[1]:
        l.t_slice(*c, hist, c[2] if rec_total is None else rec_total, slice_cap, nseg, f0, s0, out)
        assert out[0] > f0, "a slice is never less than a frame"
        got.append((f0, out[0], s0, out[1]))
        f0, s0 = out[0], out[1]
    return got


def test_constants(sched):
    assert [sched.t_const(k) for k in range(4)] == [W, SLACK, 65535, 4096]      # (the shared empty table: 2^zke_ldm_log(ZKE_WINDOW) = 2^12 entries)


def test_frame_accessors(sched):
    out = (C.c_uint64 * 3)()

    def frame(f, hist, **kw):
        keep, c = _cut(**kw)
        sched.t_frame(*c, hist, f, out)
        return list(out)
    # the uniform cut: frames of 60000 over 150000 bytes; a record is hist + frame_size bytes, the short last frame's too
    assert frame(0, 0, n=150000, fs=60000) == [0, 60000, 0]
    assert frame(2, 0, n=150000, fs=60000) == [120000, 30000, 120000]
    assert frame(2, 1000, n=150000, fs=60000) == [120000, 30000, 122000]
    # a list: offsets count from the list's first; a record is hist + the frame's own bytes
    sizes = [70001, 0, 57280, 300003]
    assert frame(0, 0, sizes=sizes, base=1000) == [0, 70001, 0]
    assert frame(1, 0, sizes=sizes, base=1000) == [70001, 0, 70001]
    assert frame(3, 0, sizes=sizes, base=1000) == [127281, 300003, 127281]
    assert frame(3, 1000, sizes=sizes, base=1000) == [127281, 300003, 130281]


@pytest.mark.parametrize("level,kind,dlog", [(0, INFRAME, 17), (1, NONE, 0), (2, INFRAME, 0), (3, INFRAME, 17), (9, INFRAME, 18)])
def test_far_history_case_by_level_and_frame_size(sched, level, kind, dlog):
    # three frames one byte beyond the ring's reach: a table per frame from level 2 on (and at 0), dense candidates at 0 and from 3 on
    p = far(sched, level, n=3 * (W + 1), fs=W + 1, nseg=3)
    assert (p["kind"], p["dlog"], p["any_pointer"]) == (kind, dlog, 0)
    if kind == INFRAME:
        assert (p["inframe"], p["frame_size"], p["n_total"], p["log"], p["plen"], p["u0"], p["nlf"], p["lf_bytes"]) == (1, W + 1, 3 * (W + 1), 12, 0, 0, 0, 0)
        assert (p["entries"], p["table_bytes"], p["build_gx"]) == (3 << 12, 4 * (3 << 12), 14)
        assert (p["dense_span"] != 0) == (dlog != 0)
    else:
        assert not any(p[k] for k in FAR)
    # frames within the ring's reach: nothing at any level
    p = far(sched, level, n=3 * W, fs=W, nseg=3)
    assert not any(p[k] for k in FAR)
    # ... and what counts is the largest frame the call HAS: one short frame of a large frame size
    p = far(sched, level, n=W, fs=1 << 21, nseg=1)
    assert p["kind"] == NONE


def test_far_history_case_by_prefix(sched):
    big = dict(n=3 * (W + 1), fs=W + 1, nseg=3)
    # a prefix of three bytes leaves no history (a multiple of 4) but is a prefix: no far history of any kind
    p = far(sched, 3, prefix_len=3, hist=0, **big)
    assert not any(p[k] for k in FAR)
    assert far(sched, 3, prefix_len=0, hist=0, **big)["kind"] == INFRAME
    # a prefix the ring holds: nothing; one byte more: a table over it
    p = far(sched, 3, prefix_len=W, hist=W, **big)
    assert not any(p[k] for k in FAR)
    p = far(sched, 3, prefix_len=W + 1, hist=W, **big)
    assert (p["kind"], p["plen"], p["u0"], p["log"], p["entries"], p["table_bytes"], p["build_gx"]) == (PREFIX, W + 1, 0, 12, 4096, 16384, 56)
    assert (p["inframe"], p["frame_size"], p["n_total"], p["dlog"], p["nlf"], p["lf_bytes"], p["slice_cap"], p["dense_span"], p["cand_words"], p["poff_words"], p["any_pointer"]) == (0,) * 11
    # at level 1 too (the fast setting has a table instance of its own)
    assert far(sched, 1, prefix_len=W + 1, hist=W, **big)["kind"] == PREFIX
    # beyond the 27 bits an offset has: the table covers the prefix's last 2^27 - 1 bytes, the largest table, the capped grid
    p = far(sched, 3, prefix_len=(1 << 27) + 100, hist=W, **big)
    assert (p["kind"], p["plen"], p["u0"], p["log"], p["entries"], p["build_gx"]) == (PREFIX, (1 << 27) + 100, 101, 23, 1 << 23, 4096)


def test_uniform_table_and_grid_follow_frame_size_and_the_log_the_bytes_there_are(sched):
    # one frame of 61000 bytes under a frame size of 2 MiB: the stride's log is the input's, the grid is the frame size's
    p = far(sched, 3, n=61000, fs=1 << 21, nseg=1)
    assert (p["kind"], p["frame_size"], p["n_total"], p["log"], p["entries"], p["table_bytes"], p["build_gx"]) == (INFRAME, 1 << 21, 61000, 12, 4096, 16384, 512)
    # two frames of 300003 and 70001: the common stride is the larger frame's 2^15
    p = far(sched, 2, n=370004, fs=300003, nseg=3)
    assert (p["log"], p["entries"], p["table_bytes"], p["build_gx"]) == (15, 2 << 15, 8 << 15, 74)


def test_list_entries_and_tbase(sched):
    sizes = [70001, 0, 57280, 300003]
    n = 427284
    for base in (0, 1000):
        p = far(sched, 3, sizes=sizes, nseg=4, base=base)
        # the shared empty table (4096) first, then frame 0's 2^13 and frame 3's 2^15 entries; 2 records of 24 bytes, rounded to 64
        assert (p["kind"], p["inframe"], p["frame_size"], p["n_total"], p["log"], p["nlf"], p["lf_bytes"]) == (INFRAME, 1, 300003, n, 15, 2, 64)
        assert (p["entries"], p["table_bytes"], p["build_gx"]) == (4096 + 8192 + 32768, 4 * 45056, 74)
        assert (p["dlog"], p["slice_cap"], p["dense_span"], p["cand_words"], p["poff_words"]) == (17, 0, n, n + SLACK, 4 * 33)
        keep, c = _cut(sizes, base=base)
        out = (C.c_uint64 * 8)()
        sched.t_list_frames(*c, 3, 2, out)
        assert list(out) == [0, 4096, 70001, 0, 127281, 4096 + 8192, 300003, 0]
    # level 2: the same tables, no dense scratch; level 1: nothing
    p = far(sched, 2, sizes=sizes, nseg=4)
    assert (p["kind"], p["nlf"], p["entries"], p["dlog"], p["dense_span"], p["cand_words"], p["poff_words"]) == (INFRAME, 2, 45056, 0, 0, 0, 0)
    assert far(sched, 1, sizes=sizes, nseg=4)["kind"] == NONE
    # no frame beyond the ring's reach: nothing, at any level
    assert far(sched, 3, sizes=[57280, 0, 100], nseg=2)["kind"] == NONE
    # 130 frames that qualify: 130 * 24 = 3120 bytes of records round up to 3136
    p = far(sched, 2, sizes=[57281] * 130, nseg=130)
    assert (p["nlf"], p["lf_bytes"], p["entries"]) == (130, 3136, 4096 + 130 * 4096)


def test_dense_slice_cap_and_span(sched):
    f = dict(fs=60000, nseg=3)
    span = lambda p: (p["slice_cap"], p["dense_span"], p["cand_words"], p["poff_words"])
    assert span(far(sched, 3, n=180000, dense_slice=90000, **f)) == (90000, 90000, 90000 + SLACK, 99)       # n above the slice: slices
    assert span(far(sched, 3, n=90000, dense_slice=90000, **f)) == (0, 90000, 90000 + SLACK, 99)            # n equal to it: one slice
    assert span(far(sched, 3, n=80000, dense_slice=90000, **f)) == (0, 80000, 80000 + SLACK, 99)            # n below it: the scratch is the input's
    assert span(far(sched, 3, n=180000, dense_slice=1024, **f)) == (60000, 60000, 60000 + SLACK, 99)        # a slice below one frame: one frame per slice
    assert span(far(sched, 3, n=180000, dense_slice=0, **f)) == (0, 180000, 180000 + SLACK, 99)             # the default of 4 GiB
    assert span(far(sched, 3, n=(4 << 30) + 1, fs=1 << 21, nseg=8193 * 8, dense_slice=0)) == (4 << 30, 4 << 30, (4 << 30) + SLACK, 8193 * 8 * 33)
    assert span(far(sched, 2, n=180000, dense_slice=90000, **f)) == (0, 0, 0, 0)                            # level 2: no dense history


def test_slice_step(sched):
    # 60000 x 2 + 30000 under a slice of 90000: the short last frame joins the frame before it; of 60000: a frame each
    u = dict(n=150000, fs=60000, nseg=3)
    assert slices(sched, slice_cap=90000, **u) == [(0, 1, 0, 1), (1, 3, 1, 3)]
    assert slices(sched, slice_cap=60000, **u) == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]
    assert slices(sched, slice_cap=89999, **u) == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]
    assert slices(sched, slice_cap=150000, **u) == [(0, 3, 0, 3)]
    assert slices(sched, slice_cap=0, **u) == [(0, 3, 0, 3)]                                # 0: one slice, whatever the frames
    # frames of two segments each (ZKE_SEGMENT = 256 KiB): the segments are counted along
    assert slices(sched, n=4 * 300000, fs=300000, nseg=8, slice_cap=600000) == [(0, 2, 0, 4), (2, 4, 4, 8)]
    # a list: a frame larger than the slice goes alone; empty frames have no segment
    big = [1000, 300000, 1000, 0, 1000]
    assert slices(sched, sizes=big, nseg=5, slice_cap=100000, base=77) == [(0, 1, 0, 1), (1, 2, 1, 3), (2, 5, 3, 5)]
    # prefix mode: a slice is measured in records (hist + frame): two records of 61000 fit in 122000, not in 121999 -- where two FRAMES would
    pre = dict(n=180000, fs=60000, nseg=3, hist=1000, rec_total=183000)
    assert slices(sched, slice_cap=122000, **pre) == [(0, 2, 0, 2), (2, 3, 2, 3)]
    assert slices(sched, slice_cap=121999, **pre) == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]
    # ... of a list: hist + the frame's own bytes
    assert slices(sched, sizes=[1000, 2000, 3000], nseg=3, hist=100, rec_total=6300, slice_cap=3200) == [(0, 2, 0, 2), (2, 3, 2, 3)]
    assert slices(sched, sizes=[1000, 2000, 3000], nseg=3, hist=100, rec_total=6300, slice_cap=3199) == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]


def test_staged_records(sched):
    out = (C.c_uint64 * 3)()

    def stage(hist, dict_, dict_slice, **kw):
        keep, c = _cut(**kw)
        sched.t_stage(*c, hist, int(dict_), dict_slice, out)
        return tuple(out)                                                                   # (rec_total, slice_cap, stage_bytes)
    u = dict(n=150000, fs=60000)
    assert stage(0, False, 0, **u) == (150000, 0, 0)                                        # no history: the input is the matcher's source
    assert stage(0, True, 100000, **u) == (150000, 0, 0)                                    # (a dictionary without content)
    assert stage(1000, False, 0, **u) == (183000, 0, 183000)                                # the prefix route: every record at once (the short last frame's is a full one)
    assert stage(1000, False, 100000, **u) == (183000, 0, 183000)                           # ... whatever the dictionary route's slice
    assert stage(1000, True, 0, **u) == (183000, 0, 183000)                                 # the dictionary route: 1 GiB
    assert stage(1000, True, 100000, **u) == (183000, 100000, 100000)
    assert stage(1000, True, 183000, **u) == (183000, 0, 183000)                            # a slice that holds the call: one slice
    assert stage(1000, True, 182999, **u) == (183000, 182999, 182999)
    assert stage(1000, True, 1024, **u) == (183000, 61000, 61000)                           # never below one record
    assert stage(W, True, 0, n=(1 << 30) + 1, fs=1 << 20) == (1025 * (W + (1 << 20)), 1 << 30, 1 << 30)
    assert stage(1000, False, 0, sizes=[70001, 0, 57280, 300003]) == (4000 + 427284, 0, 4000 + 427284)     # a list's records are as long as its frames
    assert stage(1000, True, 1024, sizes=[70001, 0, 57280, 300003]) == (431284, 301003, 301003)            # (one record of the largest frame)


def test_grids(sched):
    l = sched
    # zk_k_enc_ldm_build_frames: a workgroup per 4096 bytes of the largest frame, at most 1024
    assert [l.t_gx_frames(b) for b in (1, 4096, 4097, 1023 * 4096, 1023 * 4096 + 1, 1024 * 4096, 1024 * 4096 + 1, 0xFFFFFFFF)] == [1, 1, 2, 1023, 1024, 1024, 1024, 1024]
    # ... and a row per frame, in launches of at most 65535
    assert [l.t_gy_frames(65535, 0), l.t_gy_frames(65536, 0), l.t_gy_frames(65536, 65535), l.t_gy_frames(200000, 131070), l.t_gy_frames(200000, 196605), l.t_gy_frames(1, 0)] == \
        [65535, 65535, 1, 65535, 3395, 1]
    # zk_k_enc_ldm_build: a workgroup per 1024 bytes of prefix, at most 4096
    assert [l.t_gx_prefix(b) for b in (1, 1024, 1025, 4095 * 1024, 4095 * 1024 + 1, 4096 * 1024, 4096 * 1024 + 1, (1 << 27) - 1)] == [1, 1, 2, 4095, 4096, 4096, 4096, 4096]


# the eight instances as zk_launch_enc_match's ladder named them
FAST2, LAZY, LAZY_1K = "zk_k_enc_match2<14>", "zk_k_enc_match<15, 1, 4096, false>", "zk_k_enc_match<15, 1, 1024, false>"
FAST_T, LAZY_T, LAZY_1K_T = "zk_k_enc_match<14, 0, 4096, true>", "zk_k_enc_match<15, 1, 4096, true>", "zk_k_enc_match<15, 1, 1024, true>"
LAZY_D, LAZY_1K_D = "zk_k_enc_match<15, 1, 4096, true, true>", "zk_k_enc_match<15, 1, 1024, true, true>"
MATCH = {  # level: (no far history, a table, a table and dense candidates)
    0: (LAZY, LAZY_T, LAZY_D),
    1: (FAST2, FAST_T, LAZY_D),           # (dense history never comes with the fast setting; the ladder asked for it first)
    2: (LAZY, LAZY_T, LAZY_D),
    5: (LAZY, LAZY_T, LAZY_D),
    6: (LAZY_1K, LAZY_1K_T, LAZY_1K_D),
    9: (LAZY_1K, LAZY_1K_T, LAZY_1K_D),
}


def test_match_kernel(sched):
    rows, k = [], 0
    while sched.t_match_row(k):
        name, kernel, takes = sched.t_match_row(k).decode().split("|")
        rows.append((name, kernel.strip("()"), int(takes)))
        k += 1
    # every instance named once; the one that takes no ZkEncLdm is the level-1 kernel of zk_enc_match2.h
    assert sorted(r[1] for r in rows) == sorted([FAST2, LAZY, LAZY_1K, FAST_T, LAZY_T, LAZY_1K_T, LAZY_D, LAZY_1K_D])
    assert [r[1] for r in rows if not r[2]] == [FAST2]
    for level, want in MATCH.items():
        got = tuple(rows[sched.t_match(level, table, dense)][1] for table, dense in ((0, 0), (1, 0), (1, 1)))
        assert got == want, (level, got)
    # (dense candidates without a table do not occur; the ladder looked at them first all the same)
    assert rows[sched.t_match(3, 0, 1)][1] == LAZY_D

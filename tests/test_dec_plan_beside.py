"""zk_exec_plan's verdict for an executor that runs beside another batch's zk_k_entropy_frame (zeekstd_amd/csrc/zk_dec_plan.h; `beside` is
"not alone, and this batch took the fused kernel" at the call in zk_engine.hip), compiled with g++ as tests/test_dec_plan.py compiles the
rest: four 256-lane workgroups per CU (2 560 bytes of LDS asked for and not used) where the batch has long frames, whatever the follower
says; nothing changes for a batch that is alone, for short frames, for the other tile widths or for a pinned ZK_CHOICE_EXEC_RESIDENT.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 512 << 10               # ZK_FOLLOW_MIN_FRAME_BYTES

CLIENT = r"""
#include "zk_dec_plan.h"
extern "C" void t_exec(uint32_t count, uint64_t nseq, uint64_t out_bytes, int has_prefix, int follow, int exec_lanes, int exec_resident, int beside, int *out)
{
    ZkKernelChoice k;
    k.exec_lanes = exec_lanes; k.exec_resident = exec_resident;
    const ZkExecPlan p = zk_exec_plan(count, nseq, out_bytes, has_prefix != 0, follow != 0, k, beside != 0);
    out[0] = p.lanes; out[1] = p.ring; out[2] = (int)p.lds_pad;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("dec_plan_beside")
    src = d / "client.cpp"
    src.write_text(CLIENT)
    so = d / "libdec_plan_beside.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "zeekstd_amd", "csrc"), "-o", str(so), str(src)])
    l = C.CDLL(str(so))
    l.t_exec.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_int] * 5 + [C.c_void_p]
    return l


def execp(l, count, frame_bytes, beside, follow=False, prefix=False, lanes=0, resident=0, dense=False):
    """-> (lanes, ring, LDS pad) for `count` frames of frame_bytes each; dense: more than one sequence per 10 bytes of output"""
    out = (C.c_int * 3)()
    total = count * frame_bytes
    l.t_exec(count, total // (9 if dense else 11), total, int(prefix), int(follow), lanes, resident, int(beside), out)
    return tuple(out)


def test_four_resident_beside_another_batch_of_long_frames(plan):
    for count in (1024, 2048, 5000):
        assert execp(plan, count, 2 << 20, beside=True) == (256, 2, 2560)
        assert execp(plan, count, K, beside=True) == (256, 2, 2560)
        assert execp(plan, count, 2 << 20, beside=True, prefix=True) == (256, 2, 2560)
        # alone, or short frames: as before
        assert execp(plan, count, 2 << 20, beside=False) == (256, 2, 0)
        assert execp(plan, count, K - 1, beside=True) == (256, 2, 0)
        assert execp(plan, count, K - 1, beside=True, follow=True) == (256, 2, 2560)


def test_other_widths_and_pinned_residency_are_untouched(plan):
    assert execp(plan, 1023, 2 << 20, beside=True) == (512, 2, 0)
    assert execp(plan, 255, 2 << 20, beside=True) == (1024, 2, 0)
    assert execp(plan, 2048, 2 << 20, beside=True, dense=True) == (512, 2, 0)
    assert execp(plan, 2048, 2 << 20, beside=True, resident=5) == (256, 2, 0)
    assert execp(plan, 2048, 2 << 20, beside=True, resident=5, follow=True) == (256, 2, 0)
    assert execp(plan, 2048, 2 << 20, beside=False, resident=4) == (256, 2, 2560)
    assert execp(plan, 5, 2 << 20, beside=True, lanes=128) == (128, 2, 0)

"""What zk_k_entropy_frame and its neighbours cost a CU, read from the code object's metadata (no GPU: the decode kernels are cross-compiled
for gfx950 with the Makefile's flags, device side only, and the `amdhsa.kernels` notes are read the way tools/kinfo.py reads them).

A CU has 163 840 bytes of LDS and 512 registers per SIMD lane.  While two batches overlap, a CU holds workgroups of zk_k_entropy_frame (E)
and of the other batch's zk_k_exec<256, false, 2, false> (X).

  E  the tier it stands at: <= 37 992 bytes, FOUR per CU alone, and four in every mix with X (1 E + 4 X is the only mix of five); <= 96
     registers allocated, no scratch, no spilled vector registers.  (Five per CU in every mix needs <= 32 768 bytes; that layout was built
     and measured as no gain: profiles/r09_entropy_resident.txt.)
  X  exactly 31 032 bytes.  zk_exec_plan's two residencies rest on this size: five workgroups per CU as it is, exactly four with the
     2 560 bytes a launch asks for and does not use (ZkExecPlan::lds_pad).
  zk_k_huf  exactly 25 800 bytes: the same zk_huf_group as E's Huffman half, with its own pool."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeekstd_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

CU_LDS = 163840
ENTROPY_LDS_MAX = 37992          # four per CU; the mix it allows with five workgroups: 1 E + 4 X
VGPR_ALLOC_MAX = 96              # five waves per SIMD: 5 x 96 <= 512
HUF_LDS = 25800
EXEC_LDS = 31032
EXEC_PAD = 2560                  # ZkExecPlan::lds_pad

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: the code object cannot be made")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled kernel name: its metadata fields} of zk_decode.hip's code object"""
    out = str(tmp_path_factory.mktemp("budget") / "zk_decode.s")
    with open(os.path.join(CSRC, "Makefile")) as f:
        flags = re.search(r"^CXXFLAGS \?= (.*)$", f.read(), re.M).group(1).split()
    subprocess.check_call([HIPCC, "--offload-arch=gfx950"] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "zk_decode.hip")],
                          stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for ent in re.split(r"\n  - \.", meta)[1:]:
        fields = dict(re.findall(r"\.?(\w+):\s+(\S+)", ent))
        found[fields["name"]] = fields
    return found


def _one(kernels, prefix):
    hits = [v for k, v in kernels.items() if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, sorted(kernels))
    return hits[0]


def test_entropy_frame_budget(kernels):
    k = _one(kernels, "_Z18zk_k_entropy_frame")
    lds = int(k["group_segment_fixed_size"])
    print("zk_k_entropy_frame: lds", lds, "vgpr", k["vgpr_count"], "scratch", k["private_segment_fixed_size"], "spill", k["vgpr_spill_count"],
          "scalar registers kept in vector lanes", k.get("sgpr_spill_count"))
    assert lds <= ENTROPY_LDS_MAX
    assert 4 * lds <= CU_LDS and lds + 4 * EXEC_LDS <= CU_LDS
    assert (int(k["vgpr_count"]) + 7) // 8 * 8 <= VGPR_ALLOC_MAX
    assert int(k["private_segment_fixed_size"]) == 0
    assert int(k["vgpr_spill_count"]) == 0                   # (scalar registers parked in lanes of a vector register touch no memory: printed)


def test_neighbours_keep_their_lds(kernels):
    assert int(_one(kernels, "_Z8zk_k_huf")["group_segment_fixed_size"]) == HUF_LDS
    assert int(_one(kernels, "_Z9zk_k_execILi256ELb0ELi2ELb0EE")["group_segment_fixed_size"]) == EXEC_LDS


def test_the_executor_pad_means_four_per_cu(kernels):
    """zk_exec_plan's lds_pad (pinned at 2 560 in tests/test_dec_plan.py) turns five resident executor workgroups into exactly four"""
    x = int(_one(kernels, "_Z9zk_k_execILi256ELb0ELi2ELb0EE")["group_segment_fixed_size"])
    assert CU_LDS // x == 5
    assert CU_LDS // (x + EXEC_PAD) == 4


def test_checksum_kernels_keep_their_registers(kernels):
    """The register counts the comments in zk_decode.hip and zk_dec_plan.h rest on: zk_k_xxh64_lean and zk_k_xxh64_follow in 64 (what is
    left on a SIMD beside four executor waves), zk_k_xxh64_wide within the allocation granule above its 78, zk_k_xxh64_fed<4> in 128."""
    for prefix, most in (("_Z15zk_k_xxh64_lean", 64), ("_Z17zk_k_xxh64_follow", 64), ("_Z15zk_k_xxh64_wide", 80), ("_Z14zk_k_xxh64_fedILi4EE", 128)):
        k = _one(kernels, prefix)
        print(prefix, "vgpr", k["vgpr_count"])
        assert int(k["vgpr_count"]) <= most, prefix

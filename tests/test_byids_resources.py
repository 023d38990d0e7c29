"""Static guard on the filter_rows_by_ids kernel (tf_byids.hip), by the method of tests/test_rawtable_resources.py: hipcc cross-compiles to gfx950 ISA
without a GPU, and the kernel descriptors say how many VGPRs and SGPRs, how much scratch and how much LDS each kernel takes.  Descriptors only: no
instruction is looked for.

DESIGN §3.18's occupancy argument, whole: the kernel asks for eight waves per SIMD (`__launch_bounds__(256, 8)`), which is a CU's 32 waves = eight
workgroups of 256 lanes.  Each of a wave's three budgets has to allow that:
  LDS    the LDS variant copies the allowed-ID table into BYIDS_LDS_BUDGET bytes per workgroup: 8 x 16 KiB = 128 KiB of the CU's 160 KiB;
  VGPRs  512 per SIMD lane, handed out in blocks of 8: at most 64 a wave;
  SGPRs  800 per SIMD, handed out in blocks of 16, and a wave is charged VCC, FLAT_SCRATCH and XNACK_MASK (6 registers) on top of
         `next_free_sgpr`: at most 96 allocated, i.e. `next_free_sgpr` <= 90.  (Without the launch bound hipcc took 100 + 6 -> 112: seven waves.)
The test works the three quotients out from the descriptors and holds each to eight, for both variants (the HBM variant has no LDS to be a limit).
No scratch: the JSON string decoder keeps its state in registers; SGPRs the bound squeezes out go to VGPR lanes, which the VGPR figure includes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transferia_amd", "csrc")
SRC = os.path.join(CSRC, "tf_byids.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CU_LDS, CU_WAVES, WG_WAVES = 160 << 10, 32, 4


def lds_budget():
    with open(os.path.join(CSRC, "tf_byids.hpp")) as f:
        m = re.search(r"constexpr uint32_t BYIDS_LDS_BUDGET = (\d+)u << (\d+);", f.read())
    assert m, "BYIDS_LDS_BUDGET is not where the test reads it"
    return int(m.group(1)) << int(m.group(2))


@pytest.fixture(scope="module")
def kernels():
    asm = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", SRC], capture_output=True, text=True, timeout=900)
    assert asm.returncode == 0, asm.stderr[-2000:]
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.stdout, re.S):
        body = m.group(2)
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        out[m.group(1)] = {"vgpr": g("next_free_vgpr"), "sgpr": g("next_free_sgpr"), "vcc": g("reserve_vcc"), "scratch": g("private_segment_fixed_size"), "lds": g("group_segment_fixed_size")}
    return out


def waves_per_simd(k):
    """the waves of this kernel one SIMD holds, by each budget (gfx950: 512 VGPRs in blocks of 8, 800 SGPRs in blocks of 16 with 6 extra a wave, the
    CU's LDS over workgroups of four waves on four SIMDs; never more than 8)"""
    vgpr = 512 // (-(-k["vgpr"] // 8) * 8)
    sgpr = 800 // (-(-(k["sgpr"] + 6) // 16) * 16)
    lds = (CU_LDS // k["lds"]) * WG_WAVES // 4 if k["lds"] else 8
    return {"vgpr": min(vgpr, 8), "sgpr": min(sgpr, 8), "lds": min(lds, 8)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_byids_kernel_resources(kernels):
    budget = lds_budget()
    assert budget * (CU_WAVES // WG_WAVES) <= CU_LDS                  # the budget's own claim: eight workgroups a CU
    assert sorted(kernels) == sorted(k for k in kernels if "byids_keep_kernel" in k) and len(kernels) == 2, list(kernels)
    in_lds = [v for k, v in kernels.items() if "ILb1EE" in k]
    in_hbm = [v for k, v in kernels.items() if "ILb0EE" in k]
    assert len(in_lds) == 1 and len(in_hbm) == 1, list(kernels)
    for k in in_lds + in_hbm:
        assert k["scratch"] == 0 and k["vgpr"] <= 64 and k["sgpr"] <= 90 and k["vcc"] == 1, k
        assert waves_per_simd(k) == {"vgpr": 8, "sgpr": 8, "lds": 8}, (k, waves_per_simd(k))
    assert 0 < in_lds[0]["lds"] <= budget, in_lds[0]
    assert in_hbm[0]["lds"] <= 16, in_hbm[0]                          # (nothing but the unused one-word stand-in, if the compiler keeps it)
    # the arithmetic itself, on the figures hipcc gave this kernel before it was bound: 100 SGPRs -> 112 allocated -> seven waves
    assert waves_per_simd({"vgpr": 54, "sgpr": 100, "lds": 16384})["sgpr"] == 7

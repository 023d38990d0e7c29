"""Static guard on the protobuf parser's kernels (tf_protoparse.hip), by the method of tests/test_byids_resources.py: hipcc cross-compiles to gfx950 ISA
without a GPU, and the kernel descriptors say how many VGPRs and SGPRs, how much scratch and how much LDS each kernel takes.  Descriptors only: no
instruction is looked for.

DESIGN §3.19's occupancy argument: pp_decode is one lane per event and waits on memory most of the time, so what it needs is waves in flight, and what
would hurt it most is scratch — a spilled wire walk turns every field into extra memory round trips.  It must not spill, and its registers must allow
FOUR waves per SIMD (a CU's 16 waves = 1024 events in flight): at most 128 VGPRs a lane (512 per SIMD lane in blocks of 8) and, with the six registers
a wave is charged on top of `next_free_sgpr`, at most 200 SGPRs allocated (800 per SIMD in blocks of 16).  The framing walk (pp_frames) carries far
less state and holds eight waves.  No kernel of the file uses LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "transferia_amd", "csrc", "tf_protoparse.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels():
    asm = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", SRC], capture_output=True, text=True, timeout=900)
    assert asm.returncode == 0, asm.stderr[-2000:]
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.stdout, re.S):
        body = m.group(2)
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        out[m.group(1)] = {"vgpr": g("next_free_vgpr"), "sgpr": g("next_free_sgpr"), "scratch": g("private_segment_fixed_size"), "lds": g("group_segment_fixed_size")}
    return out


def waves_per_simd(k):
    """the waves of this kernel one SIMD holds, by each register budget (gfx950: 512 VGPRs in blocks of 8, 800 SGPRs in blocks of 16 with 6 extra a wave;
    never more than 8)"""
    return {"vgpr": min(512 // (-(-k["vgpr"] // 8) * 8), 8), "sgpr": min(800 // (-(-(k["sgpr"] + 6) // 16) * 16), 8)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_protoparse_kernel_resources(kernels):
    def one(part):
        hit = [v for k, v in kernels.items() if part in k]
        assert len(hit) == 1, (part, list(kernels))
        return hit[0]

    assert all(k["lds"] == 0 for k in kernels.values()), kernels
    decode = one("pp_decode")
    assert decode["scratch"] == 0, decode
    w = waves_per_simd(decode)
    assert w["vgpr"] >= 4 and w["sgpr"] >= 4, (decode, w)
    for part in ("pp_framesILb0", "pp_framesILb1"):
        k = one(part)
        assert k["scratch"] == 0 and waves_per_simd(k) == {"vgpr": 8, "sgpr": 8}, (part, k)
    for part in ("pp_check_batch", "pp_msg_final", "pp_keep", "pp_rows", "pp_text_copy", "pp_aux", "pp_const_text", "pp_cellsILb0ELb0"):   # the light kernels
        k = one(part)
        assert k["scratch"] == 0 and waves_per_simd(k) == {"vgpr": 8, "sgpr": 8}, (part, k)
    # the arithmetic itself: 101 VGPRs -> 104 allocated -> four waves; 100 SGPRs -> 112 allocated -> seven
    assert waves_per_simd({"vgpr": 101, "sgpr": 100}) == {"vgpr": 4, "sgpr": 7}

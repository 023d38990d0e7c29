"""Static guard on the native parser's kernels (tf_nativeparse.hip), by the method of tests/test_protoparse_resources.py: hipcc cross-compiles to gfx950
ISA without a GPU, and the kernel descriptors say how many VGPRs and SGPRs, how much scratch and how much LDS each kernel takes.  Descriptors only:
no instruction is looked for.

DESIGN §3.20 (the argument of §3.19): natp_header and natp_cells are one lane per item and wait on memory most of the time, so what they need is waves
in flight, and what would hurt them most is scratch.  Neither may spill, and both must allow FOUR waves per SIMD by both register budgets (at most
128 VGPRs a lane; at most 200 SGPRs allocated with the six a wave is charged on top of `next_free_sgpr`).  The cut carries a handful of 64-bit masks
and holds eight.  The `any` canonicaliser's container frames live in natp_any<*, true> alone, which is launched only when the batch has `any`
columns; natp_validate (the key-order check's per-depth spans) is not on the list of the issue's pinned kernels but is bounded here too.
No kernel of the file uses LDS (rocPRIM's sort kernels, instantiated in the same unit, are not ours)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "transferia_amd", "csrc", "tf_nativeparse.hip")
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
def test_nativeparse_kernel_resources(kernels):
    ours = {k: v for k, v in kernels.items() if "natp_" in k or "intern_" in k}

    def one(part):
        hit = [v for k, v in ours.items() if part in k]
        assert len(hit) == 1, (part, list(ours))
        return hit[0]

    assert all(k["lds"] == 0 for k in ours.values()), ours
    for part in ("natp_cutILb1", "natp_cutILb0"):
        k = one(part)
        assert k["scratch"] == 0 and waves_per_simd(k) == {"vgpr": 8, "sgpr": 8}, (part, k)
    for part in ("natp_header", "natp_cellsILb1", "natp_cellsILb0"):
        k = one(part)
        w = waves_per_simd(k)
        assert k["scratch"] == 0 and w["vgpr"] >= 4 and w["sgpr"] >= 4, (part, k, w)
    for part in ("natp_anyILb1ELb0", "natp_anyILb0ELb0", "natp_intern"):   # the `any` cells whose keys are in order, the grouping: no scratch either
        k = one(part)
        assert k["scratch"] == 0 and waves_per_simd(k)["vgpr"] >= 4, (part, k)
    for part in ("natp_anyILb1ELb1", "natp_anyILb0ELb1"):   # the sorting emitter's 16 frames
        assert one(part)["scratch"] <= 512, (part, one(part))
    assert one("natp_validate")["scratch"] <= 2048, one("natp_validate")   # any_keys_order: 2 x 128 words of key spans
    for part in ("natp_check_batch", "natp_tid_insert", "natp_tid_check", "natp_keep", "natp_sort_keys", "natp_rows", "intern_first", "intern_flag", "intern_ids", "intern_heads"):
        k = one(part)
        assert k["scratch"] == 0 and waves_per_simd(k) == {"vgpr": 8, "sgpr": 8}, (part, k)

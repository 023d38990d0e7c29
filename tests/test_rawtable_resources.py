"""Static guard on the raw_to_table kernels (tf_rawtable.hip), by the method of tests/test_kernel_resources.py: hipcc cross-compiles to gfx950 ISA
without a GPU, and the kernel descriptors say how many VGPRs and how much scratch each kernel takes.

The JSON scanner's container stacks and the sorting emitter's frames live only in the kernels a config with a JSON-typed key or value launches
(the third compiler trap): everything a string / bytes config runs takes no scratch at all.  The JSON kernels are held to what the Confluent
JSON parser's per-item kernels are held to (tests/test_kernel_resources.py) or take today: the check keeps per-depth key spans for the order check
(2 x 128 words, sr_parse_frames' bound of 2048 bytes and its 124 VGPRs); the `any` kernels every cell runs through are lean (no scratch, at most 96
VGPRs, sr_cell_values / sr_cell_text); the sorting variants have kernels of their own, at most sr_cell_text<true>'s 408 bytes of frames."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "transferia_amd", "csrc", "tf_rawtable.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels():
    asm = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", SRC], capture_output=True, text=True, timeout=900)
    assert asm.returncode == 0, asm.stderr[-2000:]
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.stdout, re.S):
        body = m.group(2)
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))  # noqa: E731
        out[m.group(1)] = {"vgpr": g("next_free_vgpr"), "scratch": g("private_segment_fixed_size"), "lds": g("group_segment_fixed_size")}
    return out


def find(table, fragment):
    hits = [v for k, v in table.items() if fragment in k]
    assert len(hits) == 1, (fragment, list(table))
    return hits[0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_rawtable_kernel_resources(kernels):
    assert all("rawtt_" in k for k in kernels), list(kernels)
    json_kernels = {k: v for k, v in kernels.items() if "rawtt_json_check" in k or "rawtt_any_" in k}
    assert len(json_kernels) == 5, list(json_kernels)
    # what a string / bytes config launches: no scratch, and light enough for eight waves per SIMD (64 VGPRs)
    for name, k in kernels.items():
        if name not in json_kernels:
            assert k["scratch"] == 0 and k["vgpr"] <= 64, (name, k)
    v = find(kernels, "rawtt_utf8_valid")
    assert v["lds"] == 0 and v["vgpr"] <= 48, v
    for small in ("rawtt_check_batch", "rawtt_split_flags", "rawtt_rows", "rawtt_fixed", "rawtt_validity", "rawtt_topic"):
        assert find(kernels, small)["vgpr"] <= 32, small
    for copy in (find(kernels, "rawtt_copy_cellsILi0EE"), find(kernels, "rawtt_copy_cellsILi1EE")):
        assert copy["lds"] <= 4096, copy   # the run's offsets: 257 + 256 words
    # the JSON kernels
    chk = find(kernels, "rawtt_json_check")
    assert chk["scratch"] <= 2048 and chk["vgpr"] <= 124 and chk["lds"] == 0, chk
    for lean in (find(kernels, "rawtt_any_lenILb0EE"), find(kernels, "rawtt_any_writeILb0EE")):
        assert lean["scratch"] == 0 and lean["vgpr"] <= 96 and lean["lds"] == 0, lean
    for canon in (find(kernels, "rawtt_any_lenILb1EE"), find(kernels, "rawtt_any_writeILb1EE")):
        assert 0 < canon["scratch"] <= 408 and canon["vgpr"] <= 96 and canon["lds"] == 0, canon

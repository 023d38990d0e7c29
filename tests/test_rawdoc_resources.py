"""Static guard on the raw_doc_grouper kernels (tf_rawdoc.hip), by the method of tests/test_kernel_resources.py: hipcc cross-compiles to gfx950 ISA
without a GPU, and the kernel descriptors say how many VGPRs and how much scratch each kernel takes.

The emitters are force-inlined and the sinks live in registers, as in the serializer (a sink passed by reference to a real call sits in scratch and every
put() becomes a load-modify-store there).  The `_rest` merge brings the JSON scanner with its container stack: it has kernels of its own, so a batch
without a `_rest` column does not pay for it (the third compiler trap)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "transferia_amd", "csrc", "tf_rawdoc.hip")
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
def test_rawdoc_kernel_resources(kernels):
    assert all("rawdoc_" in k for k in kernels), list(kernels)
    # Itanium mangling of the template flag: ILb0EE = without the `_rest` merge, ILb1EE = with it
    ln, wr = find(kernels, "rawdoc_lenILb0EE"), find(kernels, "rawdoc_writeILb0EE")
    assert ln["scratch"] == 0 and ln["lds"] == 0, ln
    # the bound the serializer's walks are held to: four waves per SIMD, at most the float formatter's digit buffer in scratch
    assert wr["scratch"] <= 64 and wr["vgpr"] <= 128 and wr["lds"] == 0, wr
    assert ln["vgpr"] <= 128, ln
    # the `_rest` variants are kernels of their own
    rl, rw = find(kernels, "rawdoc_lenILb1EE"), find(kernels, "rawdoc_writeILb1EE")
    assert rl is not ln and rw is not wr
    assert len([k for k in kernels if "rawdoc_len" in k]) == 2 and len([k for k in kernels if "rawdoc_write" in k]) == 2
    for small in ("rawdoc_commit_time", "rawdoc_kinds"):
        k = find(kernels, small)
        assert k["scratch"] == 0 and k["vgpr"] <= 32, (small, k)

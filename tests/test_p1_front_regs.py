"""Every instantiation of the pipelined code pass (k_chunk_codes_pipe,
csrc/phj_partition.h) that the library ships fits 16 waves per CU: at most 128
VGPRs and no scratch. The figures are the compiler's own, from the kernel
metadata of the device code compiled to gfx950 assembly (once per module);
nothing else of the assembly is read. CPU only: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "partitionedhashjoin_amd", "csrc", "phj_capi.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


def kernel_metadata(text):
    """{kernel name: {metadata key: value}} of the amdhsa.kernels list."""
    start = text.index("amdhsa.kernels:")
    end = text.index("amdhsa.target:", start)
    out = {}
    for entry in re.split(r"^  - (?=\.)", text[start:end], flags=re.M)[1:]:
        fields = dict(re.findall(r"^\s{2,4}(\.[a-z_]+):\s+(\S+)\s*$", "    " + entry, flags=re.M))
        out[fields[".name"]] = fields
    return out


@pytest.fixture(scope="module")
def pipe_kernels(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("p1_front") / "phj_device.s")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-S",
                    "--offload-device-only", "-I" + os.path.join(ROOT, "include"), SRC, "-o", asm],
                   check=True, capture_output=True, timeout=900)
    with open(asm) as f:
        meta = kernel_metadata(f.read())
    return {n: m for n, m in meta.items() if "k_chunk_codes_pipe" in n}


def test_every_form_is_compiled(pipe_kernels):
    # both hashes x (R's and S's plain forms, the pre-aggregating batched form, the column forms)
    assert len(pipe_kernels) >= 8, sorted(pipe_kernels)


def vgpr_budget(m):
    """512 VGPRs per SIMD lane over the waves per SIMD of one workgroup: 128 for
    the 1024-thread forms (16 waves per CU, every form the counting join runs).
    The 512-thread forms of the tuple-moving pass are launched one workgroup of
    8 waves per CU (two per SIMD, their amdgpu_waves_per_eu) and have always
    compiled to more than 128 (139 - 185 with DPT 2 and 4): their bound is
    that launch's, 256."""
    return 512 // (int(m[".max_flat_workgroup_size"]) // 256)


def test_vgprs_and_scratch(pipe_kernels):
    bad = {}
    for n, m in sorted(pipe_kernels.items()):
        vgprs, scratch, budget = int(m[".vgpr_count"]), int(m[".private_segment_fixed_size"]), vgpr_budget(m)
        print(n, vgprs, scratch, budget)
        if vgprs > budget or scratch != 0:
            bad[n] = (vgprs, scratch, budget)
    assert any(vgpr_budget(m) == 128 for m in pipe_kernels.values())
    assert not bad, bad

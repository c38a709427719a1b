"""Every form of the key index's lookup kernel (k_ix_lookup, csrc/phj_lookup.h:
rows from a plain index, codes from an ordinal index, rows from an ordinal
index) and the grouped accumulate (k_ix_accumulate, csrc/phj_ordinal.h) keeps
four waves per SIMD: at most 128 VGPRs and no scratch. The two forms that
existed before the ordinals (rows from a plain index, per hash) report the VGPR
count they reported then. The figures are the compiler's own, from the kernel
metadata of the device code compiled to gfx950 assembly (once per module);
nothing else of the assembly is read. CPU only: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess

import pytest

from test_p1_front_regs import HIPCC, ROOT, SRC, kernel_metadata

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

# k_ix_lookup<HK, STRIDE> of the commit before the ordinals ("S's pass 1: buffer
# key loads and a leaner batched front"), compiled with the same command: the
# .vgpr_count of its metadata, by hash (HK 0 = xxh3, 1 = murmur3), both strides
PARENT_VGPRS = {0: 99, 1: 97}
MODES = {0: "rows", 1: "codes", 2: "rows via first_rows"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("ordinal") / "phj_device.s")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-S",
                    "--offload-device-only", "-I" + os.path.join(ROOT, "include"), SRC, "-o", asm],
                   check=True, capture_output=True, timeout=900)
    with open(asm) as f:
        meta = kernel_metadata(f.read())
    return {n: m for n, m in meta.items() if "k_ix_lookup" in n or "k_ix_accumulate" in n}


def lookups(kernels):
    """{(hash, stride, mode): metadata} from the mangled template arguments."""
    out = {}
    for n, m in kernels.items():
        t = re.search(r"k_ix_lookupILi(\d)ELi(\d)ELNS_6IxModeE(\d)EEE", n)
        if t:
            out[tuple(int(x) for x in t.groups())] = m
    return out


def test_every_form_is_compiled(kernels):
    assert sorted(lookups(kernels)) == [(h, s, m) for h in (0, 1) for s in (1, 2) for m in MODES]
    assert len([n for n in kernels if "k_ix_accumulate" in n]) == 4, sorted(kernels)   # two hashes x two key strides


def test_vgprs_and_scratch(kernels):
    bad = {}
    for n, m in sorted(kernels.items()):
        vgprs, scratch = int(m[".vgpr_count"]), int(m[".private_segment_fixed_size"])
        print(n, vgprs, scratch, m.get(".group_segment_fixed_size"))
        if vgprs > 128 or scratch != 0 or int(m[".max_flat_workgroup_size"]) != 256:
            bad[n] = (vgprs, scratch)
    assert not bad, bad


def test_the_accumulate_cache_leaves_room_for_four_workgroups(kernels):
    for n, m in kernels.items():
        if "k_ix_accumulate" in n:
            assert int(m[".group_segment_fixed_size"]) * 4 <= 160 * 1024, (n, m[".group_segment_fixed_size"])


def test_the_plain_forms_kept_their_registers(kernels):
    for (h, s, mode), m in sorted(lookups(kernels).items()):
        if mode == 0:
            assert int(m[".vgpr_count"]) == PARENT_VGPRS[h], (h, s, m[".vgpr_count"])

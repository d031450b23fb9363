"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/triangulate.hip exist in the gfx950 code object and use the registers,
LDS and scratch DESIGN.md §4.8 states.  tri_kernel<true> carries the 4x4 Jacobi SVD per lane: it must keep it in registers (no scratch) and stay within 256 VGPRs
(two wavefronts per SIMD); a workgroup's LDS (the neighbour's node ids + the pair) must let several workgroups share a CU's 160 KB."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "triangulate.hip")
CU_LDS = 160 * 1024
# kernel: (VGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.8
STATED = {
    "_ZN6planar3tri10tri_kernelILb1EEEvNS0_4ArgsE": (191, 16556, 0),
    "_ZN6planar3tri10tri_kernelILb0EEEvNS0_4ArgsE": (78, 16556, 0),
    "_ZN6planar3tri18tri_compact_kernelENS0_4ArgsE": (32, 16, 0),
    "_ZN6planar3tri17tri_orient_kernelENS0_4ArgsE": (13, 136, 16),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("tri") / "triangulate.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        found[re.search(r"\.name:\s+(\S+)", b).group(1)] = (get("vgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return found


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, figures in STATED.items():
        assert kernels[name] == figures, name
    for token in ("191 VGPRs", "16 556 B", "78 VGPRs"):
        assert token in design, token


def test_search_kernels_keep_the_svd_in_registers_and_share_a_cu(kernels):
    for name, (vgpr, lds, scratch) in kernels.items():
        if "tri_kernel" in name:
            assert scratch == 0 and vgpr <= 256
        assert lds <= CU_LDS // 8, name      # eight workgroups' LDS per CU at the least

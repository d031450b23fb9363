"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/keyframe.hip exist in the gfx950 code object and use the registers, LDS
and scratch DESIGN.md §4.21 states.  None may use scratch, each stays within 128 VGPRs (two wavefronts per SIMD at the least), and a workgroup's LDS (the create
kernel's 2048 64-bit sort keys and its creator lists) stays at or below a sixth of a CU's 160 KB.  The figures are read from the code object's metadata only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "keyframe.hip")
CU_LDS = 160 * 1024
# kernel: (VGPRs, SGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.21
STATED = {
    "keyframe_need_kernel": (28, 65, 24, 0),
    "keyframe_register_kernel": (6, 16, 0, 0),
    "keyframe_create_kernel": (59, 106, 24856, 0),
    "keyframe_add_kernel": (32, 106, 24, 0),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("keyframe") / "keyframe.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+_ZN6planar8keyframe\d+([a-z_]+_kernel)", b)
        found[name.group(1)] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return found


def resources_bullet():
    """the Resources bullet of DESIGN.md §4.21, cut at the next bullet"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.21"):]
    section = section[:section.index("\n## ")]
    bullet = section[section.index("* **Resources**"):]
    return bullet[:bullet.index("\n* **")]


def stated_in_design(text, kernel):
    """(VGPRs, SGPRs, LDS bytes) the bullet states right after the kernel's name; 'no LDS' reads as 0"""
    tail = text[text.index("`" + kernel + "`") + len(kernel) + 2:]
    tail = tail[:tail.index(";")]
    vgpr = int(re.search(r"(\d+) VGPRs", tail).group(1))
    sgpr = int(re.search(r"(\d+) SGPRs", tail).group(1))
    lds = re.search(r"([\d ]+) B", tail)
    return vgpr, sgpr, 0 if "no LDS" in tail else int(lds.group(1).replace(" ", ""))


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    text = resources_bullet()
    assert "No kernel uses scratch" in text.replace("\n  ", " ")
    for name, figures in STATED.items():
        assert kernels[name] == figures, name
        assert stated_in_design(text, name) == kernels[name][:3], name


def test_no_scratch_128_vgprs_and_a_sixth_of_the_lds(kernels):
    for name, (vgpr, sgpr, lds, scratch) in kernels.items():
        assert scratch == 0, name
        assert vgpr <= 128, name
        assert lds <= CU_LDS // 6, name

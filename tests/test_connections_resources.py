"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/connections.hip exist in the gfx950 code object and use the registers, LDS
and scratch DESIGN.md §4.20 states.  None may use scratch, each stays within 128 VGPRs (two wavefronts per SIMD at the least), and a workgroup's LDS (the apply
kernel's row, rank table and 1024 64-bit sort keys) stays at or below a sixth of a CU's 160 KB.  The figures are read from the code object's metadata only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "connections.hip")
CU_LDS = 160 * 1024
# kernel: (VGPRs, SGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.20
STATED = {
    "connections_register_kernel": (8, 14, 0, 0),
    "connections_count_kernel": (9, 75, 8216, 0),
    "connections_apply_kernel": (50, 80, 16416, 0),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("connections") / "connections.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+_ZN6planar11connections\d+([a-z_]+_kernel)", b)
        found[name.group(1)] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return found


def resources_bullet():
    """the Resources bullet of DESIGN.md §4.20, cut at the next bullet"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.20"):]
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
        assert vgpr <= 128 and sgpr <= 102, name
        assert lds <= CU_LDS // 6, name

"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/newlines.hip exist in the gfx950 code object and use the registers, LDS and
scratch DESIGN.md §4.9 states.  None may use scratch, each stays within 256 VGPRs, and a workgroup's LDS (the neighbour's descriptors, the 257 counts, two poses)
stays at or below a sixteenth of a CU's 160 KB."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "newlines.hip")
CU_LDS = 160 * 1024
# kernel: (VGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.9
STATED = {
    "_ZN6planar2nl14nl_pair_kernelILi0EEEvNS0_4ArgsE": (30, 9360, 0),
    "_ZN6planar2nl14nl_pair_kernelILi1EEEvNS0_4ArgsE": (30, 9360, 0),
    "_ZN6planar2nl14nl_pair_kernelILi2EEEvNS0_4ArgsE": (66, 9360, 0),
    "_ZN6planar2nl17nl_compact_kernelENS0_4ArgsE": (30, 16, 0),
    "_ZN6planar2nl21nl_average_dir_kernelEPKiiPKdPKhPKfS2_S2_S8_NS0_6ScalesEPdPfSB_": (58, 0, 0),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("nl") / "newlines.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        found[re.search(r"\.name:\s+(\S+)", b).group(1)] = (get("vgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return found


def resources_bullet():
    """the Resources bullet of DESIGN.md §4.9, cut at the next bullet"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.9"):]
    section = section[:section.index("\n## ")]
    bullet = section[section.index("* **Resources**"):]
    return bullet[:bullet.index("\n* **")]


def stated_in_design(text, kernel):
    """(VGPRs, LDS bytes) the bullet states right after the kernel's name; 'no LDS' reads as 0"""
    tail = text[text.index(kernel) + len(kernel):]
    tail = tail[:tail.index(";")]
    vgpr = int(re.search(r"(\d+) VGPRs", tail).group(1))
    lds = re.search(r"([\d ]+) B", tail)
    return vgpr, 0 if "no LDS" in tail else int(lds.group(1).replace(" ", ""))


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    for name, figures in STATED.items():
        assert kernels[name] == figures, name
    text = resources_bullet()
    assert "No kernel\n  uses scratch" in text or "No kernel uses scratch" in text
    prose = {"`nl_pair_kernel<CREATE>`": "ILi2E", "`nl_pair_kernel<SEARCH_TRI>`": "ILi0E", "`nl_pair_kernel<SEARCH_DESC>`": "ILi1E", "`nl_compact_kernel`": "nl_compact_kernel",
             "`nl_average_dir_kernel`": "nl_average_dir_kernel"}
    for label, key in prose.items():
        name = [k for k in kernels if key in k]
        assert len(name) == 1, label
        assert stated_in_design(text, label) == kernels[name[0]][:2], label


def test_no_scratch_256_vgprs_and_a_sixteenth_of_the_lds(kernels):
    for name, (vgpr, lds, scratch) in kernels.items():
        assert scratch == 0, name
        assert vgpr <= 256, name
        assert lds <= CU_LDS // 16, name

"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/loopmatch.hip exist in the gfx950 code object and use the registers, LDS and
scratch DESIGN.md §4.12 states.  None may use scratch and each stays within 128 VGPRs (two wavefronts per SIMD at the least).  The two order-bound kernels take their
LDS dynamically: its size is a static_assert of the source, which this holds to the document as well, and the largest stays inside one CU's 160 KB."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "loopmatch.hip")
CU_LDS = 160 * 1024
# kernel: (VGPRs, SGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.12
STATED = {
    "bow_kf_kernel": (39, 86, 0, 0),
    "sim3_search_kernel": (68, 90, 27156, 0),
    "sim3_agree_kernel": (10, 27, 4, 0),
    "projection_scw_kernel": (82, 106, 0, 0),
    "fuse_scw_kernel": (72, 90, 43032, 0),
}
DYNAMIC = {"bow_kf_kernel": ("BowKfLds", 127656), "projection_scw_kernel": ("ChunkLds", 62120)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("loopmatch") / "loopmatch.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+_ZN6planar9loopmatch\d+([a-z_0-9]+_kernel)E", b).group(1)
        found[name] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return found


def resources_bullet():
    """the Resources bullet of DESIGN.md §4.12, cut at the next bullet"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.12"):]
    section = section[:section.index("\n## ")]
    bullet = section[section.index("* **Resources**"):]
    return bullet[:bullet.index("\n* **")]


def stated_in_design(text, kernel):
    """(VGPRs, SGPRs, static LDS bytes) the bullet states right after the kernel's name; 'no static LDS' reads as 0"""
    tail = text[text.index("`" + kernel + "`") + len(kernel) + 2:]
    tail = tail[:tail.index(";")]
    vgpr = int(re.search(r"(\d+) VGPRs", tail).group(1))
    sgpr = int(re.search(r"(\d+) SGPRs", tail).group(1))
    lds = re.search(r"SGPRs,\s+([\d ]+) B", tail)
    return vgpr, sgpr, 0 if "no static LDS" in tail else int(lds.group(1).replace(" ", ""))


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    text = resources_bullet()
    assert "No kernel uses scratch" in text.replace("\n  ", " ")
    for name, figures in STATED.items():
        assert kernels[name] == figures, name
        assert stated_in_design(text, name) == kernels[name][:3], name


def test_no_scratch_128_vgprs_and_the_lds_of_a_cu(kernels):
    for name, (vgpr, sgpr, lds, scratch) in kernels.items():
        assert scratch == 0, name
        assert vgpr <= 128 and sgpr <= 106, name
        assert lds + DYNAMIC.get(name, ("", 0))[1] <= CU_LDS, name


def test_dynamic_lds_is_what_the_source_asserts_and_the_document_states():
    src = open(SRC).read()
    text = resources_bullet().replace("\n  ", " ")
    for name, (struct, size) in DYNAMIC.items():
        assert f"static_assert(sizeof({struct}) == {size}," in src, name
        tail = text[text.index("`" + name + "`"):]
        tail = tail[:tail.index(";")]
        assert f"{size:,}".replace(",", " ") + " B dynamic" in tail, name

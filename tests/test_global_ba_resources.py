"""Build guard (no GPU needed: hipcc cross-compiles): the eleven kernels of planarslam_amd/csrc/gba.hip exist in the gfx950 code object, use no scratch and spill
neither VGPRs nor SGPRs, and their registers and LDS are what DESIGN.md §4.18 states; each LDS figure is a static_assert of the source and stays inside one CU's
160 KB.  Metadata only: the instructions are not read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "gba.hip")
CU_LDS = 160 * 1024
# (VGPRs: the unified file, architectural + accumulation registers; SGPRs; static LDS bytes; scratch bytes), the figures of DESIGN.md §4.18
STATED = {
    "gba_numjac": (98, 84, 0, 0),
    "gba_errors": (58, 80, 64, 0),
    "gba_linearize": (144, 34, 0, 0),
    "gba_gather": (64, 36, 0, 0),
    "gba_lambda": (14, 26, 32, 0),
    "gba_dinv": (50, 27, 0, 0),
    "gba_schur": (208, 36, 0, 0),
    "gba_factor": (140, 36, 73728, 0),
    "gba_solve": (82, 53, 32256, 0),
    "gba_update": (90, 62, 64, 0),
    "gba_decide": (30, 44, 64, 0),
}
LDS_STRUCT = {"gba_errors": "SumLds", "gba_update": "SumLds", "gba_decide": "SumLds", "gba_lambda": "MaxLds", "gba_factor": "FactorLds", "gba_solve": "SolveLds"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("gba") / "gba.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+_ZN6planar3gba\d+(gba_[a-z]+)E", b).group(1)
        found[name] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"))
    return found


def resources_bullet():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.18"):]
    section = section[:section.index("\n## ")]
    bullet = section[section.index("* **Resources**"):]
    return bullet[:bullet.index("\n* **")].replace("\n  ", " ")


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    text = resources_bullet()
    for name, figures in STATED.items():
        assert kernels[name][:4] == figures, name
        tail = text[text.index("`" + name + "`"):]
        assert f"{figures[0]} VGPRs" in tail and f"{figures[1]} SGPRs" in tail, name
        if figures[2]:
            assert f"{figures[2]:,}".replace(",", " ") + " B of LDS" in tail, name
    assert "no scratch" in text.lower()


def test_no_scratch_no_spill_and_the_lds_of_a_cu(kernels):
    for name, (vgpr, sgpr, lds, scratch, vspill, sspill) in kernels.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, name
        assert vgpr <= 512 and sgpr <= 106, name
        assert lds <= CU_LDS, name


def test_lds_is_what_the_source_asserts():
    src = open(SRC).read()
    for name, struct in LDS_STRUCT.items():
        assert f"static_assert(sizeof({struct}) == {STATED[name][2]}," in src, name
    for name in set(STATED) - set(LDS_STRUCT):
        assert STATED[name][2] == 0, name
    assert "static_assert(MAX_KF == PLANAR_GBA_MAX_KF && PLANAR_GBA_MAX_KF == PLANAR_ESSGRAPH_MAX_KF" in src

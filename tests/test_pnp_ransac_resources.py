"""Build guard (no GPU needed: hipcc cross-compiles): pnp_ransac_kernel of planarslam_amd/csrc/pnpransac.hip exists in the gfx950 code object, uses no scratch, and
its registers and LDS are what DESIGN.md §4.16 states; the LDS is a static_assert of the source and stays inside one CU's 160 KB.  The metadata
of the code object is all this reads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "pnpransac.hip")
CU_LDS = 160 * 1024
# (VGPRs: the unified file, architectural + accumulation registers; SGPRs; static LDS bytes; scratch bytes), the figures of DESIGN.md §4.16
STATED = {"pnp_ransac_kernel": (310, 106, 91864, 0)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("pnpransac") / "pnpransac.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+_ZN6planar4epnp\d+([a-z_0-9]+_kernel)E", b).group(1)
        found[name] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"))
    return found


def resources_bullet():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.16"):]
    section = section[:section.index("\n## ")]
    bullet = section[section.index("* **Resources**"):]
    return bullet[:bullet.index("\n* **")].replace("\n  ", " ")


def test_kernel_exists_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    text = resources_bullet()
    for name, figures in STATED.items():
        assert kernels[name][:4] == figures, name
        tail = text[text.index("`" + name + "`"):]
        assert f"{figures[0]} VGPRs" in tail and f"{figures[1]} SGPRs" in tail and f"{figures[2]:,}".replace(",", " ") + " B of LDS" in tail, name
    assert "no scratch" in text.lower()


def test_no_scratch_no_spilled_vgpr_and_the_lds_of_a_cu(kernels):
    for name, (vgpr, sgpr, lds, scratch, spilled) in kernels.items():
        assert scratch == 0 and spilled == 0, name
        assert vgpr <= 512 and sgpr <= 106, name
        assert lds <= CU_LDS, name


def test_lds_is_what_the_source_asserts():
    src = open(SRC).read()
    assert f"static_assert(sizeof(Lds) == {STATED['pnp_ransac_kernel'][2]}," in src

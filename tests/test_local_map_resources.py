"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/localmap.hip exist in the gfx950 code object and use the registers, LDS and
scratch DESIGN.md §4.19 states.  None may use scratch, each stays within 128 VGPRs (two wavefronts per SIMD at the least), and a workgroup's LDS (the key-frame
kernel's 1024 vote counters, rank table, list and marks) stays at or below a sixth of a CU's 160 KB."""
import pytest

from kernel_resources import CU_LDS, compiled_kernels, resources_bullet, stated_in_design

# kernel: (VGPRs, SGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.19
STATED = {
    "localmap_keyframes_kernel": (52, 96, 13348, 0),
    "localmap_mark_kernel": (12, 52, 0, 0),
    "localmap_count_kernel": (14, 50, 16, 0),
    "localmap_gather_kernel<0>": (50, 86, 16, 0),
    "localmap_gather_kernel<1>": (45, 84, 16, 0),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return compiled_kernels(tmp_path_factory, "localmap")


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    text = resources_bullet("4.19")
    assert "No kernel uses scratch" in text.replace("\n  ", " ")
    for name, figures in STATED.items():
        assert kernels[name] == figures, name
        assert stated_in_design(text, name) == kernels[name][:3], name


def test_no_scratch_128_vgprs_and_a_sixth_of_the_lds(kernels):
    for name, (vgpr, sgpr, lds, scratch) in kernels.items():
        assert scratch == 0, name
        assert vgpr <= 128 and sgpr <= 102, name
        assert lds <= CU_LDS // 6, name

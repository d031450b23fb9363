"""Build guard (no GPU needed: hipcc cross-compiles): the kernels of planarslam_amd/csrc/keyframe.hip exist in the gfx950 code object and use the registers, LDS
and scratch DESIGN.md §4.21 states.  None may use scratch, each stays within 128 VGPRs (two wavefronts per SIMD at the least), and a workgroup's LDS (the create
kernel's 2048 64-bit sort keys and its creator lists) stays at or below a sixth of a CU's 160 KB.  The figures are read from the code object's metadata only."""
import pytest

from kernel_resources import CU_LDS, compiled_kernels, resources_bullet, stated_in_design

# kernel: (VGPRs, SGPRs, static LDS bytes, scratch bytes), the figures of DESIGN.md §4.21
STATED = {
    "keyframe_need_kernel": (28, 65, 24, 0),
    "keyframe_register_kernel": (6, 16, 0, 0),
    "keyframe_create_kernel": (59, 106, 24856, 0),
    "keyframe_add_kernel": (32, 106, 24, 0),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return compiled_kernels(tmp_path_factory, "keyframe")


def test_kernels_exist_with_the_stated_resources(kernels):
    print(kernels)
    assert set(kernels) == set(STATED)
    text = resources_bullet("4.21")
    assert "No kernel uses scratch" in text.replace("\n  ", " ")
    for name, figures in STATED.items():
        assert kernels[name] == figures, name
        assert stated_in_design(text, name) == kernels[name][:3], name


def test_no_scratch_128_vgprs_and_a_sixth_of_the_lds(kernels):
    for name, (vgpr, sgpr, lds, scratch) in kernels.items():
        assert scratch == 0, name
        assert vgpr <= 128, name
        assert lds <= CU_LDS // 6, name

"""Build guard (no GPU needed: hipcc cross-compiles): the order-bound matchers of planarslam_amd/csrc/guided.hip, projection_kernel<MODE_FRAME / MODE_MAP / MODE_KF>
and bow_kernel (MODE_BOW has no projection_kernel instance: bow_kernel is it), in the gfx950 code object: no scratch, at most 128 VGPRs (two wavefronts per SIMD
at the least), and no more LDS than before the speculating resolver: the kernels take it dynamically, its size is a static_assert of the source, 62 120 B for
projection_kernel (two workgroups per 160 KB CU) and 127 656 B for bow_kernel, and there is no static LDS beside it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "planarslam_amd", "csrc", "guided.hip")
CU_LDS = 160 * 1024
# mangled-name fragment: (LDS struct, its size before the speculating resolver)
KERNELS = {"projection_kernelILi0E": ("ChunkLds", 62120), "projection_kernelILi1E": ("ChunkLds", 62120), "projection_kernelILi3E": ("ChunkLds", 62120),
           "bow_kernelE": ("BowLds", 127656)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("guided") / "guided.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only", SRC, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        for frag in KERNELS:
            if "6guided" in name and frag in name:
                found[frag] = (get("vgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return found


def test_no_scratch_and_at_most_128_vgprs(kernels):
    print(kernels)
    assert set(kernels) == set(KERNELS)
    for name, (vgpr, lds, scratch) in kernels.items():
        assert scratch == 0, name
        assert vgpr <= 128, name


def test_lds_is_at_most_what_it_was(kernels):
    src = open(SRC).read()
    for name, (struct, size) in KERNELS.items():
        assert kernels[name][1] == 0, name                                           # no static LDS beside the dynamic struct
        m = re.search(r"static_assert\(sizeof\(" + struct + r"\) == (\d+),", src)
        assert m and int(m.group(1)) <= size, name
        assert re.search(r"projection_kernel<MODE>, dim3\(a\.f\.B\), dim3\(NT\), sizeof\(ChunkLds\)", src) and "sizeof(guided::BowLds), ctx->stream" in src
    assert 2 * KERNELS["projection_kernelILi0E"][1] <= CU_LDS

"""What the build guards of the map stages share (test_local_map_resources.py, test_connections_resources.py, test_keyframe_resources.py): the kernels of one
planarslam_amd/csrc/*.hip compiled for gfx950 (hipcc cross-compiles: no GPU needed) with the figures of the code object's metadata, and the figures the Resources
bullet of a DESIGN.md section states.  The tables of expected figures and the assertions stay with each test."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CU_LDS = 160 * 1024


def compiled_kernels(tmp_path_factory, stem):
    """csrc/<stem>.hip, whose kernels live in namespace planar::<stem> -> {kernel (with <Z> for a template instance): (VGPRs, SGPRs, static LDS bytes, scratch bytes)}"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp(stem) / (stem + ".s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "planarslam_amd", "csrc", stem + ".hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for b in meta.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        name = re.search(r"\.name:\s+_ZN6planar%d%s\d+([a-z_]+_kernel)(ILi(\d)E)?" % (len(stem), stem), b)
        found[name.group(1) + (f"<{name.group(3)}>" if name.group(2) else "")] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"),
                                                                                   get("private_segment_fixed_size"))
    return found


def resources_bullet(section):
    """the Resources bullet of DESIGN.md §<section>, cut at the next bullet"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    text = design[design.index("### " + section + " "):]
    text = text[:text.index("\n## ")]
    bullet = text[text.index("* **Resources**"):]
    return bullet[:bullet.index("\n* **")]


def stated_in_design(text, kernel):
    """(VGPRs, SGPRs, LDS bytes) the bullet states right after the kernel's name; 'no LDS' reads as 0"""
    tail = text[text.index("`" + kernel + "`") + len(kernel) + 2:]
    tail = tail[:tail.index(";")]
    vgpr = int(re.search(r"(\d+) VGPRs", tail).group(1))
    sgpr = int(re.search(r"(\d+) SGPRs", tail).group(1))
    lds = re.search(r"([\d ]+) B", tail)
    return vgpr, sgpr, 0 if "no LDS" in tail else int(lds.group(1).replace(" ", ""))

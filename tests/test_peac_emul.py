"""The product's PEAC block kernel + clustering kernel (planarslam_amd/csrc/peac_common.h, peac_ahc2.h: the very source hipcc compiles for gfx950)
compiled with g++ and run on the host-side wave64 emulator (tests/host_shim/wave_emul.h), against the oracle's state after the first ahCluster
(orc_peac_cluster_state): every node's N / rid / mse / centre / normal / moments bit for bit, the extracted planes in order, the DisjointSet partition.
The emulator also fails the run when a cross-lane operation is reached by only part of a wavefront - the bug class a GPU run shows as garbage or a hang."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import peac_cases as pc
from planarslam_amd.synth import depth_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "host_shim")
SO = os.path.join(SHIM, "libpeac_emul_host.so")
K = (535.4, 539.2, 320.1, 247.6, 1.0 / 5000.0)


@pytest.fixture(scope="module")
def libs():
    src = os.path.join(SHIM, "peac_emul_host.cpp")
    csrc = os.path.join(ROOT, "planarslam_amd", "csrc")
    deps = [src, os.path.join(SHIM, "wave_emul.h")] + [os.path.join(csrc, f) for f in ("peac_ahc2.h", "peac_common.h", "peac_eig.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", SO, src])
    E = C.CDLL(SO)
    import oracle_lib as ol
    O = ol.lib() if hasattr(ol, "lib") else C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    vp = C.c_void_p
    E.peac_emul_cluster.argtypes = [vp, C.c_int, C.c_int] + [C.c_float] * 5 + [C.c_int] + [vp] * 7 + [C.c_int]
    O.orc_peac_cluster_state.argtypes = [vp, C.c_int, C.c_int] + [C.c_float] * 5 + [vp, C.c_int, vp, vp, vp, vp]
    O.orc_peac_cluster_state.restype = C.c_int
    return E, O


def _cluster(E, d, mode):
    """the emulated kernels on one frame, nothing checked but that the emulator ran: (nodes, hand, dsp, dss, nouse, stats) as peac_emul_cluster leaves them"""
    H, W = d.shape
    NB, NB2 = C.c_int(), C.c_int()
    E.peac_emul_dims(W, H, C.byref(NB), C.byref(NB2))
    NB, NB2 = NB.value, NB2.value
    nodes = np.zeros((NB2, 18)); hand = np.zeros(132, np.int32); dsp = np.zeros(NB, np.uint16); dss = np.zeros(NB, np.uint16)
    nouse = np.zeros((NB2 + 31) // 32, np.uint32); st = np.zeros(8, np.int64)
    err = C.create_string_buffer(512)
    d = np.ascontiguousarray(d, np.uint16)
    rc = E.peac_emul_cluster(d.ctypes.data, W, H, *K, mode, nodes.ctypes.data, hand.ctypes.data, dsp.ctypes.data, dss.ctypes.data, nouse.ctypes.data, st.ctypes.data, err, 512)
    assert rc == 0, err.value.decode()
    return nodes, hand, dsp, dss, nouse, st


def _run(libs, d, mode=0):
    E, O = libs
    H, W = d.shape
    nodes, hand, dsp, dss, nouse, st = _cluster(E, d, mode)
    NB, NB2 = len(dsp), len(nodes)
    onodes = np.zeros((NB2, 18)); oext = np.zeros(4096, np.int32); onext = C.c_int(); oroot = np.zeros(NB, np.int32); osize = np.zeros(NB, np.int32)
    n = O.orc_peac_cluster_state(d.ctypes.data, W, H, *K, onodes.ctypes.data, NB2, oext.ctypes.data, C.byref(onext), oroot.ctypes.data, osize.ctypes.data)
    assert st[0] == 0 and hand[1] == 0, f"kernel status {st[0]} / {hand[1]}"
    assert hand[2] == n, f"nodes: kernel {hand[2]}, oracle {n}"
    live = onodes[:n, 0] > 0                      # blocks that never held a plane: the oracle keeps NaN there, the kernel zeros
    same = (nodes[:n].view(np.uint64) == onodes[:n].view(np.uint64)).all(1) | ~live
    assert same.all(), f"first differing node {int(np.argmin(same))}: kernel {nodes[np.argmin(same)]} oracle {onodes[np.argmin(same)]}"
    assert hand[0] == onext.value and np.array_equal(hand[4:4 + hand[0]], oext[:onext.value]), "extracted planes differ"

    def find(x):
        while dsp[x] != x:
            x = dsp[x]
        return x
    roots = np.array([find(b) for b in range(NB)])
    assert np.array_equal(roots, oroot) and np.array_equal(dss[roots], osize), "DisjointSet partition differs"
    dead = np.array([(nouse[i >> 5] >> (i & 31)) & 1 for i in range(n)], bool)
    assert dead[live].all(), "a node of the graph is still marked alive after the clustering"
    return dict(retried=bool(st[4]), phases=int(st[2] >> 40), evaluated=int((st[2] >> 20) & 0xFFFFF), hits=int(st[2] & 0xFFFFF), big=int(st[3]), big_solves=int(st[5]), nodes=int(n), planes=int(hand[0]),
                sites=int(st[6]))


@pytest.mark.parametrize("w,h,seed,noise,holes", [(160, 120, 5, True, True), (320, 240, 77, True, True), (320, 240, 78, False, True), (640, 480, 4321, True, True),
                                                  (640, 480, 51, False, False)])
def test_emulated_kernel_matches_oracle(libs, w, h, seed, noise, holes):
    d = depth_image(seed, w, h, noise=noise, holes=holes)
    info = _run(libs, d)                                  # the library's flow: fast kernel (tournament queue), exact kernel if it gave up
    assert info["nodes"] > (w // 10) * (h // 10)          # something was merged
    if w <= 320:
        _run(libs, d, mode=1)                             # the exact-heap kernel alone


def test_frame_with_more_than_4096_blocks(libs):
    """960x540 = 5 184 blocks: more than 8 192 node ids, so the tournament queue's columns hold more than two ids per lane (col_recompute_large) and the clustering
    kernel's LDS grows with the block count (reference: any size, src/PlaneExtractor.cpp:59, include/peac/AHCPlaneFitter.hpp:225); the cameras' intrinsics scale with it"""
    d = depth_image(4321, 960, 540, noise=True, holes=True)
    info = _run(libs, d, mode=2)                          # the fast kernel on its own
    assert info["nodes"] > 5184 and not info["retried"]
    # noise-free: exact ties (the exact heap redoes the frame) and unions over more than 6 144 node ids (the union bitmap is walked 192 words at a time); every pruned
    # evaluation of a pooled bag checked against evaluating all its candidates
    d = depth_image(4321, 960, 540, noise=False, holes=True)
    info = _run(libs, d, mode=4)
    assert info["retried"] and info["big"] > 50


def test_fast_kernel_alone_handles_generic_frames(libs):
    """noisy depth has no bit-equal mse values: the fast kernel must finish on its own (mode 2 does not fall back)"""
    for seed in (5, 6, 7):
        info = _run(libs, depth_image(seed, 320, 240), mode=2)
        assert not info["retried"]


def test_emulated_kernel_edge_cases(libs):
    z = np.zeros((120, 160), np.uint16)
    assert _run(libs, z)["planes"] == 0                   # no valid block at all
    flat = np.full((240, 320), 10000, np.uint16)
    info = _run(libs, flat)                               # one fronto-parallel wall: exact mse ties all over the heap, one region with a long boundary
    assert info["planes"] == 1 and info["retried"]        # bit-equal keys: the fast kernel hands the frame to the exact one
    ramp = (6000 + 9 * np.arange(320)[None, :] + np.zeros((240, 1))).astype(np.uint16)
    assert _run(libs, ramp)["planes"] == 1


def test_big_bags_go_through_the_pool(libs):
    """a noise-free scene grows regions with more than 64 neighbours: the bags in the pool, their compaction and slot reuse are exercised"""
    info = _run(libs, depth_image(51, 640, 480, noise=False, holes=False))
    assert info["big"] > 0


@pytest.mark.parametrize("seed,noise", [(51, False), (4336, True), (4346, True)])
def test_pruned_evaluation_of_big_bags_agrees_with_evaluating_everything(libs, seed, noise):
    """eval_big solves only the candidates whose lower bound does not rule them out; with mode | 4 the emulated kernel also evaluates ALL candidates
    in order after every pruned evaluation and reports status 9 on any difference (best neighbour, mse, flags)"""
    info = _run(libs, depth_image(seed, 640, 480, noise=noise, holes=noise), mode=4)
    assert info["big"] > 0
    if noise:                                                         # the point of pruning: about one solve per node instead of one per 64 neighbours
        fast = _run(libs, depth_image(seed, 640, 480, noise=noise, holes=noise), mode=2)
        assert fast["big_solves"] < 1.5 * fast["big"], fast


# where the fast kernel gave up (stats [6], bits of PEAC_NOTE_RETRY in peac_ahc2.h).  The non-finite-key site of pq_push is not reachable from a depth
# image, so nothing here aims at it: a merged node is pushed only after its mse passed `mse < T_mse_merge(z)`, which NaN and +inf fail, and -inf would need
# the moment sums (finite coordinates of at most W*H pixels) to overflow.
SITE_QUEUE_TIE, SITE_POOLED_TIE = 1, 4


@pytest.mark.parametrize("w,h", [(320, 240), (640, 480)])
@pytest.mark.parametrize("name", sorted(pc.EDGE_RETRIED))
def test_which_edge_frames_the_fast_kernel_hands_over(libs, name, w, h):
    """the edge frames the GPU tests mix into their batches: the ones with bit-equal block mse (one wall, walls at constant depths) are handed to the
    exact kernel, at the queue; the others are finished by the fast kernel (and all of them equal the oracle, _run)"""
    info = _run(libs, pc.edge_frames(w, h)[name])
    assert info["retried"] == pc.EDGE_RETRIED[name], info
    assert info["sites"] == (SITE_QUEUE_TIE if pc.EDGE_RETRIED[name] else 0), info


@pytest.mark.parametrize("i", range(len(pc.POOLED_TIE_320)))
def test_a_tie_inside_a_pooled_bag_hands_the_frame_over(libs, i):
    """eval_big: two candidates of a pooled bag with bit-equal merged mse; the fast kernel's bag order is not the reference's, so it gives the frame to
    the exact kernel - there and nowhere else on these frames"""
    info = _run(libs, pc.pooled_tie(i))
    assert info["retried"] and info["big"] > 0 and info["sites"] == SITE_POOLED_TIE, info


def test_more_than_max_planes_is_a_reported_status(libs):
    """1280x720, 144 separated tilted patches of 3 600+ px: the reference extracts them all, the kernel holds MAX_PLANES = 128 and ends the clustering
    with status 4 (planar_peac_check turns it into PLANAR_ECAPACITY)"""
    import oracle_lib as ol
    E, _ = libs
    d = pc.many_planes()
    op, _ = ol.peac_run(d, max_planes=256)
    assert len(op) == 144
    _, hand, _, _, _, st = _cluster(E, d, 0)
    assert st[0] == 4 and hand[1] == 4 and hand[0] == 128 and not st[4], (st, hand[:4])

"""CPU: the edge-selection rules of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2743-2866) as the product states them over plain arrays, in C++
(planar_adapter::essential_graph_edges of include/planar_adapters.hpp, compiled with g++ into tests/adapter_shim/adapter_essential_graph_main.cpp) and in Python
(planarslam_amd.essgraph.essential_graph_edges), on a hand-built graph of 7 key frames that reaches every rule.  The expected list is written out below with the
reference line that decides each entry.  No key frame object and no device."""
import subprocess

import numpy as np
import pytest

import adapter_build as AB

L, N = 0, 1                                    # PLANAR_ESSGRAPH_LOOP, PLANAR_ESSGRAPH_NORMAL
CUR, LOOP = 6, 1
PARENT = [-1, 0, 1, 2, 3, 4, 5]                # a chain: the spanning tree
LOOP_EDGES = [[5], [], [], [], [], [0], []]    # an old loop closure between 0 and 5, held by both
COVISIBLE = [                                  # (index, weight) in GetVectorCovisibleKeyFrames() order
    [], [], [(4, 150), (0, 105)], [], [(2, 150)],
    [(6, 300), (0, 200), (3, 110), (1, 130)],
    [(5, 300), (2, 150), (4, 120), (3, 99), (0, 100)],
]
LOOP_CONNECTIONS = {4: [(1, 30)], 5: [(1, 120)], 6: [(1, 0), (2, 150), (3, 50)]}
EXPECTED = [
    # loop connections (:2748-2774), key frames in mnId order
    #   (4, 1) weight 30: not the (current, loop) pair and below minFeat, dropped although its far end is the loop key frame (:2757)
    (5, 1, L),    # weight 120 >= minFeat (:2757)
    (6, 1, L),    # weight 0, but nIDi == pCurKF->mnId && nIDj == pLoopKF->mnId: the exemption (:2757)
    (6, 2, L),    # weight 150
    #   (6, 3) weight 50: from the current key frame but not to the loop key frame, dropped (:2757)
    # normal edges (:2777-2866), key frame by key frame: spanning tree, loop edges, covisibility
    #   key frame 0: no parent; its loop edge 5 has the higher id (:2818)
    (1, 0, N),    # spanning tree (:2792)
    (2, 1, N),    # spanning tree
    #   (2, 4) weight 150: pKFn->mnId < pKF->mnId fails, key frame 4 adds the pair (:2842)
    (2, 0, N),    # covisibility, weight 105
    (3, 2, N),    # spanning tree
    (4, 3, N),    # spanning tree
    (4, 2, N),    # covisibility, weight 150, from the higher id
    (5, 4, N),    # spanning tree
    (5, 0, N),    # old loop edge towards the lower id (:2818)
    #   (5, 6) weight 300: hasChild (:2841);  (5, 0) weight 200: sLoopEdges.count (:2841)
    (5, 3, N),    # covisibility, weight 110
    #   (5, 1) weight 130: in sInsertedEdges since the loop connection (5, 1) (:2843)
    (6, 5, N),    # spanning tree: the parent needs no weight
    #   (6, 5) weight 300: pKFn != pParentKF fails (:2841);  (6, 2) weight 150: in sInsertedEdges (:2843)
    (6, 4, N),    # covisibility, weight 120
    #   (6, 3) weight 99: below minFeat, GetCovisiblesByWeight(100) does not return it (:2839)
    (6, 0, N),    # covisibility, weight 100 = minFeat
]


def test_python_rules():
    from planarslam_amd.essgraph import essential_graph_edges
    e = essential_graph_edges(PARENT, LOOP_EDGES, COVISIBLE, LOOP_CONNECTIONS, CUR, LOOP)
    assert e.dtype == np.int32 and [tuple(r) for r in e.tolist()] == EXPECTED


def test_cpp_rules(tmp_path):
    exe = str(tmp_path / "adapter_essential_graph")
    subprocess.check_call(AB.build_command(exe, [AB.shim_source("adapter_essential_graph_main.cpp")], algebra=True, shim="first", standins="opt"))
    rows = [f"{len(PARENT)} {CUR} {LOOP}", " ".join(map(str, PARENT))]
    rows += [" ".join([str(len(l))] + [f"{j} 0" for j in l]) for l in LOOP_EDGES]
    rows += [" ".join([str(len(l))] + [f"{j} {w}" for j, w in l]) for l in COVISIBLE]
    rows += [" ".join([str(len(LOOP_CONNECTIONS.get(i, [])))] + [f"{j} {w}" for j, w in LOOP_CONNECTIONS.get(i, [])]) for i in range(len(PARENT))]
    p = tmp_path / "graph.txt"
    p.write_text("\n".join(rows) + "\n")
    out = subprocess.check_output([exe, "edges", str(p)], text=True)
    assert [tuple(int(x) for x in line.split()) for line in out.splitlines()] == EXPECTED


def test_every_rule_is_reached():
    kinds = {k for _, _, k in EXPECTED}
    assert kinds == {L, N} and len(EXPECTED) == 15
    assert all(v1 < v0 for v0, v1, k in EXPECTED if k == N)                  # normal edges run from the higher id to the lower

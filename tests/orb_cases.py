"""Frames and extractor parameters shared by the CPU and GPU tests of the ORB extractor (planarslam_amd/csrc/orb.hip): one table of named cases over the
geometry and parameter space that planar_orb_create accepts - wide frames (more than one initial octree node), the packing and capacity limits, pyramid
depths, thresholds and feature budgets.  Every case carries a self-check: assertions on oracle-side facts which prove that the case still reaches the path
it exists for (tests/test_oracle_orb.py runs them, so a change to synth.gray_image cannot quietly empty a case)."""
import functools
from typing import Callable, NamedTuple

import numpy as np

from planarslam_amd.synth import gray_image

DEFAULTS = dict(nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7)
EDGE = 16                   # EDGE_THRESHOLD - 3: the FAST border of a level
CELL = 30


def noisy(seed, w, h, a):
    """gray_image(seed, w, h) plus uniform integer noise in [-a, a], clipped to u8"""
    rng = np.random.default_rng(seed)
    return np.clip(gray_image(seed, w, h).astype(np.int32) + rng.integers(-a, a + 1, (h, w)), 0, 255).astype(np.uint8)


def uniform(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def lowcontrast_half():
    img = noisy(10, 640, 480, 12).astype(np.int32)
    img[:, :320] = 100 + (img[:, :320] - 100) // 3
    return img.astype(np.uint8)


def checkerboard(w=400, h=304, px=9):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // px) + (xx // px)) & 1) * 255).astype(np.uint8)


# ---- the plan's geometry of one pyramid level (planar_orb_create), from the level's size -------------------------------------------------------------
class Cell(NamedTuple):
    x0: int
    y0: int
    ww: int
    wh: int
    slot_cap: int
    tstride: int


class LevelGeom(NamedTuple):
    w: int
    h: int
    nfeat: int
    nIni: int
    depth: int
    code_bits: int
    kept_cap: int
    nCols: int
    nRows: int
    wCell: int
    hCell: int
    cells: tuple


def level_geometry(w, h, nfeat):
    width, height = w - 2 * EDGE, h - 2 * EDGE
    nCols, nRows = width // CELL, height // CELL
    wCell, hCell = -(-width // nCols), -(-height // nRows)
    nIni = int(np.floor(width / height + 0.5))
    depth = 1
    while (1 << (depth - 1)) < max(width, height):
        depth += 1
    ini_bits = 0
    while (1 << ini_bits) < nIni:
        ini_bits += 1
    code_bits = (2 * depth + ini_bits + 3) & ~3
    cells = []
    maxBX, maxBY = w - EDGE, h - EDGE
    for i in range(nRows):
        iniY = EDGE + i * hCell
        if iniY >= maxBY - 3:
            continue
        maxY = min(iniY + hCell + 6, maxBY)
        for j in range(nCols):
            iniX = EDGE + j * wCell
            if iniX >= maxBX - 6:
                continue
            maxX = min(iniX + wCell + 6, maxBX)
            x0, y0 = iniX + 3, iniY + 3
            ww, wh = maxX - 3 - x0, maxY - 3 - y0
            if ww <= 0 or wh <= 0:
                continue
            cells.append(Cell(x0, y0, ww, wh, ((ww + 1) // 2) * ((wh + 1) // 2), (((x0 - 3) & 3) + ww + 6 + 3) & ~3))
    return LevelGeom(w, h, nfeat, nIni, depth, code_bits, max(nfeat + 4, 4 * nIni + 4), nCols, nRows, wCell, hCell, tuple(cells))


# ---- oracle-side facts of a case ---------------------------------------------------------------------------------------------------------------------
class Facts(NamedTuple):
    image: np.ndarray
    kps: np.ndarray
    desc: np.ndarray
    levels: tuple           # the pyramid
    blurred: tuple          # per level: the blurred clone, or None where the level kept no keypoint
    cand: tuple             # per level: (n, 3) x, y (relative to the FAST border), score, in the reference's emission order
    geom: tuple             # LevelGeom per level

    @property
    def per_level(self):
        return [int((self.kps["octave"] == l).sum()) for l in range(len(self.levels))]

    @property
    def ncand(self):
        return [len(c) for c in self.cand]

    def cell_counts(self, l):
        """candidates per FAST cell of level l, keyed by (row, column)"""
        g, c = self.geom[l], self.cand[l]
        rows, cols = (c[:, 1] - 3) // g.hCell, (c[:, 0] - 3) // g.wCell
        out = {}
        for r, q in zip(rows.tolist(), cols.tolist()):
            out[(r, q)] = out.get((r, q), 0) + 1
        return out


def _frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


def oracle_facts(image, params):
    import oracle_lib as ol
    o = ol.OrbOracle(**params)
    kps, desc = o.extract(image)
    n = params["nlevels"]
    levels = tuple(_frozen(o.level(l)) for l in range(n))
    nfeat = o.features_per_level()
    return Facts(_frozen(image), _frozen(kps), _frozen(desc), levels, tuple(_frozen(o.blurred(l)) for l in range(n)),
                 tuple(_frozen(o.candidates(l)) for l in range(n)), tuple(level_geometry(lv.shape[1], lv.shape[0], nfeat[l]) for l, lv in enumerate(levels)))


# ---- self-checks -------------------------------------------------------------------------------------------------------------------------------------
def _nini(f):
    return [g.nIni for g in f.geom]


def _chk_hd_720p(f):
    assert _nini(f) == [2] * 8 and [g.code_bits for g in f.geom[:2]] == [28, 28]
    assert len(f.kps) == 1008


def _chk_wvga_noise(f):
    assert _nini(f) == [2] * 8
    for l, g in enumerate(f.geom):          # worst-case density, and still inside every cell's slot array
        by_cell = {((c.y0 - 3 - EDGE) // g.hCell, (c.x0 - 3 - EDGE) // g.wCell): c for c in g.cells}
        counts = f.cell_counts(l)
        assert counts and all(n <= by_cell[k].slot_cap for k, n in counts.items())
    assert f.ncand[0] > 10 * f.geom[0].nfeat


def _chk_wide_960x320(f):
    assert _nini(f) == [3, 3, 3, 3, 4, 4, 4, 4]
    g = f.geom[7]
    assert (g.w, g.h) == (268, 89) and (g.wCell, g.hCell) == (34, 57)


def _chk_portrait(f):
    assert _nini(f) == [1] * 8 and all(g.h > g.w for g in f.geom)


def _chk_strip(f):
    assert _nini(f) == [21, 22] and [g.code_bits for g in f.geom] == [32, 32]
    assert len(f.kps) == 802


def _chk_strip_few(f):
    assert [g.nfeat for g in f.geom] == [16, 14] and _nini(f) == [21, 22]
    assert f.per_level == [84, 88] == [4 * g.nIni for g in f.geom]          # every initial node split once, whatever N is
    assert [g.kept_cap for g in f.geom] == [88, 92]


def _chk_wide_one_feature(f):
    assert [g.nfeat for g in f.geom] == [4, 4, 3, 3, 2, 2, 1, 1]
    assert f.per_level == [12, 12, 12, 12, 16, 16, 16, 15]


def _chk_max_width(f):
    assert _nini(f) == [42] and f.geom[0].code_bits == 32
    assert len(f.kps) == 1502 and f.kps["x"].max() > 4000


def _chk_one_level(f):
    assert len(f.levels) == 1 and f.geom[0].nfeat == 300 and len(f.kps) > 0


def _chk_twelve_levels(f):
    assert len(f.levels) == 12 and all(n > 0 for n in f.per_level)
    assert all(0 < a.shape[1] - b.shape[1] <= 60 for a, b in zip(f.levels, f.levels[1:]))      # ratio near 1: neighbouring levels a few dozen columns apart


def _chk_scale2(f):
    g = f.geom[2]
    assert (g.w, g.h) == (160, 120) and g.code_bits == 16 and (g.wCell, g.hCell) == (32, 44)
    assert [lv.shape for lv in f.levels] == [(480, 640), (240, 320), (120, 160)]


def _chk_ini_equals_min(f):
    assert len(f.kps) > 0 and all(c[:, 2].min() >= 12 for c in f.cand if len(c))


def _chk_high_thresholds(f):
    assert len(f.kps) == 491
    assert sum(p == n for p, n in zip(f.per_level, f.ncand)) == 7 and all(c[:, 2].min() >= 60 for c in f.cand if len(c))


def _chk_ini_254_min_1(f):
    assert f.ncand[0] == 9808
    assert all(c[:, 2].max() < 254 for c in f.cand)          # no cell reaches ini: all of them fall back to min = 1


def _chk_lowcontrast_half(f):
    g, c = f.geom[0], f.cand[0]
    cell = ((c[:, 1] - 3) // g.hCell) * g.nCols + (c[:, 0] - 3) // g.wCell
    kinds = set()
    for k in np.unique(cell):
        s = c[cell == k, 2]
        assert s.min() >= 20 or s.max() < 20                # a cell is at the initial threshold or fell back to the minimum as a whole
        kinds.add(bool(s.min() >= 20))
    assert kinds == {True, False}                           # both kinds of cell in one level
    assert len(np.unique(cell)) < len(g.cells)              # and cells without any corner (the compressed half)


def _chk_few_features(f):
    assert [g.nfeat for g in f.geom] == [9, 7, 6, 5, 4, 3, 3, 3]
    assert f.per_level[0] == 10 and f.per_level[-1] == 4     # a level stops at the first round that reaches its share
    assert all(n > 10 * g.nfeat for n, g in zip(f.ncand, f.geom))


def _chk_more_than_exist(f):
    assert len(f.kps) == 1151 == sum(f.ncand) and max(g.nfeat for g in f.geom) == 1303
    assert all(n < g.nfeat for n, g in zip(f.ncand, f.geom))


def checker_tie_count(f):
    """keypoints whose response another keypoint has as well"""
    return len(f.kps) - len(np.unique(f.kps["response"]))


def _chk_checker_ties(f):
    assert f.ncand[0] == 0 and f.per_level[0] == 0 and all(n > 0 for n in f.per_level[1:])
    assert checker_tie_count(f) == 655
    # equal responses inside one level's CANDIDATES too: the arg-max of a node and the radix sort's stable order decide between them
    assert max(int(np.unique(c[:, 2], return_counts=True)[1].max()) for c in f.cand[1:]) >= 20


def _chk_small_64(f):
    g = f.geom[0]
    assert (g.w, g.h, g.nCols, g.nRows, len(g.cells)) == (64, 64, 1, 1, 1) and f.ncand[0] > 0


def _chk_small_100x80(f):
    g = f.geom[1]
    assert (g.w, g.h) == (83, 67) and (g.wCell, g.hCell, len(g.cells)) == (51, 35, 1) and f.ncand[1] > 0


def _chk_big_cells_91(f):
    g = f.geom[0]
    assert len(g.cells) == 1 and (g.cells[0].ww, g.cells[0].wh) == (53, 53) and g.cells[0].ww * g.cells[0].wh == 2809
    assert g.cells[0].tstride == 60                         # 15 of the tile's 16 words per row
    assert f.ncand[0] > 256                                 # more survivors than one round of 256 threads: the corner list loops


def _chk_big_cells_105x104(f):
    g = f.geom[1]
    assert (g.wCell, g.hCell, len(g.cells)) == (56, 55, 1) and f.ncand[1] > 0


class Case(NamedTuple):
    name: str
    image: Callable[[], np.ndarray]
    params: dict
    check: Callable[[Facts], None]


def _p(nfeatures=1000, scale=1.2, nlevels=8, ini=20, mn=7):
    return dict(nfeatures=nfeatures, scale=scale, nlevels=nlevels, ini=ini, mn=mn)


_strip = lambda: noisy(15, 2049, 129, 30)      # noqa: E731
CASES = [
    Case("hd_720p", lambda: noisy(1, 1280, 720, 25), _p(), _chk_hd_720p),
    Case("wvga_noise", lambda: uniform(848, 848, 480), _p(), _chk_wvga_noise),
    Case("wide_960x320", lambda: noisy(2, 960, 320, 25), _p(), _chk_wide_960x320),
    Case("portrait_480x640", lambda: noisy(3, 480, 640, 25), _p(), _chk_portrait),
    Case("strip_2049x129", _strip, _p(800, 1.2, 2), _chk_strip),
    Case("strip_fewer_than_ini", _strip, _p(30, 1.2, 2), _chk_strip_few),
    Case("wide_one_feature_levels", lambda: noisy(15, 960, 320, 30), _p(20, 1.2, 8), _chk_wide_one_feature),
    Case("max_width_4096x128", lambda: noisy(16, 4096, 128, 30), _p(1500, 1.2, 1), _chk_max_width),
    Case("one_level", lambda: noisy(5, 333, 257, 25), _p(300, 1.2, 1), _chk_one_level),
    Case("twelve_levels_1p1", lambda: noisy(6, 640, 480, 25), _p(1000, 1.1, 12), _chk_twelve_levels),
    Case("scale2_three_levels", lambda: noisy(7, 640, 480, 25), _p(600, 2.0, 3), _chk_scale2),
    Case("ini_equals_min", lambda: noisy(8, 400, 304, 25), _p(1000, 1.2, 8, 12, 12), _chk_ini_equals_min),
    Case("high_thresholds", lambda: noisy(9, 400, 304, 40), _p(1000, 1.2, 8, 120, 60), _chk_high_thresholds),
    Case("ini_254_min_1", lambda: noisy(18, 400, 304, 25), _p(1000, 1.2, 8, 254, 1), _chk_ini_254_min_1),
    Case("lowcontrast_half", lowcontrast_half, _p(), _chk_lowcontrast_half),
    Case("few_features", lambda: noisy(11, 640, 480, 25), _p(40), _chk_few_features),
    Case("more_than_exist", lambda: gray_image(12, 400, 304), _p(6000), _chk_more_than_exist),
    Case("checker_ties", checkerboard, _p(), _chk_checker_ties),
    Case("small_64", lambda: noisy(13, 64, 64, 40), _p(100, 1.2, 1), _chk_small_64),
    Case("small_100x80", lambda: noisy(14, 100, 80, 40), _p(100, 1.2, 2), _chk_small_100x80),
    Case("big_cells_91", lambda: uniform(5, 91, 91), _p(500, 1.2, 1, 5, 1), _chk_big_cells_91),
    Case("big_cells_105x104", lambda: uniform(105, 105, 104), _p(500, 1.2, 2), _chk_big_cells_105x104),
]
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
# the cases whose reference-made outputs are committed (tests/golden/orb_<key>.npz, tools/gen_golden_orb.py): more than one initial node, 32 code bits, 4 nIni kept
GOLDEN = dict(wide960="wide_960x320", strip2049="strip_2049x129", strip_few="strip_fewer_than_ini")


@functools.lru_cache(maxsize=None)
def facts(name):
    """the oracle's outputs of a case, computed once per process; the arrays are read-only"""
    c = BY_NAME[name]
    return oracle_facts(c.image(), c.params)

"""normals_kernel's schedule (planarslam_amd/csrc/normals.hip): the integral images are formed in bands of 10 rows, each band as a skewed wavefront of 60 chain
lanes, and the chamfer passes carry the neighbouring row in LDS.  Only which lane forms a cell, and when, differs from the row-by-row form - so every bit must
equal the oracle at the sizes where the schedule takes another path: fewer rows than four bands and a partial last band, a skew longer than a row, rows wider
than the workgroup, and the default frame with step edges into every border and with no depth at all."""
import functools

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

RB = 10                                    # rows of a band (normals.hip)
NT = 256


def _plane(w, h, a, b, z0, step=None):
    """a tilted wall z0 + a x + b y metres; `step` = (r0, r1, c0, c1, dz) lifts a rectangle towards the camera"""
    yy, xx = np.mgrid[0:h, 0:w]
    z = z0 + a * xx + b * yy
    if step is not None:
        r0, r1, c0, c1, dz = step
        z[r0:r1, c0:c1] -= dz
    return np.rint(z * 5000).astype(np.uint16)


# name -> (W, H, the rectangle of frame 1)
SMALL = {
    "96x96": (96, 96, (48, 54, 66, 96, 0.5)),              # grid 32 x 32: three full bands and one of two rows
    "100x190": (100, 190, (95, 104, 50, 100, 0.5)),        # grid 34 x 64: taller than wide, the last band has four rows; a band's 10-step skew against 34 columns
    "1000x99": (1000, 99, (49, 58, 500, 1000, 0.5)),       # grid 334 x 33: rows wider than the workgroup (a second trip), a last band of three rows
}


@functools.lru_cache(maxsize=None)
def small_frames(name):
    w, h, step = SMALL[name]
    d = np.stack([_plane(w, h, 0.002, 0.001, 1.5), _plane(w, h, -0.001, 0.003, 2.0, step)])
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def small_oracle(name):
    out = [O.surface_normals(d) for d in small_frames(name)]
    for pair in out:
        for a in pair:
            a.setflags(write=False)
    return out


def _step_edges_640():
    """tests/normals_cases.step_edges at 640 x 480: bands into the top / bottom and left / right borders, patches on the last grid row and column"""
    h, w = 480, 640
    yy, xx = np.mgrid[0:h, 0:w]
    z = 2.0 + 0.0015 * xx + 0.001 * yy
    z[:, 300:380] -= 0.6
    z[200:260, :] -= 0.9
    z[h - 3:, 400:520] -= 0.5
    z[80:160, w - 1:] -= 0.5
    return np.rint(z * 5000).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def default_frames():
    d = np.stack([_plane(640, 480, 0.0012, 0.0007, 1.8), _step_edges_640(), np.zeros((480, 640), np.uint16)])
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def default_oracle():
    d = default_frames()
    return [O.surface_normals(d[0]), O.surface_normals(d[1], want_dist=True), O.surface_normals(d[2])]


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def _differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


@pytest.mark.parametrize("name", list(SMALL))
def test_normals_small_and_lopsided_grids(ctx, name):
    from planarslam_amd.planes import SurfaceNormals
    w, h, _ = SMALL[name]
    gw, gh = -(-w // 3), -(-h // 3)
    if name == "96x96":
        assert (gw, gh) == (32, 32) and gh < 4 * RB and gh % RB != 0
    if name == "100x190":
        assert (gw, gh) == (34, 64) and gh > gw and gh % RB != 0
    if name == "1000x99":
        assert (gw, gh) == (334, 33) and gw > NT and gh % RB != 0
    d = small_frames(name)
    assert not np.array_equal(d[0], d[1])
    want = small_oracle(name)
    for b, (rn, _) in enumerate(want):                      # at most (gh - 20) / 2 x (gw - 20) / 2 cells lie inside the 10-cell border: counts, not a fraction
        finite = ~np.isnan(rn[:, 0])
        assert finite.sum() >= 20 and (~finite).sum() >= 1, f"{name} frame {b}: {int(finite.sum())} finite normals of {len(rn)}"
    inside = (gh - 20) // 2 * ((gw - 20) // 2)
    assert (~np.isnan(want[1][0][:, 0])).sum() < inside, "the step edge of frame 1 removes no normal inside the border"
    sn = SurfaceNormals(w, h, 2, ctx)
    assert sn.count == (gw // 2) * (gh // 2)
    nrm, pts = sn.compute(d)
    for b, (rn, rp) in enumerate(want):
        assert _same(nrm[b], rn), f"{name} frame {b}: {_differing(nrm[b], rn)} of {len(rn)} normals differ from the oracle"
        np.testing.assert_array_equal(pts[b], rp)


def test_normals_default_frame_smooth_edges_and_no_depth(ctx):
    from planarslam_amd.planes import SurfaceNormals
    d = default_frames()
    (n0, p0), (n1, p1, dist), (n2, p2) = default_oracle()
    assert (~np.isnan(n0[:, 0])).sum() == 70 * 97                                 # smooth: every cell inside the border
    assert (dist[0] == 0).any() and (dist[-1] == 0).any() and (dist[:, 0] == 0).any() and (dist[:, -1] == 0).any()
    f1 = float((~np.isnan(n1[:, 0])).mean())
    assert 0.20 < f1 < 0.95, f1
    assert np.isnan(n2).all()
    nrm, pts = SurfaceNormals(640, 480, 3, ctx).compute(d)
    for b, (rn, rp) in enumerate(((n0, p0), (n1, p1), (n2, p2))):
        assert _same(nrm[b], rn), f"frame {b}: {_differing(nrm[b], rn)} of {len(rn)} normals differ from the oracle"
        np.testing.assert_array_equal(pts[b], rp)

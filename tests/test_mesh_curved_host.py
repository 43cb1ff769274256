"""
Curved boundaries on the host (`device=None`): refinement and P2 / P4 enrichment onto ellipses (include/fep.h,
fep_mesh_set_curves; midpoints.py implements the same rule in NumPy).  No GPU.

The small meshes and the assertions are curved_cases.py's.  The tunnel figures (area deficit of the wall polygon against the
ellipse pi a b per level: 1.0687e-2, 2.6787e-3, 6.7025e-4, 1.6768e-4) follow from the geometry: an inscribed polygon whose
sides are halved loses a quarter of its deficit, to O(h^2) — hence the ratio bounds [3.9, 4.1].
"""
import numpy as np
import pytest

import curved_cases as cc
from conftest import load_golden

DEFICIT = (1.0687e-2, 2.6787e-3, 6.7025e-4, 1.6768e-4)


@pytest.fixture(scope='module')
def all_cases(fep):
    return cc.cases(fep)


@pytest.mark.parametrize('name', cc.CASE_NAMES)
def test_small_meshes(fep, all_cases, name):
    cc.check_curved(fep, name, *all_cases[name], device=None)


def test_edge_through_the_centre_keeps_its_midpoint(fep, all_cases):
    coord, elem, curves = all_cases['edge through the centre'][:3]
    c, e = fep.refine_uniform(coord, elem, curves=curves)
    h = fep.create_midpoints_P2(coord, elem, curves=curves)
    k = int(np.flatnonzero((h['surf'][0] == 0) & (h['surf'][1] == 2))[0])      # the edge (1, 0) -> (-1, 0)
    m = int(h['surf'][2, k])
    assert h['surf_curve'][k] == 0 and np.array_equal(h['coord_ext'][:, m], [0.0, 0.0]) and np.array_equal(c[:, m], [0.0, 0.0])
    assert np.isfinite(c).all() and np.isfinite(fep.create_midpoints_P4(coord, elem, curves=curves)['coord_ext']).all()
    r = np.hypot(*h['coord_ext'][:, 3:])
    assert np.sum(np.abs(r - 1) < 1e-15) == 2                                 # the other two midpoints are on the circle


def test_square_diagonal_stays_straight(fep, all_cases):
    coord, elem, curves = all_cases['unit square in its circle'][:3]
    h = fep.create_midpoints_P2(coord, elem, curves=curves)
    h4 = fep.create_midpoints_P4(coord, elem, curves=curves)
    h0 = fep.create_midpoints_P4(coord, elem)
    assert (h['coord_ext'][:, 4:] == 0.5).all(axis=0).sum() == 1               # the diagonal's midpoint: the circle's centre
    assert list(h['surf_curve']) == [0, 0, 0, 0]
    on_diagonal = np.flatnonzero(np.isclose(h0['coord_ext'][0], h0['coord_ext'][1]))
    assert on_diagonal.size >= 5 and np.array_equal(h4['coord_ext'][:, on_diagonal], h0['coord_ext'][:, on_diagonal])


def test_ring_edges_go_to_their_own_curve(fep, all_cases):
    coord, elem, curves = all_cases['ring with one sector missing'][:3]
    h = fep.create_midpoints_P2(coord, elem, curves=curves)
    B, A = h['surf'][:2].astype(int)
    sc = h['surf_curve']
    assert np.array_equal(sc[(A < 6) & (B < 6)], [0] * 5) and np.array_equal(sc[(A >= 6) & (B >= 6)], [1] * 5)
    assert np.array_equal(sc[(A < 6) != (B < 6)], [-1, -1])                    # ends on different curves: straight


def test_bad_curves_are_refused(fep, all_cases):
    coord, elem, curves = all_cases['one triangle in the unit circle'][:3]
    E = fep.Ellipse
    for bad in ([E(0, 0, 1, 1)] * 5, [E(0, 0, 0, 1)], [E(0, 0, 1, -1)], [E(0, 0, 1, 1, -1e-3)], [E(np.nan, 0, 1, 1)],
                [E(0, 0, np.inf, 1)], [E(0, 0, 1, 1, np.inf)]):
        for call in (lambda: fep.create_midpoints_P2(coord, elem, curves=bad), lambda: fep.create_midpoints_P4(coord, elem, curves=bad),
                     lambda: fep.refine_uniform(coord, elem, curves=bad)):
            with pytest.raises(ValueError):
                call()
    assert fep.Ellipse(1, 2, 3, 4).tol == 1e-3 and fep.tsx_tunnel.TSX_HOLE == (0.0, 0.0, 2.1875, 1.75, 1e-3)
    assert 'surf_curve' in fep.create_midpoints_P2(coord, elem, curves=[E(0, 0, 1, 1)] * 4)


# ---- the tunnel ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tunnel_levels(fep):
    """[(coord, elem)] of levels 0..3 with TSX_HOLE, chained, and level 3 without curves."""
    g = load_golden('tsx')
    lv = [(g['coord'], g['elem'])]
    for _ in range(3):
        lv.append(fep.refine_uniform(*lv[-1], curves=[fep.tsx_tunnel.TSX_HOLE]))
    return lv, fep.refine_uniform(g['coord'], g['elem'], levels=3)


def test_tunnel_three_levels(fep, tunnel_levels):
    H = fep.tsx_tunnel.TSX_HOLE
    levels, straight3 = tunnel_levels
    ellipse = np.pi * H.a * H.b
    deficit = []
    for lv, (c, e) in enumerate(levels):
        d = cc.triangle_area(c, e)
        assert d.min() > 0, lv
        a, b = cc.wall_edges(c, e, H)
        assert a.size == 25 * 2 ** lv
        hole = cc.polygon_area(c, a, b)
        assert abs(d.sum() / 2 + hole - 1e4) <= 1e-12 * 1e4, lv
        deficit.append(1 - hole / ellipse)
        assert abs(deficit[-1] / DEFICIT[lv] - 1) <= 1e-3, (lv, deficit[-1])       # the recorded figures, to their digits
    print('deficit per level', deficit)
    for lv in range(3):
        assert 3.9 <= deficit[lv] / deficit[lv + 1] <= 4.1, (lv, deficit)
    # without curves the wall stays the 25-gon (its new nodes sit on the chords, up to 0.8 % inside the ellipse): its area is
    # the same sum up to rounding
    a, b = cc.wall_edges(*straight3, H._replace(tol=0.02))
    assert a.size == 200
    assert abs((1 - cc.polygon_area(straight3[0], a, b) / ellipse) - deficit[0]) <= 1e-12
    chained = fep.refine_uniform(*levels[0], levels=3, curves=[H])
    assert np.array_equal(chained[0], levels[3][0]) and np.array_equal(chained[1], levels[3][1])
    c, e = fep.prepare_tsx_mesh(*levels[0], 'P1', refine=3, curves=[H])[:2]
    assert np.array_equal(c, levels[3][0]) and np.array_equal(e, levels[3][1])


def _wall_rows(h, t):
    s = h['surf'][:, h['surf_curve'] >= 0].astype(np.int64)
    B, A = s[0], s[1]
    return np.stack([A, s[2], B]) if t == 'P2' else np.stack([A, s[3], s[2], s[4], B])


def test_tunnel_quadratic_wall_area(fep, tunnel_levels):
    """P2 at level 0: the area inside the quadratic wall (3-point Gauss per edge: the integrand is a cubic) misses the
    ellipse by 9.3e-6 of it; the polygon misses it by 1.07e-2."""
    H = fep.tsx_tunnel.TSX_HOLE
    coord, elem = tunnel_levels[0][0]
    h = fep.create_midpoints_P2(coord, elem, curves=[H])
    assert int((h['surf_curve'] >= 0).sum()) == 25
    miss = abs(1 - cc.curved_loop_area(h['coord_ext'], _wall_rows(h, 'P2'), 3) / (np.pi * H.a * H.b))
    print('P2 wall area misses the ellipse by', miss)
    assert miss < 1e-4
    h0 = fep.create_midpoints_P2(coord, elem)
    h0['surf_curve'] = h['surf_curve']
    assert abs(1 - cc.curved_loop_area(h0['coord_ext'], _wall_rows(h0, 'P2'), 3) / (np.pi * H.a * H.b)) > 1e-2


def test_load_and_prepare_pass_curves_on(fep, tsx_csv_dir, tunnel_levels):
    H = fep.tsx_tunnel.TSX_HOLE
    coord, elem = tunnel_levels[0][0]
    for t in ('P2', 'P4'):
        h = fep.create_midpoints(t, coord, elem, curves=[H])
        c, e = fep.load_tsx_mesh(tsx_csv_dir, t, curves=[H])
        assert np.array_equal(c, h['coord_ext']) and np.array_equal(e, h['elem_ext'])
        c1, e1 = fep.load_tsx_mesh(tsx_csv_dir, t, refine=1, curves=[H])
        h1 = fep.create_midpoints(t, *tunnel_levels[0][1], curves=[H])
        assert np.array_equal(c1, h1['coord_ext']) and np.array_equal(e1, h1['elem_ext'])
    g = load_golden('tsx')
    c, e = fep.load_tsx_mesh(tsx_csv_dir, 'P2', curves=None)
    assert np.array_equal(c, g['p2_coord']) and np.array_equal(e, g['p2_elem'])


# ---- area statistics -------------------------------------------------------------------------------------------------------
def test_area_stats_host_form(fep, tunnel_levels):
    c, e = tunnel_levels[0][2]
    d = cc.triangle_area(c, e)
    st = fep.area_stats(c, e)
    assert st.dtype == np.float64 and st[0] == d.min() and st[2] == 0 and st[3] == e.shape[1]
    assert abs(st[1] - d.sum() / 2) <= e.shape[1] * cc.U * np.abs(d / 2).sum()
    e2 = e.copy()
    e2[[1, 2], 5] = e2[[2, 1], 5]
    st = fep.area_stats(c, e2)
    assert st[2] == 1 and st[0] == -d[5]


def test_refine_refuses_a_folded_child(fep):
    coord, elem, curves = cc.over_curved(fep)
    c, e = fep.refine_uniform(coord, elem)                                      # fine without the curve
    assert cc.triangle_area(c, e).min() > 0
    with pytest.raises(ValueError, match=r'level 1: 3 of 4 triangles'):
        fep.refine_uniform(coord, elem, curves=curves)
    with pytest.raises(ValueError, match=r'level 1: 3 of 4 triangles'):
        fep.refine_uniform(coord, elem, levels=3, curves=curves)
    h = fep.create_midpoints_P2(coord, elem, curves=curves)                      # the enrichment itself does not judge
    assert list(h['surf_curve']).count(0) == 1

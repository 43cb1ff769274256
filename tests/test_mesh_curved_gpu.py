"""
Curved boundaries on the GPU: fep_mesh_set_curves / fep_mesh_surf_curve_* / fep_mesh_area_stats_* and everything above them,
against the host forms (test_mesh_curved_host.py holds those to the rule itself) and, for the curved P2 / P4 tunnel, against
the float64 element reference at test_element_route_gpu.py's bounds.

Device against host: the rule is the same operations in the same order, and square root and division are correctly rounded
on both sides; one differing rounding would show as 4 u (|c| + max(a, b)) per component.  On the MI355X every case of this
module came out bit-equal, so the comparisons are np.array_equal.
"""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import curved_cases as cc
from conftest import load_golden, relerr
from test_element_route_gpu import _run_case

pytestmark = pytest.mark.gpu

DEV = 0


@pytest.fixture(scope='module')
def all_cases(fep):
    return cc.cases(fep)


@pytest.fixture(scope='module')
def tunnel():
    g = load_golden('tsx')
    return g['coord'], g['elem']


@pytest.mark.parametrize('name', cc.CASE_NAMES)
def test_small_meshes(fep, all_cases, name):
    coord, elem, curves = all_cases[name][:3]
    dev = cc.check_curved(fep, name, *all_cases[name], device=DEV)
    again = {op: cc.run(fep, op, coord, elem, DEV, curves=curves) for op in cc.OPS}
    for op in cc.OPS:
        cc.same_bytes(again[op], dev[op], (name, op, 'second call'))
    host = {op: cc.run(fep, op, coord, elem, None, curves=curves) for op in cc.OPS}
    worst = max(np.abs(dev[op]['coord_ext'] - host[op]['coord_ext']).max() for op in cc.OPS)
    print(f'[device - host] {name}: {worst:.3e}')
    cc.compare_device_host(name, dev, host)


def test_device_mesh_curves_and_surf_curve(fep, all_cases):
    coord, elem, curves = all_cases['ring with one sector missing'][:3]
    for t in ('P2', 'P4'):
        h = fep.create_midpoints(t, coord, elem, curves=curves)
        with fep.DeviceMesh(coord, elem, DEV) as m:
            assert m.n_curves == 0 and (m.surf_curve(t) == -1).all() and 'surf_curve' not in m.enrich(t)
            m.set_curves(curves)
            assert m.n_curves == 2
            assert np.array_equal(m.surf_curve(t), h['surf_curve']) and m.surf_curve(t).dtype == np.int64
            sd = m.surf_curve_dev(t)
            assert sd.dtype.itemsize == 4 and np.array_equal(sd.cpu().numpy(), h['surf_curve'])
            out = [a.cpu().numpy() for a in m.enrich_dev(t)]
            assert np.array_equal(out[0], h['elem_ext']) and np.array_equal(out[2], h['surf'])
            assert np.array_equal(out[1], h['coord_ext'])
            m.set_curves(curves[1:])                                           # the outer ellipse alone is now curve 0
            assert sorted(set(m.surf_curve(t))) == [-1, 0] and (m.surf_curve(t) == 0).sum() == 5
            m.set_curves(None)
            cc.same_bytes(m.enrich(t), fep.create_midpoints(t, coord, elem, device=DEV), t)


def test_refusals_return_their_codes(fep, all_cases):
    lib_mod = import_module('fem-elastoplasticity_amd._lib')
    l = fep.lib()
    coord, elem, curves = all_cases['one triangle in the unit circle'][:3]
    good = np.array([[0.0, 0.0, 1.0, 1.0, 1e-9]])
    plain = fep.create_midpoints_P2(coord, elem, device=DEV)
    want = fep.create_midpoints_P2(coord, elem, device=DEV, curves=curves)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        assert l.fep_mesh_set_curves(m._h, 1, lib_mod.ptr(good)) == 0
        bad_rows = []
        for col, v in ((2, 0.0), (2, -1.0), (3, 0.0), (3, -2.0), (4, -1e-3)):
            r = good.copy()
            r[0, col] = v
            bad_rows.append(r)
        for col in range(5):
            for v in (np.nan, np.inf, -np.inf):
                r = good.copy()
                r[0, col] = v
                bad_rows.append(r)
        for r in bad_rows:
            assert l.fep_mesh_set_curves(m._h, 1, lib_mod.ptr(r)) == -1, r
        five = np.repeat(good, 5, axis=0)
        assert l.fep_mesh_set_curves(m._h, 5, lib_mod.ptr(five)) == -1 and l.fep_mesh_set_curves(m._h, -1, lib_mod.ptr(five)) == -1
        assert l.fep_mesh_set_curves(m._h, 1, None) == -1 and l.fep_mesh_set_curves(None, 0, None) == -1
        assert l.fep_mesh_set_curves(m._h, 4, lib_mod.ptr(five)) == 0 and l.fep_mesh_set_curves(m._h, 1, lib_mod.ptr(good)) == 0
        got = dict(m.enrich('P2'), surf_curve=m.surf_curve('P2'))                # (set through C: the Python object adds no key)
        cc.same_bytes(got, want, 'the curves of the last valid call hold')       # a refused call changed nothing
        sc = np.full(3, -7, dtype=np.int32)
        assert l.fep_mesh_surf_curve_host(m._h, 1, lib_mod.ptr(sc)) == -1 and l.fep_mesh_surf_curve_host(m._h, 2, None) == -1
        assert l.fep_mesh_surf_curve_host(None, 2, lib_mod.ptr(sc)) == -1 and (sc == -7).all()
        assert l.fep_mesh_set_curves(m._h, 0, None) == 0
        cc.same_bytes(m.enrich('P2'), plain, 'n = 0 clears the curves')
    out = np.zeros(4)
    e32, c64 = np.ascontiguousarray(elem, dtype=np.int32), np.ascontiguousarray(coord)
    assert l.fep_mesh_area_stats_host(DEV, 1, 3, None, lib_mod.ptr(c64), lib_mod.ptr(out)) == -1
    assert l.fep_mesh_area_stats_host(DEV, 1, 3, lib_mod.ptr(e32), lib_mod.ptr(c64), None) == -1
    assert l.fep_mesh_area_stats_host(DEV, -1, 3, lib_mod.ptr(e32), lib_mod.ptr(c64), lib_mod.ptr(out)) == -1
    assert l.fep_mesh_area_stats_dev(DEV, None, 1, 3, None, None, None) == -1
    with pytest.raises(ValueError):
        fep.create_midpoints_P2(coord, elem, device=DEV, curves=[fep.Ellipse(0, 0, -1, 1)])
    assert l.fep_mesh_area_stats_host(DEV, 1, 3, lib_mod.ptr(e32), lib_mod.ptr(c64), lib_mod.ptr(out)) == 0 and out[2] == 0
    cc.same_bytes(fep.create_midpoints_P2(coord, elem, device=DEV, curves=curves), want, 'a valid call afterwards')


# ---- area statistics -------------------------------------------------------------------------------------------------------
def _check_stats(st, coord, elem):
    d = cc.triangle_area(coord, elem)
    assert st[0] == d.min() and st[2] == np.count_nonzero(d <= 0) and st[3] == elem.shape[1]
    assert abs(st[1] - d.sum() / 2) <= elem.shape[1] * cc.U * np.abs(d / 2).sum()


@pytest.mark.parametrize('levels', [0, 2, 5])
def test_area_stats_agree_with_numpy(fep, tunnel, levels):
    """887 elements: four workgroups; level 2 (14 192): 56; level 5 (908 288): the 1024-workgroup cap, so the grid-stride loop
    runs more than once per lane.  A handful of elements turned over on purpose: count and minimum are exact."""
    import torch
    coord, elem = fep.refine_uniform(*tunnel, levels=levels, device=DEV) if levels else tunnel
    elem = np.array(elem, copy=True)
    flip = np.random.default_rng(levels).choice(elem.shape[1], 7, replace=False)
    elem[1, flip], elem[2, flip] = elem[2, flip].copy(), elem[1, flip].copy()
    st = fep.area_stats(coord, elem, device=DEV)
    assert st[2] == 7
    _check_stats(st, coord, elem)
    c_d = torch.from_numpy(np.ascontiguousarray(coord)).to(f'cuda:{DEV}')
    e_d = torch.from_numpy(elem.astype(np.int32)).to(f'cuda:{DEV}')
    a = fep.area_stats_dev(c_d, e_d, DEV).cpu().numpy()
    b = fep.area_stats_dev(c_d, e_d, DEV).cpu().numpy()
    assert a.tobytes() == b.tobytes() == st.tobytes()
    bad = elem.astype(np.int32)
    bad[2, 3] = coord.shape[1]                                                  # out of range: reads nothing, counts as d = 0
    d = np.delete(cc.triangle_area(coord, elem), 3)
    st = fep.area_stats(coord, bad, device=DEV)
    assert st[2] == np.count_nonzero(d <= 0) + 1 and st[0] == d.min()


def test_area_stats_report_the_folded_children(fep):
    coord, elem, curves = cc.over_curved(fep)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        m.set_curves(curves)
        c, e = m.refine()
    st = fep.area_stats(c, e, device=DEV)
    assert st[2] == 3 and st[0] < 0 and st[3] == 4
    _check_stats(st, c, e)
    for levels in (1, 3):
        with pytest.raises(ValueError, match=r'level 1: 3 of 4 triangles'):
            fep.refine_uniform(coord, elem, levels=levels, device=DEV, curves=curves)
    c0, e0 = fep.refine_uniform(coord, elem, device=DEV)
    assert cc.triangle_area(c0, e0).min() > 0


# ---- the tunnel ------------------------------------------------------------------------------------------------------------
def test_tunnel_three_chained_levels_equal_the_host_levels(fep, tunnel):
    H = fep.tsx_tunnel.TSX_HOLE
    c, e = fep.refine_uniform(*tunnel, levels=3, device=DEV, curves=[H])
    ch, eh = fep.refine_uniform(*tunnel, levels=3, curves=[H])
    assert np.array_equal(e, eh) and e.dtype == eh.dtype and c.shape == ch.shape
    print('[device - host] tunnel, three levels:', np.abs(c - ch).max())
    assert np.array_equal(c, ch)
    d = cc.triangle_area(c, e)
    assert d.min() > 0
    a, b = cc.wall_edges(c, e, H)
    assert a.size == 200 and abs(d.sum() / 2 + cc.polygon_area(c, a, b) - 1e4) <= 1e-12 * 1e4
    c2, e2 = fep.refine_uniform(*tunnel, levels=3, device=DEV, curves=[H])
    assert c2.tobytes() == c.tobytes() and e2.tobytes() == e.tobytes()


def _wall_rows(h, t):
    s = h['surf'][:, h['surf_curve'] >= 0].astype(np.int64)
    B, A = s[0], s[1]
    return np.stack([A, s[2], B]) if t == 'P2' else np.stack([A, s[3], s[2], s[4], B])


@pytest.mark.parametrize('t', ['P2', 'P4'])
def test_curved_tunnel_context(fep, monkeypatch, capfd, tunnel, t):
    """The curved P2 / P4 tunnel mesh as a context: positive determinants, the weights sum to the square minus the area inside
    the polynomial wall (Gauss on each edge, exact for its integrand: degree 3 for P2, 7 for P4), and one plastic step's K
    and F against the element reference.  The step runs on the mesh mapped to [0, 10]^2 — test_element_route_gpu.py's state
    is made for that square — which keeps every element's shape."""
    H = fep.tsx_tunnel.TSX_HOLE
    h = fep.create_midpoints(t, *tunnel, device=DEV, curves=[H])
    coord, elem = h['coord_ext'], h['elem_ext']
    ctx = fep.MeshContext(elem, coord)
    _, _, w, det = ctx.geometry()
    ctx.close()
    assert det.min() > 0
    hole = cc.curved_loop_area(coord, _wall_rows(h, t), 3 if t == 'P2' else 4)
    print(f'{t}: hole area {hole!r}, ellipse {np.pi * H.a * H.b!r}, sum of weights {w.sum()!r}')
    assert abs(w.sum() - (1e4 - hole)) <= 1e-12 * 1e4
    assert abs(1 - hole / (np.pi * H.a * H.b)) < 1e-4
    rng = np.random.default_rng(11)
    _run_case(fep, monkeypatch, capfd, t, 'default', elem, coord / 10 + 5, 'plain', 0.1, rng)


# ---- drivers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'P2'])
def test_tsx_driver_on_the_curved_tunnel(fep, tsx_csv_dir, tunnel, t):
    """refine=1 with TSX_HOLE: the mesh prepared on the GPU against the same driver fed the host-projected arrays, to DESIGN
    section 7's driver tolerance.  No displacement is pinned: the curved run has no reference."""
    H = fep.tsx_tunnel.TSX_HOLE
    c1, e1 = fep.refine_uniform(*tunnel, curves=[H])
    if t == 'P2':
        p2 = fep.create_midpoints_P2(c1, e1, curves=[H])
        c1, e1 = p2['coord_ext'], p2['elem_ext']
    hd = fep.solve_tsx_tunnel(mesh_dir=tsx_csv_dir, element_type=t, refine=1, curves=[H])
    assert np.array_equal(hd['elem'], e1) and np.array_equal(hd['coords'], c1)
    hh = fep.solve_tsx_tunnel(c1, e1, t)
    for h in (hd, hh):
        print(f'{t} level 1, ellipse:', repr(h['displ'][-1]), h['n_plast'][-1], h['n_calls'])
        assert len(h['zeta']) == 17 and h['zeta'][-1] == 1.0
    assert hd['n_plast'] == hh['n_plast']
    for k in range(17):
        assert relerr(hd['U'][k], hh['U'][k]) <= 1e-10, k


def test_tsx_sharded_driver_takes_curves(fep, tunnel):
    """One rank: the sharded driver prepares the same curved mesh and reaches the single-GPU driver's displacement with the
    same solver (the gathered multigrid is the single-GPU one on the merged K)."""
    H = fep.tsx_tunnel.TSX_HOLE
    a = fep.solve_tsx_tunnel(*tunnel, 'P1', refine=1, curves=[H], linear_solver='amg')
    b = fep.solve_tsx_tunnel_sharded(*tunnel, 'P1', refine=1, curves=[H], linear_solver='amg')
    assert np.array_equal(a['coords'], b['coords']) and np.array_equal(a['elem'], b['elem'])
    assert len(b['zeta']) == 17 and a['n_plast'] == b['n_plast']
    assert relerr(b['U'][-1], a['U'][-1]) <= 1e-9


def test_tsx_driver_without_curves_is_the_recorded_run(fep, tunnel):
    tr = load_golden('tsx_refined1_trace')
    h = fep.solve_tsx_tunnel(*tunnel, 'P1', refine=1, curves=None)
    assert np.array_equal(tr['coord'], h['coords']) and np.array_equal(tr['elem'], h['elem'])
    assert len(h['zeta']) == 17 and h['n_plast'] == tr['nplast'].tolist()
    assert np.abs(np.array(h['displ']) - tr['U_mon']).max() <= 1e-10 * np.abs(tr['U_mon']).max()
    assert relerr(h['U'][-1], tr['U_final']) <= 1e-10


def test_driver_refuses_a_folded_curved_element(fep):
    """The over-curved triangle as one P2 element: its curved side passes the apex, the determinant changes sign inside."""
    newton = import_module('fem-elastoplasticity_amd.newton')
    coord, elem, curves = cc.over_curved(fep)
    h = fep.create_midpoints_P2(coord, elem, device=DEV, curves=curves)
    ctx = fep.MeshContext(h['elem_ext'], h['coord_ext'])
    try:
        assert ctx.geometry()[3].min() <= 0
        newton._refuse_folded({'curved': False}, ctx)
        with pytest.raises(ValueError, match='non-positive Jacobian determinant'):
            newton._refuse_folded({'curved': True}, ctx)
    finally:
        ctx.close()

"""
Refinement of marked triangles on the GPU (fep_mesh_mark, fep_mesh_refine_marked_*) against the NumPy twin
(refine_marked(device=None)): every array bit for bit, every result conforming by fep_mesh_info of a DeviceMesh built from
it; the refusals; and the adaptive tunnel driver against its run on the CPU through the oracle context.
"""
import ctypes as C
from contextlib import closing

import numpy as np
import pytest

import marked_cases as mc
from conftest import relerr
from oracle_context import OracleContext

pytestmark = pytest.mark.gpu

DEV = 0
EINVAL, ESTATE = -1, -6                                       # include/fep.h


def _both(fep, coord, elem, marked, curves=None, info=None):
    """Device result, checked bit for bit against the host's and for conformity; `info`: the expected mark counts."""
    host = fep.refine_marked(coord, elem, marked, curves=curves)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        if curves:
            m.set_curves(curves)
        got = m.mark(marked)
        dev = m.refine_marked()
        again = m.refine_marked()
        res = [a.cpu().numpy() for a in m.refine_marked_dev()]
    assert got['n_child'] == host[1].shape[1] and got['n_new_nodes'] == host[0].shape[1] - np.shape(coord)[1]
    if info is not None:
        assert (got['n_child'], got['n_new_nodes'], got['n_marked_elements']) == info, got
    for d, h, a in zip(dev, host, again):
        assert d.shape == h.shape and d.dtype == h.dtype and d.tobytes() == h.tobytes() == a.tobytes()
    for d, r in zip(dev, res):
        assert np.array_equal(d, r) and r.dtype == (np.float64 if d.dtype == np.float64 else np.int32)
    for a, b in zip(dev, fep.refine_marked(coord, elem, marked, device=DEV, curves=curves)):
        assert a.tobytes() == b.tobytes()
    c, e, p = dev
    with fep.DeviceMesh(c, e, DEV) as m2:
        if not curves:
            mc.check_conforming(np.asarray(coord, dtype=float), np.asarray(elem), mc.marked_boundary_edges(coord, elem, c, e),
                                c, e, p, info=m2.info)
        else:
            assert (m2.info['n_nonmanifold'], m2.info['n_inconsistent'], m2.info['n_degenerate']) == (0, 0, 0)
            assert (mc.mp.doubled_areas(c, e) > 0).all()
    return dev


def _rows(elem):
    return [tuple(int(v) for v in col) for col in np.asarray(elem).T]


def test_patterns_by_hand(fep):
    tri = np.array([[0], [1], [2]])
    for slot in (0, 1, 2):
        c, e, p = _both(fep, np.array(mc.ONE_TRIANGLE[slot], dtype=float).T, tri, [1], info=(4, 3, 1))
        assert _rows(e) == mc.ONE_TRIANGLE_CHILDREN[slot]
    c, e, p = _both(fep, mc.PAIR_COORD, mc.PAIR_ELEM, [0, 1], info=(6, 3, 2))
    assert _rows(e) == [(1, 4, 0), (4, 2, 0), (3, 5, 6), (6, 5, 1), (5, 2, 4), (5, 4, 1)]
    c, e, p = _both(fep, mc.PAIR_COORD, mc.PAIR_ELEM, [1, 0], info=(7, 4, 2))
    assert _rows(e) == [(1, 4, 6), (6, 4, 0), (4, 2, 5), (4, 5, 0), (3, 7, 1), (7, 2, 4), (7, 4, 1)]
    equi = np.array([[0.0, 3.0, 1.5], [0.0, 0.0, 3 * np.sqrt(0.75)]])                  # an exact tie: test_refine_marked_host
    assert _rows(_both(fep, equi, tri, [1])[1]) == mc.ONE_TRIANGLE_CHILDREN[0]
    coord = np.array([[0.0, 4.0, 0.0, 9.0, 4.0, 7.0], [0.0, 0.0, 3.0, 3.0, 0.0, 7.0]])  # a repeated and an orphan node
    c, e, p = _both(fep, coord, np.array([[0, 4], [1, 3], [2, 2]]), [1, 0], info=(5, 3, 1))
    assert _rows(e) == [(1, 6, 8), (8, 6, 0), (6, 2, 7), (6, 7, 0), (4, 3, 2)]


def test_no_marks_is_the_identity(fep):
    coord, elem = mc.tunnel()
    c, e, p = _both(fep, coord, elem, np.zeros(887, dtype=bool), info=(887, 0, 0))
    assert np.array_equal(c, coord) and np.array_equal(e, elem) and np.array_equal(p, np.arange(887))


@pytest.mark.parametrize('name', ['tunnel', 'unstructured'])
def test_all_marked_gives_uniform_refinements_nodes(fep, name):
    coord, elem = mc.tunnel() if name == 'tunnel' else mc.unstructured()
    n_e, n_edges = elem.shape[1], len(mc.mp._edge_map(elem))
    c, e, p = _both(fep, coord, elem, np.ones(n_e, dtype=bool), info=(4 * n_e, n_edges, n_e))
    cu, eu = fep.refine_uniform(coord, elem, device=DEV)
    assert c.tobytes() == cu.tobytes() and c.shape == cu.shape


def test_all_marked_with_the_tunnel_wall(fep):
    coord, elem = mc.tunnel()
    hole = [fep.tsx_tunnel.TSX_HOLE]
    c, e, p = _both(fep, coord, elem, np.ones(887, dtype=bool), curves=hole)
    cu, eu = fep.refine_uniform(coord, elem, device=DEV, curves=hole)
    straight = fep.refine_uniform(coord, elem, device=DEV)[0]
    assert c.tobytes() == cu.tobytes()
    moved = np.flatnonzero((c != straight).any(axis=0))
    h = hole[0]
    g = np.sqrt(((c[0, moved] - h.cx) / h.a) ** 2 + ((c[1, moved] - h.cy) / h.b) ** 2)
    assert moved.size == 25 and np.abs(g - 1).max() <= 4 * np.finfo(float).eps


def test_a_child_folded_by_the_curve_is_refused(fep):
    with pytest.raises(ValueError, match='non-positive area'):
        fep.refine_marked(mc.FOLD_COORD, mc.FOLD_ELEM, [1], device=DEV, curves=[fep.Ellipse(0.0, 0.0, 1.0, 1.0)])
    _both(fep, mc.FOLD_COORD, mc.FOLD_ELEM, [1], info=(4, 3, 1))


def test_closure_chain_through_several_workgroups(fep):
    coord, elem = mc.chain()
    first, last = np.zeros(600, dtype=bool), np.zeros(600, dtype=bool)
    first[0], last[599] = True, True
    _both(fep, coord, elem, first, info=(1801, 602, 600))
    _both(fep, coord, elem, last, info=(604, 3, 2))
    both = first | last                                                              # marks replace the earlier ones
    with fep.DeviceMesh(coord, elem, DEV) as m:
        assert m.mark(first)['n_child'] == 1801 and m.mark(last)['n_child'] == 604
        assert m.mark(both)['n_child'] == 1802                                       # triangle 599's third edge as well
        import torch
        on_dev = torch.from_numpy(last.view(np.uint8)).to(f'cuda:{DEV}')
        assert m.mark(on_dev, on_device=True)['n_child'] == 604
        assert m.refine_marked()[1].tobytes() == fep.refine_marked(coord, elem, last)[1].tobytes()


def test_chained_rounds(fep):
    coord, elem = mc.perturbed_square()
    angle0, area0 = mc.smallest_angle(coord, elem), mc.mp.doubled_areas(coord, elem).sum() / 2
    rng = np.random.default_rng(11)
    for rnd in range(1, 13):
        coord, elem, parent = _both(fep, coord, elem, mc.round_marks(rnd, elem, rng))
        assert mc.smallest_angle(coord, elem) >= angle0 / 2, rnd
        assert abs(mc.mp.doubled_areas(coord, elem).sum() / 2 - area0) <= mc.total_area_bound(coord, elem.shape[1] + 72), rnd
    assert elem.shape[1] > 5000


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _raw_refine(fep, m, n_child, n_tot, null=None):
    """fep_mesh_refine_marked_host on canary-filled outputs -> (code, outputs untouched)."""
    child = np.full((3, n_child), -77, dtype=np.int32)
    coord = np.full((2, n_tot), -7.5)
    parent = np.full(n_child, -77, dtype=np.int32)
    ptrs = [fep._lib.ptr(child), fep._lib.ptr(coord), fep._lib.ptr(parent)]
    if null is not None:
        ptrs[null] = None
    rc = fep.lib().fep_mesh_refine_marked_host(m._h, *ptrs)
    return rc, bool((child == -77).all() and (coord == -7.5).all() and (parent == -77).all())


def test_refusals_leave_the_outputs_alone(fep):
    import torch
    coord, elem = mc.PAIR_COORD, mc.PAIR_ELEM
    out = np.zeros(4, dtype=np.int64)
    p_out = out.ctypes.data_as(fep._lib.c_i64_p)
    marks = np.array([1, 0], dtype=np.uint8)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        with pytest.raises(ValueError, match='mark'):
            m.refine_marked()
        assert _raw_refine(fep, m, 7, 8) == (ESTATE, True)                            # before any mark
        dev_child = torch.full((3, 7), -77, dtype=torch.int32, device=f'cuda:{DEV}')
        dev_coord = torch.full((2, 8), -7.5, dtype=torch.float64, device=f'cuda:{DEV}')
        rc = fep.lib().fep_mesh_refine_marked_dev(m._h, None, C.c_void_p(dev_child.data_ptr()), C.c_void_p(dev_coord.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == ESTATE and bool((dev_child == -77).all()) and bool((dev_coord == -7.5).all())
        # marks on the wrong side: a host array called a device one, a device tensor called a host one
        assert fep.lib().fep_mesh_mark(m._h, None, fep._lib.ptr(marks), 1, p_out) == EINVAL
        on_dev = torch.from_numpy(marks).to(f'cuda:{DEV}')
        assert fep.lib().fep_mesh_mark(m._h, None, C.c_void_p(on_dev.data_ptr()), 0, p_out) == EINVAL
        assert fep.lib().fep_mesh_mark(m._h, None, None, 0, p_out) == EINVAL
        assert fep.lib().fep_mesh_mark(m._h, None, fep._lib.ptr(marks), 0, None) == EINVAL
        assert not out.any()
        assert _raw_refine(fep, m, 7, 8) == (ESTATE, True)                            # still no marks
        assert m.mark(marks)['n_child'] == 7
        for null in (0, 1):
            assert _raw_refine(fep, m, 7, 8, null=null) == (EINVAL, True)
        assert fep.lib().fep_mesh_mark(m._h, None, fep._lib.ptr(marks), 1, p_out) == EINVAL      # keeps the marks it had
        rc, clean = _raw_refine(fep, m, 7, 8, null=2)                                 # parent may be NULL
        assert rc == 0 and not clean
    assert fep.lib().fep_mesh_refine_marked_host(None, None, None, None) == EINVAL
    # a non-manifold mesh: three triangles on the edge 0-1
    co = np.array([[0.0, 1.0, 0.0, 1.0, 0.5], [0.0, 0.0, 1.0, 1.0, -1.0]])
    el = np.array([[0, 1, 0], [1, 0, 1], [2, 4, 3]])
    with fep.DeviceMesh(co, el, DEV) as m:
        assert m.info['n_nonmanifold'] > 0 or m.info['n_inconsistent'] > 0
        assert fep.lib().fep_mesh_mark(m._h, None, fep._lib.ptr(np.ones(3, dtype=np.uint8)), 0, p_out) == ESTATE
        assert _raw_refine(fep, m, 12, 14) == (ESTATE, True)
        with pytest.raises(ValueError, match='edge-manifold'):
            m.mark([1, 1, 1])
    # a valid call on the same device still passes
    _both(fep, mc.PAIR_COORD, mc.PAIR_ELEM, [1, 0], info=(7, 4, 2))


# ---- the driver -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_run(fep):
    coord, elem = mc.tunnel()
    return fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, adapt=2, mark=mc.near_tunnel)


def test_driver_gpu_against_the_host_run(fep, host_run):
    coord, elem = mc.tunnel()
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', adapt=2, mark=mc.near_tunnel)
    assert h['coords'].tobytes() == host_run['coords'].tobytes() and h['elem'].tobytes() == host_run['elem'].tobytes()
    for a, b in zip(h['adapt'], host_run['adapt']):
        assert (a['n_e'], a['n_n'], a['n_marked'], a['n_child']) == (b['n_e'], b['n_n'], b['n_marked'], b['n_child'])
        assert (a['parent'] is None and b['parent'] is None) or np.array_equal(a['parent'], b['parent'])
    assert len(h['zeta']) == 17 == len(host_run['zeta']) and np.allclose(h['zeta'], host_run['zeta'], rtol=0, atol=1e-15)
    assert h['n_plast'] == host_run['n_plast']
    mon = np.array(host_run['displ'])
    assert np.abs(np.array(h['displ']) - mon).max() <= 1e-10 * np.abs(mon).max()
    for k in range(17):
        assert relerr(h['U'][k], host_run['U'][k]) <= 1e-10, k


@pytest.mark.parametrize('t,curves', [('P1', False), ('P2', True)])
def test_driver_marks_where_it_went_plastic(fep, t, curves):
    coord, elem = mc.tunnel()
    kw = dict(curves=[fep.tsx_tunnel.TSX_HOLE]) if curves else {}
    h = fep.solve_tsx_tunnel(coord, elem, t, adapt=2, **kw)
    assert [row['n_steps'] for row in h['adapt']] == [17, 17, 17] and abs(h['zeta'][-1] - 1) < 1e-12
    d1, d2, wf = fep.element_tables(t)
    for row in h['adapt'][:-1]:
        # the plastic elements found by where the plastic points ARE, not by their position in the flag array
        with closing(fep.MeshContext(row['elem'], row['coords'], d1, d2, wf)) as ctx:
            xq = np.asarray(ctx.point_coords())
        assert xq.shape == (2, row['ind_p'].size) and row['ind_p'].sum() == row['n_plast'] > 0
        plastic = np.zeros(row['n_e'], dtype=bool)
        plastic[mc.elements_of_points(row['coords'], row['elem'], xq[:, row['ind_p']])] = True
        assert np.array_equal(plastic, row['plastic'])
        assert (row['marked'] | ~plastic).all()
        assert np.bincount(row['parent'], minlength=row['n_e'])[plastic].min() > 1
    final = h['elem'][:3]
    with fep.DeviceMesh(h['coords'], final, DEV) as m:
        assert (m.info['n_nonmanifold'], m.info['n_inconsistent'], m.info['n_degenerate']) == (0, 0, 0)
    assert final.shape[1] == h['adapt'][-1]['n_e'] < 16 * 887                        # refine=2 has 14 192
    assert (mc.mp.doubled_areas(h['coords'], final) > 0).all()


def test_adapt_0_is_the_plain_run(fep):
    coord, elem = mc.tunnel()
    a = fep.solve_tsx_tunnel(coord, elem, 'P1')
    b = fep.solve_tsx_tunnel(coord, elem, 'P1', adapt=0, mark=mc.near_tunnel)
    assert sorted(a) == sorted(b) and 'adapt' not in b and 'ind_p' not in b
    assert a['zeta'] == b['zeta'] and a['n_plast'] == b['n_plast'] and a['n_calls'] == b['n_calls']
    # exactly: results are run-to-run bitwise reproducible and adapt=0 is the same code path
    assert len(a['U']) == len(b['U']) == 17 and all(x.tobytes() == y.tobytes() for x, y in zip(a['U'], b['U']))
    assert np.array(a['displ']).tobytes() == np.array(b['displ']).tobytes() and a['F0'].tobytes() == b['F0'].tobytes()
    assert np.array_equal(a['Q'], b['Q'])
    assert abs(a['displ'][-1] - (-0.0019794496707526746)) <= 1e-10 * 0.0019794496707526746

"""
The mesh kernels (fep_mesh_*: half-edge matching, P1 -> P2 / P4 enrichment, uniform refinement) against the host
create_midpoints_P2 / _P4 — themselves pinned bit for bit to the reference's generator on the tunnel mesh by
test_midpoint_numbering_bit_exact_on_tunnel_mesh — and, on the tunnel mesh, against the arrays recorded in tsx.npz.
Every comparison is np.array_equal plus equal shape and dtype on every key: there is no tolerance to choose.
The refusals (mixed orientation, non-manifold edge, degenerate triangle, vertex id out of range) are ordinary error
returns; after each one a valid call on the same device must still pass.
"""
import numpy as np
import pytest

import fan_mesh
import meshes
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

DEV = 0


def _orient(elem, coord):
    """Delaunay's triangles are not guaranteed to be counter-clockwise: make them."""
    x, y = coord
    d = (x[elem[1]] - x[elem[0]]) * (y[elem[2]] - y[elem[0]]) - (x[elem[2]] - x[elem[0]]) * (y[elem[1]] - y[elem[0]])
    e = np.array(elem, copy=True)
    e[1, d < 0], e[2, d < 0] = elem[2, d < 0], elem[1, d < 0]
    return e


def _same(a, b, what=''):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.shape(a[k]) == np.shape(b[k]) and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _tunnel():
    g = load_golden('tsx')
    return g['coord'], g['elem']


def _cases(fep):
    rng = np.random.default_rng(3)
    coord, elem = _tunnel()
    yield 'tunnel', coord, elem
    m = fep.square_mesh(37, 'P1', 10)
    yield 'square 37', m['coordinates'], m['elements']
    el, co = meshes.delaunay('P1', 40, rng)
    el = _orient(el, co)
    yield 'delaunay 40', co, el
    el2, co2 = meshes.renumber(el, co, rng)
    yield 'delaunay 40 renumbered', co2, el2
    ef, cf = fan_mesh.fan_p1(200)
    yield 'fan 200', cf, ef
    yield 'delaunay 40, last 40 dropped', co, meshes.drop_last(el, 40)


@pytest.mark.parametrize('t', ['P2', 'P4'])
def test_enrichment_bit_equal_to_host(fep, t):
    host = fep.create_midpoints_P2 if t == 'P2' else fep.create_midpoints_P4
    for name, coord, elem in _cases(fep):
        h = host(coord, elem)
        d = (fep.create_midpoints_P2 if t == 'P2' else fep.create_midpoints_P4)(coord, elem, device=DEV)
        _same(d, h, name)
        _same(fep.create_midpoints(t, coord, elem, device=DEV), h, name)
        if name == 'tunnel':
            g = load_golden('tsx')
            assert np.array_equal(d['coord_ext'], g[f'{t.lower()}_coord']) and np.array_equal(d['elem_ext'], g[f'{t.lower()}_elem'])


@pytest.mark.parametrize('t', ['P2', 'P4'])
def test_enrichment_on_the_tunnel_refined_three_times(fep, t):
    coord, elem = fep.refine_uniform(*_tunnel(), levels=3)
    assert elem.shape[1] == 56768
    h = fep.create_midpoints(t, coord, elem)
    d = fep.create_midpoints(t, coord, elem, device=DEV)
    _same(d, h)
    _same(fep.create_midpoints(t, coord, elem, device=DEV), d, 'second call')          # two calls: identical bytes


def test_device_resident_outputs_equal_host_outputs(fep):
    coord, elem = _tunnel()
    for t in ('P2', 'P4'):
        h = fep.create_midpoints(t, coord, elem)
        with fep.DeviceMesh(coord, elem, DEV) as m:
            assert m.info['n_e'] == 887 and m.info['n_n'] == coord.shape[1]
            assert m.info['n_boundary_edges'] == h['surf'].shape[1]
            assert coord.shape[1] + m.new_nodes(t) == h['coord_ext'].shape[1]
            out = [a.cpu().numpy() for a in m.enrich_dev(t)]
            again = [a.cpu().numpy() for a in m.enrich_dev(t)]
        assert np.array_equal(out[0], h['elem_ext']) and np.array_equal(out[1], h['coord_ext'])
        assert np.array_equal(out[2], h['surf'])
        if t == 'P2':
            assert np.array_equal(out[3], h['elem_ed']) and np.array_equal(out[4], h['edge_el'])
        for a, b in zip(out, again):
            assert a.tobytes() == b.tobytes()


def test_refine_uniform_bit_equal_to_host(fep):
    coord, elem = _tunnel()
    c, e = coord, elem
    for lv in (1, 2, 3):
        c, e = fep.refine_uniform(c, e)                                               # three host levels
        cd, ed = fep.refine_uniform(coord, elem, levels=lv, device=DEV)               # chained on the device
        assert cd.shape == c.shape and cd.dtype == c.dtype and np.array_equal(cd, c), lv
        assert ed.shape == e.shape and ed.dtype == e.dtype and np.array_equal(ed, e), lv
    cd2, ed2 = fep.refine_uniform(coord, elem, levels=3, device=DEV)
    assert cd2.tobytes() == cd.tobytes() and ed2.tobytes() == ed.tobytes()
    co, el = next(x[1:] for x in _cases(fep) if x[0] == 'delaunay 40')
    for a, b in zip(fep.refine_uniform(co, el, device=DEV), fep.refine_uniform(co, el)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def _valid_call_passes(fep):
    coord, elem = _tunnel()
    _same(fep.create_midpoints_P2(coord, elem, device=DEV), fep.create_midpoints_P2(coord, elem))


def test_refuses_mixed_orientation(fep):
    rng = np.random.default_rng(5)
    el, co = meshes.delaunay('P1', 12, rng)
    el = meshes.mixed_orientation(_orient(el, co), rng)
    with fep.DeviceMesh(co, el, DEV) as m:
        assert m.info['n_inconsistent'] > 0 and m.info['n_nonmanifold'] == 0 and m.info['n_degenerate'] == 0
        n = m.info['n_inconsistent']
    for call in (lambda: fep.create_midpoints_P2(co, el, device=DEV), lambda: fep.create_midpoints_P4(co, el, device=DEV),
                 lambda: fep.refine_uniform(co, el, device=DEV)):
        with pytest.raises(ValueError, match=f'n_inconsistent={n}') as ei:
            call()
        assert 'host functions' in str(ei.value)
    assert isinstance(fep.create_midpoints_P2(co, el), dict)                           # the host form keeps its behaviour
    _valid_call_passes(fep)


def test_refusal_writes_nothing(fep):
    """The C entry points on a refused mesh: FEP_ESTATE and the output buffers untouched."""
    import ctypes as C
    lib_mod = __import__('importlib').import_module('fem-elastoplasticity_amd._lib')
    rng = np.random.default_rng(5)
    el, co = meshes.delaunay('P1', 12, rng)
    el = meshes.mixed_orientation(_orient(el, co), rng)
    with fep.DeviceMesh(co, el, DEV) as m:
        n_e, n_n = m.info['n_e'], m.info['n_n']
        elem_ext = np.full((6, n_e), -7, dtype=np.int32)
        coord_ext = np.full((2, n_n + 3 * n_e), -7.0)
        surf = np.full((3, 3 * n_e), -7, dtype=np.int32)
        rc = fep.lib().fep_mesh_enrich_host(m._h, 2, lib_mod.ptr(elem_ext), lib_mod.ptr(coord_ext), lib_mod.ptr(surf), None, None)
        assert rc == -6
        child = np.full((3, 4 * n_e), -7, dtype=np.int32)
        assert fep.lib().fep_mesh_refine_host(m._h, lib_mod.ptr(child), lib_mod.ptr(coord_ext)) == -6
        assert (elem_ext == -7).all() and (coord_ext == -7.0).all() and (surf == -7).all() and (child == -7).all()
        assert fep.lib().fep_mesh_enrich_host(m._h, 1, lib_mod.ptr(elem_ext), lib_mod.ptr(coord_ext), lib_mod.ptr(surf), None, None) == -1
    h = C.c_void_p()
    e32 = np.ascontiguousarray(el, dtype=np.int32)
    assert fep.lib().fep_mesh_create(C.byref(h), DEV, None, 0, co.shape[1], lib_mod.ptr(e32), lib_mod.ptr(co), 0) == -1
    assert fep.lib().fep_mesh_create(C.byref(h), DEV, None, el.shape[1], co.shape[1], None, lib_mod.ptr(co), 0) == -1
    assert fep.lib().fep_mesh_info(None, None) == -1 and fep.lib().fep_mesh_destroy(None) == 0
    _valid_call_passes(fep)


def test_refuses_nonmanifold_edge(fep):
    coord, elem = _tunnel()
    h = fep.create_midpoints_P2(coord, elem)
    k = int(np.flatnonzero(h['edge_el'][1] > 0)[0])                                   # an interior edge
    i = int(h['edge_el'][0, k])
    s = int(np.flatnonzero(h['elem_ed'][:, i] == k)[0])
    A, B = elem[(s + 1) % 3, i], elem[(s + 2) % 3, i]
    co = np.concatenate([coord, [[1000.0], [1000.0]]], axis=1)                        # a third triangle on that edge
    el = np.concatenate([elem, [[A], [B], [coord.shape[1]]]], axis=1)
    with fep.DeviceMesh(co, el, DEV) as m:
        assert m.info['n_nonmanifold'] == 1 and m.info['n_degenerate'] == 0
    with pytest.raises(ValueError, match='n_nonmanifold=1'):
        fep.create_midpoints_P2(co, el, device=DEV)
    _valid_call_passes(fep)


def test_refuses_degenerate_triangle(fep):
    coord, elem = _tunnel()
    el = elem.copy()
    el[1, 5] = el[0, 5]                                                               # (v, v, w)
    with fep.DeviceMesh(coord, el, DEV) as m:
        assert m.info['n_degenerate'] == 1
    with pytest.raises(ValueError, match='n_degenerate=1'):
        fep.create_midpoints_P4(coord, el, device=DEV)
    _valid_call_passes(fep)


def test_vertex_id_out_of_range_is_erange(fep):
    coord, elem = _tunnel()
    for bad in (coord.shape[1], -1, 2 ** 40):
        el = elem.copy()
        el[2, 7] = bad
        with pytest.raises(fep.FepError) as ei:
            fep.create_midpoints_P2(coord, el, device=DEV)
        assert ei.value.code == -5
    _valid_call_passes(fep)


def test_tsx_driver_on_the_device_mesh_path(fep, tsx_csv_dir):
    """refine=1, P2: the mesh made on the GPU against the same driver on arrays made by the host forms — equal meshes, so
    equal histories (the tolerance test_newton_gpu.py holds a TSX trace to) — and both against the CPU checker's figures."""
    coord, elem = _tunnel()
    c1, e1 = fep.refine_uniform(coord, elem)
    p2 = fep.create_midpoints_P2(c1, e1)
    hd = fep.solve_tsx_tunnel(mesh_dir=tsx_csv_dir, element_type='P2', refine=1)
    assert np.array_equal(hd['coords'], p2['coord_ext']) and np.array_equal(hd['elem'], p2['elem_ext'])
    hh = fep.solve_tsx_tunnel(p2['coord_ext'], p2['elem_ext'], 'P2')
    for h in (hd, hh):
        print('P2 level 1:', repr(h['displ'][-1]), h['n_plast'][-1], h['n_calls'])
        assert len(h['zeta']) == 17 and h['zeta'][-1] == 1.0
        assert abs(h['displ'][-1] - (-0.002268048311244893)) <= 1e-9 * 0.002268048311244893
        assert h['n_plast'][-1] == 171 and abs(h['n_calls'] - 58) <= 2
    assert hd['n_plast'] == hh['n_plast']
    assert np.abs(np.array(hd['displ']) - np.array(hh['displ'])).max() <= 1e-10 * np.abs(np.array(hh['displ'])).max()
    for k in range(17):
        assert relerr(hd['U'][k], hh['U'][k]) <= 1e-10, k


def test_tsx_driver_amg_on_the_tunnel_refined_twice(fep, tsx_csv_dir):
    h = fep.solve_tsx_tunnel(mesh_dir=tsx_csv_dir, element_type='P1', refine=2, linear_solver='amg')
    print('P1 level 2, amg:', repr(h['displ'][-1]), h['n_plast'][-1], h['n_calls'])
    assert h['elem'].shape == (3, 14192) and h['coords'].shape == (2, 7226)
    assert len(h['zeta']) == 17 and h['zeta'][-1] == 1.0
    assert abs(h['displ'][-1] - (-0.0022392766813373157)) <= 1e-9 * 0.0022392766813373157

"""
Uniform refinement and the TSX driver on refined meshes, without a GPU: the host forms (`device=None`) and the CPU
checker as hot path (oracle_context.OracleContext through `context_factory`).

Counts and areas of the refined tunnel mesh are properties of the mesh (Euler's formula, and a child of a red refinement
has a quarter of its parent's area up to the few roundings of a cross product: bound 1e-12 relative).  The driver pins are
the CPU checker's with SuperLU (1e-9 relative, what DESIGN section 7 grants a driver result across solvers; return-map
calls within +-2) and, for the level-1 P1 run, the reference's own functions replayed with dense solves
(tests/golden/make_golden_tsx_refined.py -> tsx_refined1_trace.npz; 1e-10 on the displacement and exact plastic counts,
as test_newton_gpu.py holds the level-0 run).
"""
import numpy as np
import pytest

from conftest import load_golden, relerr
from oracle_context import OracleContext

COUNTS = {1: (3548, 1839), 2: (14192, 7226), 3: (56768, 28644)}
AREA = 9988.102114272


def _areas(coord, elem):
    x, y = coord
    return 0.5 * ((x[elem[1]] - x[elem[0]]) * (y[elem[2]] - y[elem[0]]) - (x[elem[2]] - x[elem[0]]) * (y[elem[1]] - y[elem[0]]))


def _check_edges(elem):
    """Every edge belongs to one or two triangles; the two of an interior edge walk it in opposite directions."""
    a = np.concatenate([elem[0], elem[1], elem[2]]).astype(np.int64)
    b = np.concatenate([elem[1], elem[2], elem[0]]).astype(np.int64)
    n = int(max(a.max(), b.max())) + 1
    directed = a * n + b
    assert np.unique(directed).size == directed.size                    # no edge walked twice the same way
    und, cnt = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    assert cnt.max() == 2 and cnt.min() == 1
    interior = und[cnt == 2]
    lo, hi = interior // n, interior % n
    assert np.isin(lo * n + hi, directed).all() and np.isin(hi * n + lo, directed).all()


@pytest.fixture(scope='module')
def tunnel():
    g = load_golden('tsx')
    return g['coord'], g['elem']


def test_refine_uniform_tunnel_levels(fep, tunnel):
    coord, elem = tunnel
    a0 = _areas(coord, elem)
    assert a0.min() > 0 and abs(a0.sum() - AREA) <= 1e-12 * AREA
    c, e = coord, elem
    for lv in (1, 2, 3):
        h = fep.create_midpoints_P2(c, e)
        c1, e1 = fep.refine_uniform(c, e)
        assert (e1.shape[1], c1.shape[1]) == COUNTS[lv] and e1.shape[0] == 3 and e1.dtype == np.int64
        assert np.array_equal(c1, h['coord_ext']) and np.array_equal(c1[:, :c.shape[1]], c)   # old nodes keep id and place
        V1, V2, V3, m23, m31, m12 = h['elem_ext']
        for k, child in enumerate(((V1, m12, m31), (m12, V2, m23), (m31, m23, V3), (m12, m23, m31))):
            assert np.array_equal(e1[:, k::4], np.stack(child)), (lv, k)
        a, a1 = _areas(c, e), _areas(c1, e1)
        assert a1.min() > 0                                              # orientation preserved
        assert abs(a1.sum() - AREA) <= 1e-12 * AREA
        assert (np.abs(a1.reshape(-1, 4) / (a[:, None] / 4) - 1)).max() <= 1e-12
        _check_edges(e1)
        c, e = c1, e1


def test_refine_uniform_levels_chain(fep, tunnel):
    coord, elem = tunnel
    c0, e0 = fep.refine_uniform(coord, elem, levels=0)
    assert np.array_equal(c0, coord) and np.array_equal(e0, elem)
    c2, e2 = fep.refine_uniform(coord, elem, levels=2)
    c1, e1 = fep.refine_uniform(*fep.refine_uniform(coord, elem))
    assert np.array_equal(c2, c1) and np.array_equal(e2, e1) and e2.dtype == e1.dtype
    cl, el = fep.prepare_tsx_mesh(coord, elem, 'P1', refine=2)[:2]
    assert np.array_equal(cl, c2) and np.array_equal(el, e2)


def test_load_tsx_mesh_refine(fep, tsx_csv_dir, tunnel):
    coord, elem = tunnel
    c1, e1 = fep.refine_uniform(coord, elem)
    for t, rows in (('P1', 3), ('P2', 6), ('P4', 15)):
        c, e = fep.load_tsx_mesh(tsx_csv_dir, t, refine=1)
        assert e.shape == (rows, 3548) and e.dtype == np.int64
        if t == 'P1':
            assert np.array_equal(c, c1) and np.array_equal(e, e1)
        else:
            h = fep.create_midpoints(t, c1, e1)
            assert np.array_equal(c, h['coord_ext']) and np.array_equal(e, h['elem_ext'])
    c, e = fep.load_tsx_mesh(tsx_csv_dir, 'P2')                          # refine=0: as before
    g = load_golden('tsx')
    assert np.array_equal(c, g['p2_coord']) and np.array_equal(e, g['p2_elem'])


def test_tsx_driver_refine0_is_the_level0_pin(fep, tunnel):
    coord, elem = tunnel
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', refine=0, linear_solver='direct', context_factory=OracleContext)
    assert len(h['zeta']) == 17 and h['n_plast'][-1] == 3
    assert abs(h['displ'][-1] - (-0.0019794496707526746)) <= 1e-10 * 0.0019794496707526746
    assert 'node_of_input' not in h


@pytest.fixture(scope='module')
def level1_run(fep, tunnel):
    coord, elem = tunnel
    return fep.solve_tsx_tunnel(coord, elem, 'P1', refine=1, linear_solver='direct', context_factory=OracleContext)


def test_tsx_driver_refine1_on_oracle(level1_run):
    h = level1_run
    print('level 1:', repr(h['displ'][-1]), h['n_plast'][-1], h['n_calls'])
    assert len(h['zeta']) == 17 and h['zeta'][-1] == 1.0
    assert h['n_plast'][-1] == 20
    assert abs(h['displ'][-1] - (-0.002167352630121635)) <= 1e-9 * 0.002167352630121635
    assert abs(h['n_calls'] - 54) <= 2
    assert h['elem'].shape == (3, 3548) and h['coords'].shape == (2, 1839) and h['node_of_input'] is None


def test_tsx_driver_refine1_vs_reference_replay(fep, level1_run, tunnel):
    """The level-1 P1 run against the reference's own functions and dense solves on the same mesh."""
    tr = load_golden('tsx_refined1_trace')
    c1, e1 = fep.refine_uniform(*tunnel)
    assert np.array_equal(tr['coord'], c1) and np.array_equal(tr['elem'], e1)
    h = level1_run
    assert len(h['zeta']) == 17 == len(tr['zeta']) and np.allclose(h['zeta'], tr['zeta'], rtol=0, atol=1e-15)
    assert h['n_plast'] == tr['nplast'].tolist()
    assert relerr(h['F0'], tr['F0']) <= 1e-12
    print('displ error', np.abs(np.array(h['displ']) - tr['U_mon']).max() / np.abs(tr['U_mon']).max())
    assert np.abs(np.array(h['displ']) - tr['U_mon']).max() <= 1e-10 * np.abs(tr['U_mon']).max()
    assert relerr(h['U'][-1], tr['U_final']) <= 1e-10
    assert abs(h['n_calls'] - int(tr['n_calls'])) <= 2


def test_tsx_driver_monitor_under_renumber(fep, level1_run, tunnel):
    coord, elem = tunnel
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', refine=1, renumber=True, linear_solver='direct', context_factory=OracleContext)
    ref = level1_run
    assert len(h['zeta']) == 17 and h['n_plast'] == ref['n_plast']
    print('renumbered:', repr(h['displ'][-1]))
    assert abs(h['displ'][-1] - ref['displ'][-1]) <= 1e-9 * abs(ref['displ'][-1])
    assert abs(h['displ'][-1] - (-0.002167352630121635)) <= 1e-9 * 0.002167352630121635
    inv = h['node_of_input']
    assert inv.shape == (coord.shape[1],) and np.array_equal(h['coords'][:, inv], coord)
    assert inv[40] != 40 or np.array_equal(inv, np.arange(inv.size))
    assert relerr(h['U'][-1][:, inv], ref['U'][-1][:, :coord.shape[1]]) <= 1e-9


def test_refine_needs_p1_vertices(fep):
    g = load_golden('tsx')
    with pytest.raises(ValueError, match='P1 mesh'):
        fep.solve_tsx_tunnel(g['p2_coord'], g['p2_elem'], 'P2', refine=1, context_factory=OracleContext)

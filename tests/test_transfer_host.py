"""
State transfer across refinement on the host: corner codes, the tables and the NumPy twin (transfer.py) against hand-written
tables, exact rational arithmetic and the rules of include/fep.h.  No GPU.
"""
from fractions import Fraction

import numpy as np
import pytest

import marked_cases as mc
import transfer_cases as tc

TYPES = ('P1', 'P2', 'P4')
U = 2.0 ** -53

# children of marked_cases.ONE_TRIANGLE_CHILDREN with the ids replaced by hand: vertex k -> k; node 3 lies on edge 1 (code 4),
# node 4 on edge 2 (code 5), node 5 on edge 0 (code 3)
ONE_TRIANGLE_CORNERS = {
    0: [(0, 3, 5), (5, 3, 2), (3, 1, 4), (3, 4, 2)],
    1: [(1, 4, 3), (3, 4, 0), (4, 2, 5), (4, 5, 0)],
    2: [(2, 5, 4), (4, 5, 1), (5, 0, 3), (5, 3, 1)],
}
# element 0 of transfer_cases.flower(slot) by the edge flags (p, q) of the edges after its reference edge r = slot
FLOWER_CORNERS = {
    0: {(0, 0): [(0, 3, 2), (3, 1, 2)], (0, 1): [(0, 3, 5), (5, 3, 2), (3, 1, 2)], (1, 0): [(0, 3, 2), (3, 1, 4), (3, 4, 2)]},
    1: {(0, 0): [(1, 4, 0), (4, 2, 0)], (0, 1): [(1, 4, 3), (3, 4, 0), (4, 2, 0)], (1, 0): [(1, 4, 0), (4, 2, 5), (4, 5, 0)]},
    2: {(0, 0): [(2, 5, 1), (5, 0, 1)], (0, 1): [(2, 5, 4), (4, 5, 1), (5, 0, 1)], (1, 0): [(2, 5, 1), (5, 0, 3), (5, 3, 1)]},
}


def _rows(a):
    return [tuple(int(v) for v in col) for col in np.asarray(a).T]


# ---- corner codes -------------------------------------------------------------------------------------------------------------
def test_corner_codes_by_hand(fep):
    tri = np.array([[0], [1], [2]])
    for slot in (0, 1, 2):
        coord = np.array(mc.ONE_TRIANGLE[slot], dtype=float).T
        corners = fep.child_corners(coord, tri, [1])
        assert corners.dtype == np.uint8 and _rows(corners) == ONE_TRIANGLE_CORNERS[slot]
        # the codes name the ids of ONE_TRIANGLE_CHILDREN: vertex k -> k, edge k -> the node refine_marked put on it
        node_of_code = {0: 0, 1: 1, 2: 2, 3: 5, 4: 3, 5: 4}
        assert [tuple(node_of_code[c] for c in row) for row in _rows(corners)] == mc.ONE_TRIANGLE_CHILDREN[slot]
        assert _rows(fep.child_corners(coord, tri, [0])) == [(0, 1, 2)]
        for (p_on, q_on), want in FLOWER_CORNERS[slot].items():
            c = tc.case(f'flower{slot}-p{p_on}q{q_on}')
            assert _rows(c['corners'][:, c['parent'] == 0]) == want
        c = tc.case(f'flower{slot}-p1q1')
        assert _rows(c['corners'][:, c['parent'] == 0]) == ONE_TRIANGLE_CORNERS[slot]
    corners, parent = fep.uniform_corners(2)
    assert _rows(corners) == [(0, 3, 5), (3, 1, 4), (5, 4, 2), (3, 4, 5)] * 2 and parent.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError):
        fep.child_corners(mc.PAIR_COORD, mc.PAIR_ELEM, [1])


@pytest.mark.parametrize('name', [c['name'] for c in tc.cases()])
def test_coordinates_reproduce(fep, name):
    """Codes, parents and node ownership together: the parent's vertex coordinates, transferred as a P1 field, are the
    child's vertex coordinates — exactly (a midpoint is one rounding either way); on a curved wall against the same
    refinement without curves, which has the same codes."""
    c = tc.case(name)
    want = c['coord_child']
    if c['curves']:
        want = fep.refine_marked(c['coord'], c['elem'], c['marked'])[0]
        assert (want != c['coord_child']).any()
    got = fep.transfer_nodes_np('P1', c['elem'], c['elem_child'], c['parent'], c['corners'], c['coord'].T, n_n_child=want.shape[1])
    assert got.shape == (want.shape[1], 2) and np.array_equal(got, want.T)
    if c['marked'] is not None and not c['marked'].any():
        assert np.array_equal(c['parent'], np.arange(c['elem'].shape[1])) and (c['corners'] == [[0], [1], [2]]).all()
    else:
        assert c['elem_child'].shape[1] > c['elem'].shape[1]


# ---- the tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', TYPES)
def test_tables(fep, t):
    tab = fep.transfer_tables(t)
    n_p, n_q = tc.N_P[t], tc.N_Q[t]
    shapes, soc, W, near = tab['shapes'], tab['shape_of_code'], tab['W'], tab['near']
    assert shapes.shape == (21, 3) and shapes.dtype == np.uint8 and W.shape == (21, n_p, n_p) and near.shape == (21, n_q)
    assert soc.shape == (216,) and soc.dtype == np.int8 and near.dtype == np.uint8
    code = shapes[:, 0].astype(int) + 6 * shapes[:, 1] + 36 * shapes[:, 2]
    assert (np.diff(code) > 0).all() and np.array_equal(soc[code], np.arange(21)) and (soc >= 0).sum() == 21
    seen = set()
    for c in tc.cases():
        seen |= set(_rows(c['corners']))
    assert seen == set(_rows(shapes.T))                                  # the cases meet every shape, and no other occurs
    ident = int(soc[0 + 6 * 1 + 36 * 2])
    assert np.array_equal(W[ident], np.eye(n_p)) and near[ident].tolist() == list(range(n_q))
    assert np.abs(W.sum(axis=2) - 1).max() <= (n_p + 8) * U
    if t != 'P4':
        assert np.array_equal(W * 8, np.round(W * 8))                    # exact weights: multiples of 1/8
    else:
        assert near.max() > 0
    if t == 'P1':
        assert not near.any()


def _dec(x):
    """A table entry as the exact rational of its shortest decimal form: the literal of tables.py (1/3 stays the double)."""
    return Fraction(1, 3) if x == 1 / 3 else Fraction(repr(float(x)))


@pytest.mark.parametrize('t', ('P2', 'P4'))
def test_nearest_point_is_nearest(fep, t, capsys):
    """For every shape and child point the chosen parent point has the smallest distance, recomputed in exact rationals from
    the decimal literals of the quadrature table.  A true tie, or one closer than 1e-12 (relative), is listed, not failed:
    the table, not this test, is the definition."""
    tab = fep.transfer_tables(t)
    xi, _ = fep.get_quadrature_volume(t)
    n_q = xi.shape[1]
    pts = [(_dec(xi[0, k]), _dec(xi[1, k])) for k in range(n_q)]
    B = [(Fraction(1), 0, 0), (0, Fraction(1), 0), (0, 0, Fraction(1)), (Fraction(1, 2), Fraction(1, 2), 0),
         (0, Fraction(1, 2), Fraction(1, 2)), (Fraction(1, 2), 0, Fraction(1, 2))]
    ties = []
    for s, codes in enumerate(tab['shapes']):
        for k, (x1, x2) in enumerate(pts):
            l = (1 - x1 - x2, x1, x2)
            L = [sum(l[m] * B[int(codes[m])][i] for m in range(3)) for i in range(3)]
            d = [(L[1] - a) ** 2 + (L[2] - b) ** 2 for a, b in pts]
            best = min(d)
            close = [kk for kk in range(n_q) if d[kk] - best <= Fraction(1, 10 ** 12) * best]
            chosen = int(tab['near'][s, k])
            if len(close) > 1:
                ties.append((s, k, chosen, close))
                assert chosen in close
            else:
                assert chosen == close[0], (s, k)
    with capsys.disabled():
        if ties:
            print(f'\n{t}: {len(ties)} (shape, point, chosen, candidates) ties or near ties: {ties[:8]}')


# ---- the twin -----------------------------------------------------------------------------------------------------------------
def _poly(t, x, y):
    """Integer-coefficient polynomials of degree p (two components) in exact arithmetic."""
    p = {'P1': 1, 'P2': 2, 'P4': 4}[t]
    a = 3 - 2 * x + 5 * y
    b = (x - 2 * y) ** p + 3 * x * y ** (p - 1) - 7 if p > 1 else 4 * x - y + 1
    return a ** p if p > 1 else a, b


def _integer_meshes(fep):
    m = fep.square_mesh(3, 'P1', 3)
    coord, elem = np.array(m['coordinates'], dtype=float), np.asarray(m['elements'], dtype=np.int64)
    marked = np.zeros(elem.shape[1], dtype=bool)
    marked[[0, 7, 8]] = True
    cc, ec, parent = fep.refine_marked(coord, elem, marked)
    yield coord, elem, cc, ec, parent, fep.child_corners(coord, elem, marked)
    cc, ec = fep.refine_uniform(coord, elem)
    corners, parent = fep.uniform_corners(elem.shape[1])
    yield coord, elem, cc, ec, parent, corners
    cc, ec, parent = fep.refine_marked(mc.PAIR_COORD, mc.PAIR_ELEM, [1, 0])
    yield mc.PAIR_COORD, mc.PAIR_ELEM, cc, ec, parent, fep.child_corners(mc.PAIR_COORD, mc.PAIR_ELEM, [1, 0])


@pytest.mark.parametrize('t', TYPES)
def test_polynomials_are_reproduced(fep, t):
    """Nested spaces: a polynomial of degree <= p interpolated on the parent is the same polynomial on the child.  Straight
    meshes with integer vertices, so every node is a multiple of 1/8 and the polynomial's values are exact doubles.  Bound per
    entry: n_p products and n_p additions of the sum, each within u = 2^-53 of its exact value relative to the running
    magnitude <= sum_a |W_a| |u_a|, plus at most 8 roundings inside a P4 basis value (P1 and P2 weights are exact):
    (n_p + 8) u sum_a |W_a| |u_a|."""
    tab = fep.transfer_tables(t)
    n_p = tc.N_P[t]
    for coord, elem, cc, ec, parent, corners in _integer_meshes(fep):
        if t == 'P1':
            ep, xp, ech, xc = elem, coord, ec, cc
        else:
            hp, hc = fep.create_midpoints(t, coord, elem), fep.create_midpoints(t, cc, ec)
            ep, xp, ech, xc = hp['elem_ext'], hp['coord_ext'], hc['elem_ext'], hc['coord_ext']
        assert np.array_equal(xp * 8, np.round(xp * 8)) and np.array_equal(xc * 8, np.round(xc * 8))
        exact_p = [_poly(t, Fraction(float(x)), Fraction(float(y))) for x, y in xp.T]
        u = np.array([[float(v) for v in row] for row in exact_p])
        assert all(Fraction(float(v)) == v for row in exact_p for v in row)
        got = fep.transfer_nodes_np(t, ep, ech, parent, corners, u, n_n_child=xc.shape[1])
        own_ch, own_j = tc.owner_pairs(ech, xc.shape[1])
        for n in range(xc.shape[1]):
            ch, j = int(own_ch[n]), int(own_j[n])
            s = int(tab['shape_of_code'][int(corners[0, ch]) + 6 * int(corners[1, ch]) + 36 * int(corners[2, ch])])
            want = _poly(t, Fraction(float(xc[0, n])), Fraction(float(xc[1, n])))
            for i in range(2):
                scale = float(np.abs(tab['W'][s, j]) @ np.abs(u[ep[:, int(parent[ch])], i]))
                err = abs(Fraction(float(got[n, i])) - want[i])
                assert err <= Fraction((n_p + 8) * U) * Fraction(scale), (n, i, float(err), scale)


@pytest.mark.parametrize('t', TYPES)
@pytest.mark.parametrize('n_comp', (1, 2, 4))
def test_old_vertices_keep_their_values(fep, t, n_comp):
    for name in ('pair-10', 'flower1-p0q1', 'square-uniform'):
        c = tc.case(name)
        ep, n_np, ech, n_nc, _, _ = tc.raised(name, t)
        u = tc.nodal_field(n_np, n_comp)
        n_old = c['coord'].shape[1]
        u[1, 0] = -0.0
        got = fep.transfer_nodes_np(t, ep, ech, c['parent'], c['corners'], u, n_n_child=n_nc)
        assert got.shape == (n_nc, n_comp) and np.isfinite(got).all()
        assert np.array_equal(got[:n_old], u[:n_old])                      # ==; the vertices keep their ids
        keep = np.ones(n_old, dtype=bool)
        keep[1] = False
        assert got[:n_old][keep].tobytes() == u[:n_old][keep].tobytes()
        assert got[1, 0] == 0.0 and not np.signbit(got[1, 0])               # -0.0 becomes +0.0
        flat = fep.transfer_nodes_np(t, ep, ech, c['parent'], c['corners'], u[:, 0], n_n_child=n_nc)
        assert flat.shape == (n_nc,) and flat.tobytes() == np.ascontiguousarray(got[:, 0]).tobytes()


@pytest.mark.parametrize('t', TYPES)
def test_a_nan_reaches_exactly_its_set(fep, t):
    for name in ('pair-10', 'unstructured' if t == 'P1' else 'flower0-p1q1'):
        c = tc.case(name)
        ep, n_np, ech, n_nc, _, _ = tc.raised(name, t)
        parent, corners = c['parent'], c['corners']
        u = tc.nodal_field(n_np, 2)
        clean = fep.transfer_nodes_np(t, ep, ech, parent, corners, u, n_n_child=n_nc)
        own_ch, _ = tc.owner_pairs(ech, n_nc)
        for n0 in (0, n_np - 1):                                            # a vertex, and (P2, P4) a node with zero weights elsewhere
            bad = u.copy()
            bad[n0, 1] = np.nan
            got = fep.transfer_nodes_np(t, ep, ech, parent, corners, bad, n_n_child=n_nc)
            holds = (ep == n0).any(axis=0)
            want = holds[parent[own_ch]]
            assert want.any() and not want.all()
            assert np.array_equal(np.isnan(got[:, 1]), want) and got[:, 0].tobytes() == clean[:, 0].tobytes()
            assert got[~want].tobytes() == clean[~want].tobytes()
        assert fep.transfer_nodes_np(t, ep, ech, parent, corners, u, n_n_child=n_nc).tobytes() == clean.tobytes()
        # points
        n_q = tc.N_Q[t]
        q = tc.point_field(4, c['elem'].shape[1] * n_q)
        src = tc.point_sources(t, parent, corners)
        clean_q = fep.transfer_points_np(t, parent, corners, q)
        assert clean_q.tobytes() == np.ascontiguousarray(q[:, src]).tobytes()
        k0 = int(src[len(src) // 2])
        bad = q.copy()
        bad[2, k0] = np.inf
        bad[3, k0] = np.nan
        got = fep.transfer_points_np(t, parent, corners, bad)
        assert np.array_equal(np.isnan(got[3]), src == k0) and np.array_equal(np.isinf(got[2]), src == k0)
        assert got[:2].tobytes() == clean_q[:2].tobytes() and got[:, src != k0].tobytes() == clean_q[:, src != k0].tobytes()
        one = fep.transfer_points_np(t, parent, corners, q[0])
        assert one.shape == (src.size,) and one.tobytes() == np.ascontiguousarray(clean_q[0]).tobytes()


@pytest.mark.parametrize('t', TYPES)
def test_bad_children_get_nan_and_nothing_else_changes(fep, t):
    c = tc.case('unstructured' if t == 'P1' else 'tunnel-curved')
    ep, n_np, ech, n_nc, _, _ = tc.raised(c['name'], t)
    n_e, n_child, n_q = c['elem'].shape[1], c['parent'].size, tc.N_Q[t]
    u, q = tc.nodal_field(n_np, 2), tc.point_field(1, n_e * n_q)
    clean_u = fep.transfer_nodes_np(t, ep, ech, c['parent'], c['corners'], u, n_n_child=n_nc + 2)
    assert np.isnan(clean_u[n_nc:]).all() and np.isfinite(clean_u[:n_nc]).all()       # nodes of no child element
    clean_q = fep.transfer_points_np(t, c['parent'], c['corners'], q)
    parent, corners = c['parent'].copy(), c['corners'].copy()
    hit = [3, n_child // 2, n_child - 1, 7, 11]
    parent[hit[0]], parent[hit[1]] = n_e, -1
    corners[:, hit[2]] = (6, 0, 1)
    corners[:, hit[3]] = (0, 0, 1)                                                     # codes in range, no shape
    corners[:, hit[4]] = (255, 1, 2)
    got_u = fep.transfer_nodes_np(t, ep, ech, parent, corners, u, n_n_child=n_nc + 2)
    got_q = fep.transfer_points_np(t, parent, corners, q)
    own_ch, _ = tc.owner_pairs(ech, n_nc)
    want_u = np.concatenate([np.isin(own_ch, hit), [True, True]])
    want_q = np.repeat(np.isin(np.arange(n_child), hit), n_q)
    assert np.array_equal(np.isnan(got_u).all(axis=1), want_u) and np.array_equal(np.isnan(got_u).any(axis=1), want_u)
    assert got_u[~want_u].tobytes() == clean_u[~want_u].tobytes()
    assert np.array_equal(np.isnan(got_q[0]), want_q) and got_q[:, ~want_q].tobytes() == clean_q[:, ~want_q].tobytes()
    with pytest.raises(ValueError):
        fep.transfer_tables('Q1')
    with pytest.raises(ValueError):
        fep.transfer_points_np('Q2', parent, corners, q)


# ---- the driver: refinement in the middle of a load history, on the CPU restatement -------------------------------------------
def test_driver_runs_through_a_refinement(fep):
    import vm_cases as vc
    from vm_ref import VMRefContext
    vm, mesh0 = fep.vonmises, fep.assemble_mesh_el(0, 'P1')
    h = tc.cpu_adaptive_cycle()
    ref = vc.cpu_cycle('P1', 200.0)
    assert h['failed_at'] is None and len(h['adapt']) == 1
    row = h['adapt'][0]
    zetas = list(ref['zeta'])
    assert h['zeta'] == zetas[:4] + [zetas[3]] + zetas[4:] and row['step'] == 3 and row['equilibration'] == 4
    assert (row['n_e'], row['n_n']) == (150, 96) and row['n_child'] == row['elem'].shape[1] > 150 and row['n_marked'] > 0
    assert row['eta'] is None and row['parent'].shape == (row['n_child'],) and row['corners'].shape == (3, row['n_child'])
    n_c = row['coords'].shape[1]
    assert [U.shape for U in h['U']] == [(2, 96)] * 4 + [(2, n_c)] * 13 and len(h['n_plast']) == len(h['newton_its']) == 17
    # before the refinement the run is the plain one's (its load vector is summed elsewhere: equal up to that sum's rounding)
    assert h['n_plast'][:4] == ref['n_plast'][:4]
    assert all(np.abs(a - b).max() <= 1e-13 * np.abs(b).max() for a, b in zip(h['U'][:4], ref['U'][:4]))
    assert h['Ep'].shape == (4, row['n_child']) and np.isfinite(h['Ep']).all() and np.isfinite(h['work']) and h['work'] > 0
    m = h['mesh']
    assert np.array_equal(m['coordinates'], row['coords']) and np.array_equal(m['elements'] - 1, row['elem'])
    assert m['Q'].shape == (2, n_c) and h['f_ext'].shape == (2, n_c)
    assert abs(h['f_ext'][1].sum() - 200.0 * 10.0) <= 1e-12 * 2000.0 and not h['f_ext'][0].any()     # the whole top side, once
    top = m['neumann_nodes'].astype(int)
    assert (m['coordinates'][1, top] == 10.0).all() and top.shape[1] >= 10
    # the transferred state: old vertices keep their displacement, the plastic strain is a copy
    # the transferred state: old vertices keep their displacement, the plastic strain is a copy of the parent's after step 3
    # (the plain run stopped there, on the first segment's own load vector)
    first = fep.solve_cutout_cyclic('P1', level=0, context_factory=VMRefContext, linear_solver='direct', zetas=zetas[:4],
                                    f_ext=vm._p1_traction(mesh0['neumann_nodes'].astype(np.int64), mesh0['coordinates'], np.array([0.0, 200.0])))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(h['U'][:4], first['U']))
    assert np.array_equal(row['U'][:, :96], h['U'][3]) and np.array_equal(row['Ep'], first['Ep'][:, row['parent']])


def test_driver_transferred_state_has_the_parents_stresses(fep):
    from vm_ref import VMRefContext
    gap = tc.stress_gap(tc.cpu_adaptive_cycle()['adapt'][0], VMRefContext)
    print('stress gap on the CPU restatement', gap)
    assert gap <= tc.STRESS_TOL_CPU


def test_driver_without_adapt_at_is_what_it_was(fep):
    """The defaults keep the run: the history of the plain level-0 cycle, pinned when the keywords were added."""
    import vm_cases as vc
    from vm_ref import VMRefContext
    ref = vc.cpu_cycle('P1', 200.0)
    h = fep.solve_cutout_cyclic('P1', level=0, context_factory=VMRefContext, linear_solver='direct', f_ext=vc.top_load('P1', 0, (0, 200.0)),
                                adapt_at=None, mark='zz', theta=0.5)
    assert sorted(h) == sorted(ref) and 'adapt' not in h
    assert h['n_plast'] == ref['n_plast'] == [0, 0, 2, 18, 0, 0, 0, 0, 1, 2, 6, 18, 0, 0, 0, 0]
    assert h['newton_its'] == [2, 2, 6, 6, 3, 2, 2, 2, 5, 6, 6, 6, 3, 2, 2, 2] and h['work'] == ref['work']
    assert abs(h['work'] - 8.910867175891788) <= 1e-9 * 8.910867175891788        # (the literal: another machine's solver may round otherwise)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(h['U'], ref['U'])) and h['Ep'].tobytes() == ref['Ep'].tobytes()


def test_driver_refusals(fep):
    from vm_ref import VMRefContext
    kw = dict(level=0, context_factory=VMRefContext, linear_solver='direct')
    with pytest.raises(ValueError, match='P1'):
        fep.solve_cutout_cyclic('Q1', adapt_at=(3,), mark=tc.near_corner, **kw)
    with pytest.raises(ValueError, match='f_ext'):
        fep.solve_cutout_cyclic('P1', adapt_at=(3,), mark=tc.near_corner, f_ext=np.zeros((2, 96)), **kw)
    with pytest.raises(ValueError, match='adapt_at'):
        fep.solve_cutout_cyclic('P1', adapt_at=(16,), mark=tc.near_corner, **kw)
    with pytest.raises(ValueError, match='mark'):
        fep.solve_cutout_cyclic('P1', adapt_at=(3,), mark='plastic', **kw)


def test_tsx_materials_go_along_on_the_host(fep):
    """solve_tsx_tunnel(adapt=1, transfer_materials=True) with two layers: the next round's arrays are transfer_points_np of
    the round's; without the keyword the refusal stands."""
    from oracle_context import OracleContext
    coord, elem = mc.tunnel()
    upper = coord[1][elem].mean(axis=0) > 0
    mats = (np.where(upper, 25000.0, 30000.0), np.where(upper, 100000.0 / 3, 40000.0), 0.3, 12.0)
    with pytest.raises(ValueError, match='no parent-to-child rule yet'):
        fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, adapt=1, mark=mc.near_tunnel, materials=mats)
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, adapt=1, mark=mc.near_tunnel, materials=mats,
                             transfer_materials=True, n_load_steps=2)
    a, b = h['adapt']
    assert b['n_e'] == a['n_child'] > a['n_e'] and a['corners'].shape == (3, a['n_child'])
    for i in (0, 1):
        want = fep.transfer_points_np('P1', a['parent'], a['corners'], a['materials'][i])
        assert b['materials'][i].tobytes() == want.tobytes() and set(np.unique(want)) == set(np.unique(mats[i]))
    assert b['materials'][2:] == (0.3, 12.0)
    assert np.array_equal(b['materials'][0], a['materials'][0][a['parent']])         # a child is of its parent's layer: the interface stays

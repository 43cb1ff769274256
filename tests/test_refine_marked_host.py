"""
Refinement of marked triangles, host form (midpoints.refine_marked(device=None), mark_plastic) and the adaptive tunnel
driver on the CPU through the oracle context.  The child tables of the hand patterns are written out here; everything else
is checked for conformity (marked_cases.check_conforming) and against counts worked out from the rule.
"""
import numpy as np
import pytest

import marked_cases as mc
from oracle_context import OracleContext


def _rows(elem):
    return [tuple(int(v) for v in col) for col in np.asarray(elem).T]


def _refine(fep, coord, elem, marked, curves=None):
    c, e, p = fep.refine_marked(coord, elem, marked, curves=curves)
    assert c.dtype == np.float64 and e.dtype == np.int64 and p.dtype == np.int64
    assert np.array_equal(c[:, :np.shape(coord)[1]], np.asarray(coord, dtype=float))          # old nodes keep ids and places
    if curves is None:
        mc.check_conforming(np.asarray(coord, dtype=float), np.asarray(elem), mc.marked_boundary_edges(coord, elem, c, e), c, e, p)
    return c, e, p


@pytest.mark.parametrize('slot', [0, 1, 2])
def test_one_triangle_longest_edge_in_every_slot(fep, slot):
    coord = np.array(mc.ONE_TRIANGLE[slot], dtype=float).T
    elem = np.array([[0], [1], [2]])
    assert mc.mp.reference_edges(coord, elem).tolist() == [slot]
    c, e, p = _refine(fep, coord, elem, [1])
    assert _rows(e) == mc.ONE_TRIANGLE_CHILDREN[slot] and p.tolist() == [0, 0, 0, 0]
    # nodes 3, 4, 5 are the midpoints of the edges 1, 2, 0 (the P2 order)
    for node, (a, b) in zip((3, 4, 5), ((1, 2), (2, 0), (0, 1))):
        assert np.array_equal(c[:, node], (coord[:, a] + coord[:, b]) / 2)


def test_pair_marked_from_either_side(fep):
    coord, elem = mc.PAIR_COORD, mc.PAIR_ELEM
    assert mc.mp.reference_edges(coord, elem).tolist() == [1, 1]           # 1-2 for element 0; 3-2 for element 1
    # element 1 marked: its side 2-1 is element 0's longest edge, so element 0 is only bisected: 2 + 4
    c, e, p = _refine(fep, coord, elem, [0, 1])
    assert _rows(e) == [(1, 4, 0), (4, 2, 0), (3, 5, 6), (6, 5, 1), (5, 2, 4), (5, 4, 1)] and p.tolist() == [0, 0, 1, 1, 1, 1]
    # element 0 marked: element 1 gets the node on 2-1, which is not its longest edge: the closure adds 3-2: 4 + 3
    c, e, p = _refine(fep, coord, elem, [1, 0])
    assert _rows(e) == [(1, 4, 6), (6, 4, 0), (4, 2, 5), (4, 5, 0), (3, 7, 1), (7, 2, 4), (7, 4, 1)]
    assert p.tolist() == [0, 0, 0, 0, 1, 1, 1] and c.shape == (2, 8)
    assert np.array_equal(c[:, 7], (coord[:, 3] + coord[:, 2]) / 2)


def test_equilateral_tie_goes_to_slot_0(fep):
    coord = np.array([[0.0, 3.0, 1.5], [0.0, 0.0, 3 * np.sqrt(0.75)]])
    elem = np.array([[0], [1], [2]])
    x, y = coord
    L = [(x[(k + 1) % 3] - x[k]) ** 2 + (y[(k + 1) % 3] - y[k]) ** 2 for k in range(3)]
    assert L[0] == L[1] == L[2]                                          # an exact three-way tie in float64
    assert mc.mp.reference_edges(coord, elem).tolist() == [0]
    assert _rows(_refine(fep, coord, elem, [1])[1]) == mc.ONE_TRIANGLE_CHILDREN[0]


def test_no_marks_is_the_identity(fep):
    coord, elem = mc.tunnel()
    c, e, p = _refine(fep, coord, elem, np.zeros(elem.shape[1], dtype=bool))
    assert np.array_equal(c, coord) and np.array_equal(e, elem) and np.array_equal(p, np.arange(elem.shape[1]))


def test_repeated_and_orphan_nodes_are_left_alone(fep):
    # node 4 repeats node 1's place, node 5 belongs to no element; the two triangles do not share the edge 1-2 / 4-2
    coord = np.array([[0.0, 4.0, 0.0, 9.0, 4.0, 7.0], [0.0, 0.0, 3.0, 3.0, 0.0, 7.0]])
    elem = np.array([[0, 4], [1, 3], [2, 2]])
    c, e, p = _refine(fep, coord, elem, [1, 0])
    # element 0: r = 1 (the edge 1-2), a, b, c = 1, 2, 0; its edges 1, 2, 0 get the nodes 6, 7, 8: m, p, q = 6, 7, 8
    assert _rows(e) == [(1, 6, 8), (8, 6, 0), (6, 2, 7), (6, 7, 0), (4, 3, 2)] and p.tolist() == [0, 0, 0, 0, 1]
    assert np.array_equal(c[:, :6], coord) and c.shape == (2, 9)


def test_wrong_inputs_raise(fep):
    coord, elem = mc.PAIR_COORD, mc.PAIR_ELEM
    with pytest.raises(ValueError, match='one entry per element'):
        fep.refine_marked(coord, elem, [1])
    with pytest.raises(ValueError, match='same way'):
        fep.refine_marked(coord, np.array([[0, 1], [1, 2], [2, 3]]), [1, 0])           # both walk 1 -> 2


@pytest.mark.parametrize('name', ['tunnel', 'unstructured'])
def test_all_marked_gives_uniform_refinements_nodes(fep, name):
    coord, elem = mc.tunnel() if name == 'tunnel' else mc.unstructured()
    c, e, p = _refine(fep, coord, elem, np.ones(elem.shape[1], dtype=bool))
    cu, eu = fep.refine_uniform(coord, elem)
    assert c.shape == cu.shape and np.array_equal(c, cu)
    assert e.shape[1] == 4 * elem.shape[1] and c.shape[1] - coord.shape[1] == len(mc.mp._edge_map(elem))
    assert np.array_equal(p, np.repeat(np.arange(elem.shape[1]), 4))


def test_all_marked_with_the_tunnel_wall(fep):
    coord, elem = mc.tunnel()
    hole = [fep.tsx_tunnel.TSX_HOLE]
    c, e, p = _refine(fep, coord, elem, np.ones(elem.shape[1], dtype=bool), curves=hole)
    cu, eu = fep.refine_uniform(coord, elem, curves=hole)
    assert np.array_equal(c, cu) and not np.array_equal(c, fep.refine_uniform(coord, elem)[0])
    moved = np.flatnonzero((c != fep.refine_uniform(coord, elem)[0]).any(axis=0))
    h = hole[0]
    g = np.sqrt(((c[0, moved] - h.cx) / h.a) ** 2 + ((c[1, moved] - h.cy) / h.b) ** 2)
    assert moved.size == 25 and np.abs(g - 1).max() <= 4 * np.finfo(float).eps
    assert (mc.mp.doubled_areas(c, e) > 0).all()


def test_a_child_folded_by_the_curve_is_refused(fep):
    c, e, p = _refine(fep, mc.FOLD_COORD, mc.FOLD_ELEM, [1])                              # straight: fine
    assert e.shape[1] == 4
    with pytest.raises(ValueError, match='non-positive area'):
        fep.refine_marked(mc.FOLD_COORD, mc.FOLD_ELEM, [1], curves=[fep.Ellipse(0.0, 0.0, 1.0, 1.0)])


def test_closure_chain(fep):
    coord, elem = mc.chain()
    ref = mc.mp.reference_edges(coord, elem)
    nbr = mc.mp._half_edges(elem)[0]
    assert all(nbr[ref[k], k] // 3 == k + 1 for k in range(599))                     # longest edge = the one shared with the next
    first = np.zeros(600, dtype=bool)
    first[0] = True
    c, e, p = _refine(fep, coord, elem, first)
    assert c.shape[1] - coord.shape[1] == 602 and e.shape[1] == 1801 == 4 + 598 * 3 + 3
    last = np.zeros(600, dtype=bool)
    last[599] = True
    c, e, p = _refine(fep, coord, elem, last)
    assert c.shape[1] - coord.shape[1] == 3 and e.shape[1] == 604


def test_chained_rounds_keep_the_angle_bound(fep):
    coord, elem = mc.perturbed_square()
    assert elem.shape[1] == 72
    angle0, area0 = mc.smallest_angle(coord, elem), mc.mp.doubled_areas(coord, elem).sum() / 2
    rng = np.random.default_rng(11)
    for rnd in range(1, 13):
        coord, elem, parent = _refine(fep, coord, elem, mc.round_marks(rnd, elem, rng))
        assert mc.smallest_angle(coord, elem) >= angle0 / 2, rnd                    # Rosenberg-Stenger / Rivara
        assert abs(mc.mp.doubled_areas(coord, elem).sum() / 2 - area0) <= mc.total_area_bound(coord, elem.shape[1] + 72), rnd
    assert elem.shape[1] > 5000


# ---- mark_plastic -----------------------------------------------------------------------------------------------------------
#  5 - 6 - 7 - 8 - 9      a row of four cells (vertex numbers of the P1 form): cell c holds the elements 2 c = (c, c + 1, c + 5)
#  | / | / | / | / |      and 2 c + 1 = (c + 1, c + 6, c + 5)
#  0 - 1 - 2 - 3 - 4
def _strip(fep, t):
    m = fep.rect_mesh(4, 1, t, 4.0, 1.0)                                         # 8 triangles in a row
    return np.asarray(m['elements'])


@pytest.mark.parametrize('t,n_q', [('P1', 1), ('P2', 7)])
def test_mark_plastic_rings(fep, t, n_q):
    elem = _strip(fep, t)
    assert elem.shape[1] == 8
    flags = np.zeros(8 * n_q, dtype=bool)
    flags[0 * n_q + n_q - 1] = True                                              # the last point of element 0
    got = {r: set(np.flatnonzero(fep.mark_plastic(flags, elem, n_q, rings=r)).tolist()) for r in (0, 1, 2)}
    # vertex adjacency of the row, worked out from the element table itself: ring r = elements within r vertex-steps
    share = [[bool(set(elem[:3, i]) & set(elem[:3, j])) for j in range(8)] for i in range(8)]
    ring1 = {j for j in range(8) if share[0][j]}
    ring2 = {j for j in range(8) if any(share[i][j] for i in ring1)}
    assert got[0] == {0} and got[1] == ring1 and got[2] == ring2
    # element 0 = (0, 1, 5) meets 1 and 2 at the vertices 1 and 5 (3 = (2, 7, 6) has none of them); those reach 3 and 4
    assert got[1] == {0, 1, 2} and got[2] == {0, 1, 2, 3, 4}
    assert fep.mark_plastic(flags, elem, n_q).dtype == bool and got[1] == set(np.flatnonzero(fep.mark_plastic(flags, elem, n_q)).tolist())
    assert not fep.mark_plastic(np.zeros(8 * n_q), elem, n_q, rings=2).any()
    with pytest.raises(ValueError):
        fep.mark_plastic(flags[:-1], elem, n_q)


# ---- the driver -------------------------------------------------------------------------------------------------------------
def test_driver_adapt_on_the_oracle_context(fep):
    coord, elem = mc.tunnel()
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, adapt=2, mark=mc.near_tunnel)
    rounds = h['adapt']
    assert len(rounds) == 3 and len(h['zeta']) == 17
    assert rounds[0]['n_e'] == 887 and rounds[0]['n_n'] == coord.shape[1]
    assert abs(rounds[0]['displ'] - (-0.0019794496707526746)) <= 1e-10 * 0.0019794496707526746    # round 0 is the plain run
    for a, b in zip(rounds[:-1], rounds[1:]):
        assert a['n_child'] == b['n_e'] > a['n_e'] and a['n_marked'] == int(a['marked'].sum()) > 0
        assert np.bincount(a['parent'], minlength=a['n_e'])[a['marked']].min() >= 2
    assert rounds[-1]['n_marked'] is None and rounds[-1]['displ'] == h['displ'][-1]
    assert h['elem'].shape == (3, rounds[-1]['n_e']) and h['coords'].shape == (2, rounds[-1]['n_n'])
    assert np.array_equal(h['coords'][:, :coord.shape[1]], coord)                 # old nodes keep their ids
    n_bnd0 = len(mc.boundary_edges(elem))
    assert mc.edge_counts(h['elem'])[2:] == (0, 0, 0) and mc.edge_counts(h['elem'])[1] > n_bnd0
    # renumbered on every round: the monitor and node_of_input follow the input's nodes; the same mesh up to numbering
    r = fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, adapt=1, mark=mc.near_tunnel, renumber=True)
    assert np.array_equal(r['coords'][:, r['node_of_input']], coord)
    assert [row['n_e'] for row in r['adapt']] == [row['n_e'] for row in rounds[:2]]
    assert abs(r['adapt'][0]['displ'] - rounds[0]['displ']) <= 1e-10 * abs(rounds[0]['displ'])
    assert abs(r['adapt'][1]['displ'] - rounds[1]['displ']) <= 1e-10 * abs(rounds[1]['displ'])
    with pytest.raises(ValueError, match='parent-to-child'):
        fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, adapt=1,
                             materials=(np.full(887, 25000.0), 33333.0, 0.5, 10.0))

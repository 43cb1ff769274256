"""
Closed-form elasticity for tests/test_exact_solutions_host.py (the oracle) and tests/test_exact_solutions_gpu.py (the
product): the cases, their meshes, the error metrics, the order rule and every case's measured values.  No GPU and no
library call here: the mesh functions, the stiffness matrix and the load vector are handed in by the two test files.

Every other reference of the suite restates the formulas the kernels implement.  This one does not: a thick-walled cylinder
under internal pressure in plane strain (Lame) has the displacement
    u = u_r(r) e_r,    u_r = (1 + nu) / E ((1 - 2 nu) A r + B / r),    A = p a^2 / (b^2 - a^2),    B = A b^2,
with sigma_rr(a) = -p, so the traction on the inner wall is p e_r.  The field has no body force, so its restriction to any
domain that leaves out the axis is the solution of the Dirichlet problem with its own boundary values: the straight
square [1, 2]^2 and the unit square at distance from the axis use that.  A finite-element method of degree k converges to
it at the order k in the energy norm and k + 1 at the nodes; tables, numbering, curved-boundary rule or assembly that are
wrong in a way every restatement shares show as a lower order.

Cases (CASES): a = 1, b = 2.5, p = 7, E = 1000, nu = 0.3.
  ring    the hexagonal ring of twelve triangles between the circles r = a and r = b about (0.3, -0.2), refined with
          refine_uniform(curves=) and raised with create_midpoints(curves=); 'Dirichlet' (exact u on both walls) or 'pressure'
          (p e_r on the inner wall through the traction vector, exact u on the outer wall)
  ring5   the same with one sector missing: two straight radial boundary edges between the curves, which carry exact u
  square  [1, 2]^2 (axis at the origin) cut into four triangles by its centre and refined: straight sides, exact u all round
  rect    rect_mesh(n, n) on the unit square, axis at (-1, -1), exact u all round; Q1 and Q2, Q2 also with the true 3 x 3 Gauss
          points passed as tables

Metrics: `max` = the largest nodal error over max |u|; `energy` = the K-norm of U minus the nodal values of u over the K-norm
of those nodal values.  Order = log2 of the ratio between two successive levels.

The order rule (`rule`): at the finest pair of levels, energy order >= k - 0.3 and max order >= k + 0.2, k the polynomial
degree.  The one exception is Q2 with the default tables, whose quadrature (the 3 x 3 Gauss weights at the 2 x 2 points
+-1/sqrt(3), kept from the reference: tables.get_quadrature_volume) is not a rule for its weights: the element is first
order, less accurate than Q1, and only energy >= 0.8, max >= 1.5 is asked of it (measured 0.96 and 1.80).

MEASURED holds, per case, what the host test found on the oracle: the orders at the finest pair, the errors at the finest
level and the sensitivity (the largest relative change of U when every value of K moves by one unit of rounding, the
practice of solver_cases.perturbed).  The host test asserts that it finds these figures; the GPU test takes its bound on
|U_gpu - U_oracle| from the sensitivity.  PATCH holds the worst strain and interior-force ratios of the patch test.
"""
import numpy as np
import scipy.sparse as ssp
import scipy.sparse.linalg as spla

A_IN, B_OUT, PRESSURE, YOUNG, NU = 1.0, 2.5, 7.0, 1000.0, 0.3
SHEAR, BULK = YOUNG / (2 * (1 + NU)), YOUNG / (3 * (1 - 2 * NU))
RING_CENTRE = (0.3, -0.2)
U_RND = 2.0 ** -53

DEGREE = {'P1': 1, 'P2': 2, 'Q1': 1, 'Q2': 2, 'P4': 4}

# name: kind, element type, load, levels (ring / square: refinements; rect: cells per side), tables
CASES = {
    'P1 ring, Dirichlet':   dict(kind='ring', et='P1', load='dirichlet', levels=(1, 2, 3, 4, 5)),         # level 0 has no free node
    'P1 ring, pressure':    dict(kind='ring', et='P1', load='pressure', levels=(0, 1, 2, 3, 4, 5)),
    'P2 ring, Dirichlet':   dict(kind='ring', et='P2', load='dirichlet', levels=(0, 1, 2, 3, 4)),
    'P2 ring, pressure':    dict(kind='ring', et='P2', load='pressure', levels=(0, 1, 2, 3, 4)),
    'P4 ring, Dirichlet':   dict(kind='ring', et='P4', load='dirichlet', levels=(0, 1, 2, 3, 4)),
    'P4 ring, pressure':    dict(kind='ring', et='P4', load='pressure', levels=(0, 1, 2, 3, 4)),
    'P1 ring5, pressure':   dict(kind='ring5', et='P1', load='pressure', levels=(0, 1, 2, 3, 4, 5)),
    'P2 ring5, pressure':   dict(kind='ring5', et='P2', load='pressure', levels=(0, 1, 2, 3, 4)),
    'P4 ring5, Dirichlet':  dict(kind='ring5', et='P4', load='dirichlet', levels=(0, 1, 2, 3, 4)),
    'P4 ring5, pressure':   dict(kind='ring5', et='P4', load='pressure', levels=(0, 1, 2, 3, 4)),
    'P1 square':            dict(kind='square', et='P1', load='dirichlet', levels=(0, 1, 2, 3)),
    'P2 square':            dict(kind='square', et='P2', load='dirichlet', levels=(0, 1, 2, 3)),
    'P4 square':            dict(kind='square', et='P4', load='dirichlet', levels=(0, 1, 2, 3)),
    'Q1 rect':              dict(kind='rect', et='Q1', load='dirichlet', levels=(2, 4, 8, 16, 32)),
    'Q2 rect':              dict(kind='rect', et='Q2', load='dirichlet', levels=(2, 4, 8, 16, 32)),
    'Q2 rect, Gauss':       dict(kind='rect', et='Q2', load='dirichlet', levels=(2, 4, 8, 16, 32), tables='gauss'),
}
for _c in CASES.values():
    _c.setdefault('tables', 'default')

# Per case, on the oracle (test_exact_solutions_host.py asserts them: orders to 0.05, errors and sensitivity to a factor of two):
# (max order, energy order) at the finest pair, (max error, energy error) at the finest level, sensitivity of U.
MEASURED = {
    'P1 ring, Dirichlet': ((1.83, 1.88), (7.95e-04, 2.25e-03), 1.6e-14),
    'P1 ring, pressure': ((1.42, 1.55), (5.23e-03, 9.36e-03), 3.5e-14),
    'P2 ring, Dirichlet': ((2.53, 2.49), (9.95e-05, 7.69e-04), 1.7e-14),
    'P2 ring, pressure': ((2.71, 2.58), (3.15e-04, 1.22e-03), 7.0e-14),
    'P4 ring, Dirichlet': ((4.48, 3.95), (2.19e-07, 4.20e-06), 7.2e-14),
    'P4 ring, pressure': ((4.65, 3.99), (2.47e-07, 4.36e-06), 4.8e-13),
    'P1 ring5, pressure': ((1.50, 1.58), (5.23e-03, 9.03e-03), 5.6e-14),
    'P2 ring5, pressure': ((2.88, 2.58), (3.15e-04, 1.20e-03), 4.8e-14),
    'P4 ring5, Dirichlet': ((4.48, 3.95), (2.19e-07, 4.20e-06), 5.0e-14),
    'P4 ring5, pressure': ((4.61, 3.99), (2.54e-07, 4.35e-06), 3.0e-13),
    'P1 square': ((1.69, 1.87), (1.65e-03, 5.38e-03), 1.5e-15),
    'P2 square': ((2.87, 2.48), (1.54e-05, 2.37e-04), 3.8e-15),
    'P4 square': ((4.65, 3.98), (1.82e-08, 3.84e-07), 1.5e-14),
    'Q1 rect': ((2.01, 1.99), (1.20e-05, 6.44e-05), 6.1e-15),
    'Q2 rect': ((1.80, 0.96), (2.43e-04, 8.66e-03), 8.7e-15),
    'Q2 rect, Gauss': ((3.80, 2.95), (4.66e-08, 2.93e-06), 3.0e-14),
}

# Patch test, per case of patch_names(): (worst strain ratio to u S_E, worst interior-force ratio to u S_F) on the oracle.
# The force ratios of P2 and P4 are in the thousands because the reference's quadrature tables carry 13 and 15 digits (and P4's
# a digit typo, tables.get_quadrature_volume): the rule integrates the constant stress to 1e-13 and 2e-12, not to rounding.
# The distorted Q2 meshes run on the Gauss tables: with the default rule Q2 fails the patch test on any element that is not
# a parallelogram (test_exact_solutions_host.py: test_default_q2_fails_the_patch_test_on_distorted_elements).
PATCH = {
    'P1 ring': (3.55, 6.13),
    'P1 ring5': (3.55, 4.70),
    'P1 square': (1.43, 24.96),
    'P2 ring': (9.02, 1084.14),
    'P2 ring5': (9.02, 1084.14),
    'P2 square': (7.18, 906.95),
    'P4 ring': (8.04, 16515.79),
    'P4 ring5': (8.04, 16515.79),
    'P4 square': (3.67, 15712.85),
    'Q1 rect': (2.39, 5.96),
    'Q2 rect': (6.90, 17.17),
    'P1 curved': (16.93, 37.75),
    'P1 delaunay': (14.62, 50.54),
    'P1 renumbered': (14.32, 60.58),
    'P1 mixed': (14.32, 63.30),
    'P2 curved': (22.41, 1364.21),
    'P2 delaunay': (33.87, 1159.44),
    'P2 renumbered': (34.19, 1264.37),
    'P2 mixed': (34.19, 1255.29),
    'P4 curved': (33.36, 21236.84),
    'P4 delaunay': (33.91, 16506.08),
    'P4 renumbered': (17.70, 19290.86),
    'P4 mixed': (16.03, 19112.33),
    'Q1 curved': (22.14, 33.82),
    'Q1 renumbered': (23.39, 41.19),
    'Q1 mixed': (19.53, 34.24),
    'Q2 curved': (17.27, 50.95),
    'Q2 renumbered': (17.99, 48.46),
    'Q2 mixed': (17.37, 39.69),
}


# ---- the fields ------------------------------------------------------------------------------------------------------------
def lame(coord, centre):
    """The Lame displacement (2, n) at the points `coord` (2, n) for the axis `centre`."""
    dx, dy = coord[0] - centre[0], coord[1] - centre[1]
    r = np.hypot(dx, dy)
    A = PRESSURE * A_IN ** 2 / (B_OUT ** 2 - A_IN ** 2)
    B = A * B_OUT ** 2
    ur = (1 + NU) / YOUNG * ((1 - 2 * NU) * A * r + B / r)
    return np.stack([ur * dx / r, ur * dy / r])


LIN = ((2e-3, 1.5e-3, -0.7e-3), (-1e-3, 0.4e-3, 1.1e-3))                    # u_c = LIN[c][0] + LIN[c][1] x + LIN[c][2] y
LIN_STRAIN = (LIN[0][1], LIN[1][2], LIN[0][2] + LIN[1][1])                  # (e11, e22, engineering e12)


def linear(coord):
    x, y = coord
    return np.stack([LIN[c][0] + LIN[c][1] * x + LIN[c][2] * y for c in range(2)])


def linear_stress():
    """(s11, s22, s12) of LIN_STRAIN in plane strain."""
    e11, e22, g12 = LIN_STRAIN
    tr = e11 + e22
    return (BULK * tr + 2 * SHEAR * (e11 - tr / 3), BULK * tr + 2 * SHEAR * (e22 - tr / 3), SHEAR * g12)


# ---- tables ----------------------------------------------------------------------------------------------------------------
def q2_gauss_tables(fep):
    """(dhatp1, dhatp2, wf) of Q2 at the true 3 x 3 Gauss points +-sqrt(3/5), 0, in the order and with the weights of the
    default rule, from tables.get_local_basis_volume."""
    g = np.sqrt(3 / 5)
    xi = np.array([[-g, g, g, -g, 0, g, 0, -g, 0], [-g, -g, g, g, -g, 0, g, 0, 0]])
    _, d1, d2 = fep.get_local_basis_volume('Q2', xi)
    wc, we, wm = 25 / 81, 40 / 81, 64 / 81
    return (np.ascontiguousarray(d1, dtype=np.float64), np.ascontiguousarray(d2, dtype=np.float64),
            np.array([wc, wc, wc, wc, we, we, we, we, wm]))


def tables(fep, case):
    return q2_gauss_tables(fep) if case['tables'] == 'gauss' else fep.element_tables(case['et'])


EDGE_NODES = {'P1': (-1, 1), 'P2': (-1, 1, 0), 'P4': (-1, 1, 0, 0.5, -0.5)}     # surf's (B, A[, mid[, quarter nearer A, nearer B]])
EDGE_POINTS = {'P1': 3, 'P2': 4, 'P4': 6}                                    # Gauss points per edge: one more than its nodes


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def ring_base(fep, sectors):
    """curved_cases._ring with circles: (coord, elem, curves)."""
    cx, cy = RING_CENTRE
    inner, outer = fep.Ellipse(cx, cy, A_IN, A_IN, 1e-9), fep.Ellipse(cx, cy, B_OUT, B_OUT, 1e-9)
    th = np.pi / 3 * np.arange(6)
    coord = np.concatenate([[cx + A_IN * np.cos(th), cy + A_IN * np.sin(th)],
                            [cx + B_OUT * np.cos(th), cy + B_OUT * np.sin(th)]], axis=1)
    el = []
    for i in sectors:
        j = (i + 1) % 6
        el += [(i, 6 + i, 6 + j), (i, 6 + j, j)]
    return np.ascontiguousarray(coord), np.array(el, dtype=np.int64).T.copy(), [inner, outer]


def square_base():
    coord = np.array([[1.0, 2.0, 2.0, 1.0, 1.5], [1.0, 1.0, 2.0, 2.0, 1.5]])
    return coord, np.array([[0, 1, 2, 3], [1, 2, 3, 0], [4, 4, 4, 4]], dtype=np.int64), None


def mesh(fep, kind, et, level, device=None):
    """-> dict(elem, coord, centre, fixed (n_n,) bool per load, edges of the inner wall).  Triangles: refine_uniform and
    create_midpoints on the host (device=None) or on GPU `device`.  'surf' columns are (B, A[, nodes between]); the inner
    wall is curve 0."""
    if kind == 'rect':
        m = fep.rect_mesh(level, level, et, 1.0, 1.0)
        elem, coord = np.ascontiguousarray(m['elements'], dtype=np.int64), np.ascontiguousarray(m['coordinates'], dtype=np.float64)
        x, y = coord
        on = (x == 0) | (x == 1) | (y == 0) | (y == 1)
        return dict(elem=elem, coord=coord, centre=(-1.0, -1.0), fixed={'dirichlet': on}, wall=None, boundary=on)
    coord, elem, curves = square_base() if kind == 'square' else ring_base(fep, range(6) if kind == 'ring' else range(5))
    centre = (0.0, 0.0) if kind == 'square' else RING_CENTRE
    c1, e1 = fep.refine_uniform(coord, elem, levels=level, device=device, curves=curves)
    h = fep.create_midpoints('P2' if et == 'P1' else et, c1, e1, device=device, curves=curves)
    if et == 'P1':
        elem, coord, surf = e1, c1, h['surf'][:2].astype(np.int64)
    else:
        elem, coord, surf = h['elem_ext'].astype(np.int64), h['coord_ext'], h['surf'].astype(np.int64)
    sc = h['surf_curve'] if curves else np.full(surf.shape[1], -1, dtype=np.int64)
    n_n = coord.shape[1]
    on = np.zeros(n_n, dtype=bool)
    on[surf.ravel()] = True
    not_wall = np.zeros(n_n, dtype=bool)
    not_wall[surf[:, sc != 0].ravel()] = True
    return dict(elem=np.ascontiguousarray(elem, dtype=np.int64), coord=np.ascontiguousarray(coord, dtype=np.float64),
                centre=centre, fixed={'dirichlet': on, 'pressure': not_wall}, wall=np.ascontiguousarray(surf[:, sc == 0]),
                boundary=on, surf=surf, surf_curve=sc)


def check_mesh(case, level, m):
    """What both test files ask of a mesh before they use it: the sizes, positive orientation at the vertices, every
    boundary node of a wall on its circle, the inner wall closed (ring) or open at the two radial edges (ring5)."""
    kind, et = case['kind'], case['et']
    elem, coord = m['elem'], m['coord']
    assert np.isfinite(coord).all() and elem.min() == 0 and elem.max() == coord.shape[1] - 1
    assert np.unique(elem).size == coord.shape[1]
    if kind == 'rect':
        assert elem.shape == ({'Q1': 4, 'Q2': 8}[et], level * level)
        assert int(m['boundary'].sum()) == 4 * level * (1 if et == 'Q1' else 2)
        return
    n0 = {'ring': 12, 'ring5': 10, 'square': 4}[kind]
    assert elem.shape == ({'P1': 3, 'P2': 6, 'P4': 15}[et], n0 * 4 ** level)
    x, y = coord
    d = (x[elem[1]] - x[elem[0]]) * (y[elem[2]] - y[elem[0]]) - (x[elem[2]] - x[elem[0]]) * (y[elem[1]] - y[elem[0]])
    assert d.min() > 0
    per_edge = {'P1': 1, 'P2': 2, 'P4': 4}[et]
    if kind == 'square':
        assert m['wall'].shape[1] == 0 and int(m['boundary'].sum()) == 4 * 2 ** level * per_edge
        assert abs(d.sum() / 2 - 1.0) <= 1e-13
        return
    sc, surf = m['surf_curve'], m['surf']
    n_wall = (6 if kind == 'ring' else 5) * 2 ** level
    assert (sc == 0).sum() == n_wall and (sc == 1).sum() == n_wall and (sc == -1).sum() == (0 if kind == 'ring' else 2 * 2 ** level)
    r = np.hypot(x - RING_CENTRE[0], y - RING_CENTRE[1])
    assert np.abs(r[surf[:, sc == 0]] - A_IN).max() <= 8 * U_RND * B_OUT
    assert np.abs(r[surf[:, sc == 1]] - B_OUT).max() <= 8 * U_RND * B_OUT
    assert m['wall'].shape == (surf.shape[0], n_wall)
    assert int(m['fixed']['pressure'].sum()) == int(m['boundary'].sum()) - (n_wall * per_edge if kind == 'ring' else n_wall * per_edge - 1)


def wall_traction(m, et):
    """(edges, t_int (2, n_e_s * n_q_s), tables) of p e_r on the inner wall: e_r at each surface point of the edge's own
    polynomial, tables from loads_exact.edge_tables."""
    import loads_exact
    hat, dhat, wf = loads_exact.edge_tables(EDGE_NODES[et], EDGE_POINTS[et])
    edges = m['wall']
    px = np.einsum('aq,ae->eq', hat, m['coord'][0][edges]) - m['centre'][0]
    py = np.einsum('aq,ae->eq', hat, m['coord'][1][edges]) - m['centre'][1]
    r = np.hypot(px, py)
    t = PRESSURE * np.stack([(px / r).ravel(), (py / r).ravel()])
    return edges, np.ascontiguousarray(t), (hat, dhat, wf)


# ---- solve and measure -----------------------------------------------------------------------------------------------------
def dof_mask(node_mask):
    return np.repeat(node_mask, 2)


def flat(u):
    return np.ascontiguousarray(u.T).ravel()


def solve(K, m, load, f_wall=None):
    """Dirichlet lifting and SciPy LU on the free DOFs -> U (n_dof,) in DOF order.  `f_wall` (2, n_n): the traction vector."""
    K = ssp.csr_matrix(K)
    fixed = dof_mask(m['fixed'][load])
    u_ex = flat(lame(m['coord'], m['centre']))
    U = np.where(fixed, u_ex, 0.0)
    f = np.zeros(U.size) if f_wall is None else flat(np.asarray(f_wall))
    free = np.flatnonzero(~fixed)
    rhs = (f - K @ U)[free]
    U[free] = spla.splu(ssp.csc_matrix(K[free][:, free])).solve(rhs)
    return U


def lifted_rhs(K, m, load, f_wall=None):
    """(free-DOF mask, right-hand side with zeros on the fixed DOFs, the lifting U_D) of `solve`, for a device solver."""
    K = ssp.csr_matrix(K)
    fixed = dof_mask(m['fixed'][load])
    U = np.where(fixed, flat(lame(m['coord'], m['centre'])), 0.0)
    f = np.zeros(U.size) if f_wall is None else flat(np.asarray(f_wall))
    return ~fixed, np.where(fixed, 0.0, f - K @ U), U


def errors(K, m, U):
    """(max, energy): the two metrics of the module docstring."""
    u = flat(lame(m['coord'], m['centre']))
    e = U - u
    return float(np.abs(e).max() / np.abs(u).max()), float(np.sqrt((e @ (K @ e)) / (u @ (K @ u))))


def perturbed(K, seed=23):
    """solver_cases.perturbed: every value times 1 + 2.2e-16 uniform(-1, 1)."""
    Kp = ssp.csr_matrix(K, copy=True)
    Kp.data = Kp.data * (1.0 + 2.2e-16 * np.random.default_rng(seed).uniform(-1.0, 1.0, Kp.data.size))
    return Kp


def orders(errs):
    """[(max order, energy order)] between successive levels of [(max, energy)]."""
    return [(float(np.log2(a[0] / b[0])), float(np.log2(a[1] / b[1]))) for a, b in zip(errs[:-1], errs[1:])]


def rule(name):
    """(least max order, least energy order) at the finest pair of levels."""
    c = CASES[name]
    if c['et'] == 'Q2' and c['tables'] == 'default':
        return 1.5, 0.8
    k = DEGREE[c['et']]
    return k + 0.2, k - 0.3


def bound(name):
    """The GPU test's bound on relerr(U_gpu, U_oracle): 30 x the case's sensitivity, never above 1e-9."""
    return min(30.0 * MEASURED[name][2], 1e-9)


# ---- patch test ------------------------------------------------------------------------------------------------------------
PATCH_DISTORTED = {'P1': ('curved', 'delaunay', 'renumbered', 'mixed'), 'P2': ('curved', 'delaunay', 'renumbered', 'mixed'),
                   'P4': ('curved', 'delaunay', 'renumbered', 'mixed'), 'Q1': ('curved', 'renumbered', 'mixed'),
                   'Q2': ('curved', 'renumbered', 'mixed')}


def patch_names():
    out = []
    for et in ('P1', 'P2', 'P4'):
        out += [f'{et} ring', f'{et} ring5', f'{et} square']
    out += ['Q1 rect', 'Q2 rect']
    for et, names in PATCH_DISTORTED.items():
        out += [f'{et} {n}' for n in names]
    return tuple(out)


def patch_mesh(fep, name, device=None):
    """(elem, coord, interior-node mask) of a patch-test mesh: ring and ring5 at level 1 (curved as P2 and P4), the square at
    level 2, rect_mesh(4, 4), and the distorted meshes of meshes.named (seed 5; their boundary is the box [0, 10]^2)."""
    import meshes
    et, kind = name.split()
    if kind in ('ring', 'ring5', 'square', 'rect'):
        m = mesh(fep, kind, et, 4 if kind == 'rect' else (2 if kind == 'square' else 1), device=device)
        return m['elem'], m['coord'], ~m['boundary']
    elem, coord = meshes.named(et, kind, np.random.default_rng(5))[:2]
    x, y = coord
    return (np.ascontiguousarray(elem, dtype=np.int64), np.ascontiguousarray(coord, dtype=np.float64),
            ~((x == 0) | (x == 10) | (y == 0) | (y == 10)))


def patch_tables(fep, name):
    """The tables of a patch-test case: the default ones, but the Gauss tables for Q2 on the distorted meshes."""
    et, kind = name.split()
    return q2_gauss_tables(fep) if et == 'Q2' and kind != 'rect' else fep.element_tables(et)


def patch_ratios(elem, coord, tabs, inner, E, F):
    """(worst strain ratio, worst interior-force ratio): |E - LIN_STRAIN| over u S_E at every point, |F| over u S_F at every
    DOF of an interior node, with ElemRef's scales for the linear field and its stress."""
    from elem_ref import ElemRef, ratio
    ref = ElemRef(elem, coord, tabs)
    _, S_E = ref.strain(linear(coord))
    s = np.repeat(np.array(linear_stress())[:, None], ref.n_int, axis=1)
    _, _, _, S_F = ref.assemble(s=s)
    want = np.repeat(np.array(LIN_STRAIN)[:, None], ref.n_int, axis=1)
    dofs = dof_mask(inner)
    return ratio(np.asarray(E)[:3], want, S_E), ratio(np.asarray(F)[dofs], np.zeros(int(dofs.sum())), S_F[dofs])

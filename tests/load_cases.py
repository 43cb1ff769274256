"""
Inputs shared by tests/test_loads_exact_host.py and tests/test_loads_shapes_gpu.py: the edge lists, tables and tractions
at which load_traction_kernel can go wrong (more than one workgroup, ragged last block, 4- and 5-node edges, 8 surface
points, curved walls away from the origin, shuffled / repeated / reversed edges, a hub of high degree, ids at both ends of
a large array, nothing at all), the meshes for load_volume_kernel, and the bound on the total of a pressure load on a closed
loop.  Everything is generated on the host (the mesh routines with device=None) from fixed seeds, so both files see the
same bytes.  The high-precision values of a traction case are computed once per process (`exact`).
"""
import functools

import numpy as np

import curved_cases
import fan_mesh
import loads_exact as lx
from conftest import load_golden

U = lx.U
CENTRE, RADIUS = (30.0, -20.0), 40.0
NODES = {2: (-1, 1), 3: lx.P2_NODES, 4: lx.P3_NODES, 5: lx.P4_NODES}


class Case:
    """One traction input.  edges (n_p_s, n_e_s) int64, coord (2, n_n), t_int (2, n_e_s n_q_s), tables h / dh / wf;
    pressure = p when t_int is the uniform pressure p (j2, -j1) / |J|; closed: the edges form closed loops;
    sorted_edges / sorted_t: the same load in the unshuffled order (or None)."""

    def __init__(self, name, edges, coord, t_int, n_q, pressure=None, closed=False, sorted_edges=None, sorted_t=None):
        self.name = name
        self.edges = np.ascontiguousarray(edges, dtype=np.int64)
        self.coord = np.ascontiguousarray(coord, dtype=np.float64)
        self.n_p_s, self.n_e_s = self.edges.shape
        self.n_n = self.coord.shape[1]
        self.nodes_xi = NODES[self.n_p_s]
        self.h, self.dh, self.wf = _tables(self.n_p_s, n_q)
        self.n_q_s = n_q
        self.t_int = np.ascontiguousarray(t_int, dtype=np.float64).reshape(2, self.n_e_s * n_q)
        self.pressure, self.closed = pressure, closed
        self.sorted_edges, self.sorted_t = sorted_edges, sorted_t

    def args(self):
        return self.edges, self.coord, self.t_int, self.h, self.dh, self.wf


@functools.lru_cache(maxsize=None)
def _tables(n_p_s, n_q):
    return lx.edge_tables(NODES[n_p_s], n_q)


def float_jacobian(edges, coord, dh):
    """(j1, j2) (n_e_s, n_q_s) in float64 from the test's own tables: what a caller computes to set up a pressure."""
    j = []
    for c in range(2):
        x = coord[c][edges]                                                 # (n_p_s, n_e_s)
        acc = np.zeros((edges.shape[1], dh.shape[1]))
        for a in range(edges.shape[0]):
            acc += x[a][:, None] * dh[a][None, :]
        j.append(acc)
    return j


def pressure_field(edges, coord, dh, p):
    """t = p (j2, -j1) / |J| per surface point -> (2, n_e_s n_q_s)."""
    j1, j2 = float_jacobian(edges, coord, dh)
    J = np.sqrt(j1 * j1 + j2 * j2)
    return np.stack([(p * j2 / J).ravel(), (p * -j1 / J).ravel()])


def _with_load(name, edges, coord, n_q, rng, kind, closed=False, shuffle=False):
    """A Case with a random traction or the pressure 3.5; `shuffle`: the edges (and their tractions) in random order, the
    given order kept beside."""
    edges = np.asarray(edges, dtype=np.int64)
    n_p_s, n_e_s = edges.shape
    if kind == 'pressure':
        t = pressure_field(edges, coord, _tables(n_p_s, n_q)[1], 3.5)
    else:
        t = rng.uniform(-2.0, 2.0, size=(2, n_e_s * n_q))
    if not shuffle:
        return Case(f'{name}, {n_q}-point, {kind}', edges, coord, t, n_q, 3.5 if kind == 'pressure' else None, closed)
    perm = rng.permutation(n_e_s)
    ts = t.reshape(2, n_e_s, n_q)[:, perm].reshape(2, -1)
    return Case(f'{name}, {n_q}-point, {kind}, shuffled', edges[:, perm], coord, ts, n_q, 3.5 if kind == 'pressure' else None,
                closed, sorted_edges=edges, sorted_t=t)


def _arc(n_edges, n_p_s, rng, spare=37):
    """An open polyline of n_edges edges of n_p_s nodes each on the circle, every node ON the circle at the parameter of
    its reference position, the node ids a random subset of a larger array in random order (bnode[b] != b, unloaded nodes
    in between)."""
    n_loaded = n_edges * (n_p_s - 1) + 1
    n_n = n_loaded + spare
    ids = rng.permutation(n_n)[:n_loaded]
    step = 1.5 * np.pi / n_edges
    coord = rng.uniform(-80.0, 80.0, size=(2, n_n))
    xi = np.array([float(v) for v in NODES[n_p_s]])
    edges = np.zeros((n_p_s, n_edges), dtype=np.int64)
    inner = [a for a in np.argsort(xi) if a > 1]                            # interior local nodes from B towards A
    for e in range(n_edges):
        base = e * (n_p_s - 1)
        edges[0, e], edges[1, e] = ids[base], ids[base + n_p_s - 1]
        for k, a in enumerate(inner):
            edges[a, e] = ids[base + 1 + k]
        th = 0.3 + step * (e + (xi + 1) / 2)
        coord[0, edges[:, e]] = CENTRE[0] + RADIUS * np.cos(th)
        coord[1, edges[:, e]] = CENTRE[1] + RADIUS * np.sin(th)
    return edges, coord


def _wall(fep, level, t):
    g = load_golden('tsx')
    H = fep.tsx_tunnel.TSX_HOLE
    c, e = fep.refine_uniform(g['coord'], g['elem'], levels=level, curves=[H])
    h = fep.create_midpoints(t, c, e, curves=[H])
    return h['surf'][:, h['surf_curve'] == 0].astype(np.int64), h['coord_ext']


def _ring_outer(fep, name, t):
    coord, elem, curves = curved_cases.cases(fep)[name][:3]
    c, e = fep.refine_uniform(coord, elem, levels=1, curves=curves)
    h = fep.create_midpoints(t, c, e, curves=curves)
    return h['surf'][:, h['surf_curve'] == 1].astype(np.int64), h['coord_ext']


@functools.lru_cache(maxsize=None)
def _traction_cases(fep):
    rng = np.random.default_rng(20260317)
    out = []
    for n in (254, 255, 256, 512):                                          # 255 / 256 / 257 / 513 loaded nodes
        ed, co = _arc(n, 2, rng)
        for n_q in (1, 8):
            out.append(_with_load(f'arc of {n} two-node edges', ed, co, n_q, rng, 'random'))
    ed, co = _arc(64, 5, rng)                                               # 257 loaded nodes
    out.append(_with_load('arc of 64 five-node edges', ed, co, 8, rng, 'random'))
    out.append(_with_load('arc of 64 five-node edges', ed, co, 8, rng, 'pressure'))
    ed, co = _arc(86, 4, rng)                                               # 259 loaded nodes
    out.append(_with_load('arc of 86 four-node edges', ed, co, 5, rng, 'random'))
    walls = {}
    for level in (0, 2):
        for t in ('P2', 'P4'):
            ed, co = walls[level, t] = _wall(fep, level, t)
            for n_q in (2, 5, 8):
                for kind in ('random', 'pressure'):
                    out.append(_with_load(f'tunnel wall level {level} {t}', ed, co, n_q, rng, kind, closed=True, shuffle=True))
    for name in ('ring between two ellipses', 'ring with one sector missing'):
        for t in ('P2', 'P4'):
            ed, co = _ring_outer(fep, name, t)
            for kind in ('random', 'pressure'):
                out.append(_with_load(f'outer boundary of the {name} {t}', ed, co, 5, rng, kind,
                                      closed=name == 'ring between two ellipses', shuffle=True))
    # a hub of 40 edges at node 0 and a star of 7 at node n_n - 1 in a large array; the hub is local node 0 or 1 in turn
    n_n = 100_000
    co = rng.uniform(-50.0, 50.0, size=(2, n_n))
    k = np.arange(1, 41)
    hub = np.where(k % 2 == 0, np.stack([0 * k, k]), np.stack([k, 0 * k]))
    k = np.arange(1, 8)
    star = np.where(k % 2 == 0, np.stack([0 * k + n_n - 1, n_n - 1 - k]), np.stack([n_n - 1 - k, 0 * k + n_n - 1]))
    ed = np.concatenate([hub, star], axis=1)[:, rng.permutation(47)]
    for n_q in (1, 8):
        out.append(_with_load('hub of 40 and star of 7 in 100 000 nodes', ed, co, n_q, rng, 'random'))
    # the level-2 P2 wall with every edge listed twice (each listing with its own traction), and with half of the edges
    # reversed: rows 0 and 1 swapped, which with the symmetric node order (-1, 1, 0) is the same table at xi -> -xi
    ed, co = walls[2, 'P2']
    twice = np.concatenate([ed, ed[:, rng.permutation(ed.shape[1])]], axis=1)
    out.append(_with_load('level-2 P2 wall, every edge twice', twice, co, 2, rng, 'random'))
    rev = ed.copy()
    flip = rng.random(ed.shape[1]) < 0.5
    rev[0, flip], rev[1, flip] = ed[1, flip], ed[0, flip]
    out.append(_with_load('level-2 P2 wall, half of the edges reversed', rev, co, 5, rng, 'random'))
    # nothing to do
    out.append(Case('no edges, 1000 nodes', np.zeros((2, 0)), rng.uniform(-1, 1, size=(2, 1000)), np.zeros((2, 0)), 2))
    out.append(Case('no edges, no nodes', np.zeros((3, 0)), np.zeros((2, 0)), np.zeros((2, 0)), 2))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def traction_cases(fep):
    return _traction_cases(fep)


def _names():
    """The names of _traction_cases, for parametrize: known without building a mesh (traction_case checks them)."""
    out = [f'arc of {n} two-node edges, {q}-point, random' for n in (254, 255, 256, 512) for q in (1, 8)]
    out += ['arc of 64 five-node edges, 8-point, random', 'arc of 64 five-node edges, 8-point, pressure',
            'arc of 86 four-node edges, 5-point, random']
    out += [f'tunnel wall level {lv} {t}, {q}-point, {kind}, shuffled' for lv in (0, 2) for t in ('P2', 'P4') for q in (2, 5, 8)
            for kind in ('random', 'pressure')]
    out += [f'outer boundary of the {n} {t}, 5-point, {kind}, shuffled' for n in ('ring between two ellipses', 'ring with one sector missing')
            for t in ('P2', 'P4') for kind in ('random', 'pressure')]
    out += [f'hub of 40 and star of 7 in 100 000 nodes, {q}-point, random' for q in (1, 8)]
    out += ['level-2 P2 wall, every edge twice, 2-point, random', 'level-2 P2 wall, half of the edges reversed, 5-point, random',
            'no edges, 1000 nodes', 'no edges, no nodes']
    return tuple(out)


TRACTION_NAMES = _names()


def traction_case(fep, name):
    cases = traction_cases(fep)
    assert tuple(c.name for c in cases) == TRACTION_NAMES
    return cases[TRACTION_NAMES.index(name)]


_EXACT = {}


def exact(case):
    """(traction_exact, lim, m) of a case, computed once per process and returned read-only."""
    if case.name not in _EXACT:
        f = lx.traction_exact(*case.args())
        lim, m = lx.traction_bound(*case.args())
        for a in (f, lim, m):
            a.setflags(write=False)
        _EXACT[case.name] = (f, lim, m)
    return _EXACT[case.name]


def within(name, got, ref, lim):
    """Every entry of got within lim of ref; prints and returns the worst ratio (an entry with lim = 0 must be equal)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape == lim.shape, (name, got.shape, ref.shape, lim.shape)
    d = np.abs(got - ref)
    worst = float((d / np.where(lim > 0, lim, 1.0)).max(initial=0.0))
    print(f'{name}: worst |delta| / bound = {worst:.3f} over {d.size} entries')
    assert not np.isnan(got).any(), name
    assert np.all(d <= lim), (name, worst, np.argwhere(d > lim)[:5])
    return worst


def pressure_total_bound(case, f):
    """Bound on |sum_n f[c, n]| (2,) of a uniform pressure p on closed loops, f the vector under test (2, n_n).

    With H_q = sum_a hatp_s[a, q] the exact sum over n of the exact vector is  sum_{e, q} H_q wf_q J t_c(e, q).  The test set
    t_0 = p j2 / J, t_1 = -p j1 / J from its own float64 j^ and J^, so J t_0 = p j2 + d with
        |d| <= |p| [ |j2^ - j2| + |j2^| |J / J^ - 1| + 2 u |j2| ] <= |p| [ 4 u J + 2 n_p_s u (A_1 + A_2) ]
    (|j_c^ - j_c| <= n_p_s u A_c, |J^ - J| <= 2 u J + n_p_s u (A_1 + A_2), |j2| <= J, one rounding each for the product and the
    quotient; loads_exact's docstring has the parts), and  sum_{e, q} wf_q p j2(e, q) = p sum_e sum_a y_a (I_a + E_a) with
    I_a = L_a(1) - L_a(-1): dL_a has degree n_p_s - 2 <= 2 n_q_s - 1, so the Gauss rule integrates it exactly but for the
    rounding of its points, weights and of the table, E_a, which loads_exact.gauss_defect evaluates exactly from the tables.
    sum_e sum_a y_a I_a = sum_e (y_A - y_B) = 0 on closed loops: every end node is A of one edge and B of another.  Adding up:
      * the per-entry bounds of f against the exact vector                                sum_n lim[c, n]
      * this function's caller sums n_b entries in float64                                n_b u sum |f[c]|
      * H_q = 1 up to the rounding of n_p_s table entries, |H_q - 1| <= u sum_a |h_a| <= (n_p_s + 2) u (the Lebesgue
        function of at most 5 equispaced nodes is below 2.3):                             (n_p_s + 3) u sum_{e, q} |wf J t_c|
      * the roundings of t_int (one more u on each constant for the second order)         |p| u sum_{e, q} wf [5 J + (2 n_p_s + 1) (A_1 + A_2)]
      * the Gauss defect                                                                   |p| sum_e sum_a |x_{c', a}| E_a
    """
    assert case.pressure is not None and case.closed and case.n_p_s - 2 <= 2 * case.n_q_s - 1
    _, lim, m = exact(case)
    p = abs(case.pressure)
    J, A = lx.jacobian_sizes(case.edges, case.coord, case.dh, case.wf)
    E = lx.gauss_defect(case.nodes_xi, case.dh, case.wf)
    t = case.t_int.reshape(2, case.n_e_s, case.n_q_s)
    n_b = int((m > 0).sum())
    out = np.zeros(2)
    for c in range(2):
        other = case.coord[1 - c][case.edges]                               # (n_p_s, n_e_s)
        out[c] = (lim[c].sum() + n_b * U * np.abs(f[c]).sum()
                  + (case.n_p_s + 3) * U * np.abs(case.wf[None, :] * J * t[c]).sum()
                  + p * U * (case.wf[None, :] * (5 * J + (2 * case.n_p_s + 1) * A)).sum()
                  + p * (np.abs(other) * E[:, None]).sum())
    return out


# ---- volume ----------------------------------------------------------------------------------------------------------------
VOLUME_NAMES = ('fan 255 P1', 'fan 85 P2', 'delaunay 40 P1 renumbered', 'curved tunnel refine 1 P2', 'curved tunnel refine 1 P4')
UNIFORM = (0.37, -9.81)


@functools.lru_cache(maxsize=None)
def volume_mesh(fep, name):
    """(element type, elements (n_p, n_e) int64, coordinates (2, n_n), random field (2, n_int))"""
    import meshes
    rng = np.random.default_rng(VOLUME_NAMES.index(name) + 77)
    if name.startswith('fan'):
        t = name.split()[2]
        elem, coord = fan_mesh.fan_mesh(int(name.split()[1]), t)
    elif name.startswith('delaunay'):
        t = 'P1'
        elem, coord = meshes.renumber(*meshes.delaunay('P1', 40, rng), rng)
    else:
        t = name.split()[-1]
        g = load_golden('tsx')
        coord, elem = fep.prepare_tsx_mesh(g['coord'], g['elem'], t, refine=1, curves=[fep.tsx_tunnel.TSX_HOLE])[:2]
    elem = np.ascontiguousarray(elem, dtype=np.int64)
    n_q = fep.element_tables(t)[2].size
    return t, elem, np.ascontiguousarray(coord, dtype=np.float64), rng.uniform(-2.0, 2.0, size=(2, elem.shape[1] * n_q))


def hatp(fep, t):
    h = fep.get_local_basis_volume(t, fep.get_quadrature_volume(t)[0])[0]
    n_p, n_q = fep.element_tables(t)[0].shape
    return np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), (n_p, n_q)))


def host_weight(fep, t, elem, coord):
    """|det J| wf per integration point (n_e n_q,) in NumPy: the weights of the host test, where no context exists.  (The GPU
    test takes the context's own; weights are an input of the load vector either way.)"""
    d1, d2, wf = fep.element_tables(t)
    x, y = coord[0][elem], coord[1][elem]                                   # (n_p, n_e)
    j11, j12, j21, j22 = x.T @ d1, y.T @ d1, x.T @ d2, y.T @ d2             # (n_e, n_q)
    return (np.abs(j11 * j22 - j12 * j21) * wf[None, :]).ravel()


def uniform_field(n_int):
    return np.array([[UNIFORM[0]], [UNIFORM[1]]]) * np.ones((1, n_int))


def exact_volume(elem, n_n, f, h, w):
    """(volume_exact, lim, m); not cached: the weights differ between the host and the GPU test."""
    lim, m = lx.volume_bound(elem, n_n, f, h, w)
    return lx.volume_exact(elem, n_n, f, h, w), lim, m

"""
Meshes and checks shared by test_mesh_curved_host.py and test_mesh_curved_gpu.py: the smallest meshes on which the
curved-boundary rule (include/fep.h, fep_mesh_set_curves) can go wrong, and the properties every result must have.

Everything here recomputes the rule with vectorised NumPy (np.sqrt, /: correctly rounded, like the library's operations),
independently of midpoints.py's scalar code.
"""
from fractions import Fraction

import numpy as np

import fan_mesh
from conftest import load_golden

U = 2.0 ** -53
OPS = ('refine', 'P2', 'P4')


def _ccw(coord, elem):
    x, y = coord
    d = (x[elem[1]] - x[elem[0]]) * (y[elem[2]] - y[elem[0]]) - (x[elem[2]] - x[elem[0]]) * (y[elem[1]] - y[elem[0]])
    assert (d > 0).all()
    return np.ascontiguousarray(coord, dtype=np.float64), np.ascontiguousarray(elem, dtype=np.int64)


def _ring(fep, sectors):
    cx, cy = 0.3, -0.2
    inner, outer = fep.Ellipse(cx, cy, 1.0, 0.8, 1e-9), fep.Ellipse(cx, cy, 2.5, 2.0, 1e-9)
    th = np.pi / 3 * np.arange(6)
    coord = np.concatenate([[cx + inner.a * np.cos(th), cy + inner.b * np.sin(th)],
                            [cx + outer.a * np.cos(th), cy + outer.b * np.sin(th)]], axis=1)
    el = []
    for i in sectors:
        j = (i + 1) % 6
        el += [(i, 6 + i, 6 + j), (i, 6 + j, j)]
    return _ccw(coord, np.array(el).T) + ([inner, outer],)


def cases(fep):
    """name -> (coord, elem, curves, number of boundary edges, number of curved edges)"""
    E = fep.Ellipse
    th = np.deg2rad([90.0, 210.0, 330.0])
    tri = np.array([np.cos(th), np.sin(th)])
    e1 = np.array([[0], [1], [2]])
    out = {}
    out['one triangle in the unit circle'] = _ccw(tri, e1) + ([E(0, 0, 1, 1, 1e-9)], 3, 3)
    sq = np.array([[0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0]])
    out['unit square in its circle'] = _ccw(sq, np.array([[0, 0], [1, 2], [2, 3]])) + ([E(0.5, 0.5, np.sqrt(0.5), np.sqrt(0.5), 1e-9)], 4, 4)
    out['edge through the centre'] = _ccw(np.array([[-1.0, 0.0, 1.0], [0.0, -1.0, 0.0]]), e1) + ([E(0, 0, 1, 1, 1e-9)], 3, 3)
    out['ring between two ellipses'] = _ring(fep, range(6)) + (12, 12)
    out['ring with one sector missing'] = _ring(fep, range(5)) + (12, 10)   # two radial boundary edges between the curves
    tol = 1e-3
    off = tri.copy()
    off[:, 0] *= 1 + 2 * tol                                                # g = 1 + 2 tol: not on the curve
    out['vertex at g = 1 + 2 tol'] = _ccw(off, e1) + ([E(0, 0, 1, 1, tol)], 3, 1)
    ef, cf = fan_mesh.fan_p1(200)                                           # the rim's edges are interior: never curved
    out['fan 200'] = _ccw(cf, ef) + ([E(0, 0, 1, 1, 0.05), E(0, 0, 2, 2, 0.05)], 200, 200)
    g = load_golden('tsx')
    out['tunnel'] = _ccw(g['coord'], g['elem']) + ([fep.tsx_tunnel.TSX_HOLE], 65, 25)
    return out


CASE_NAMES = ('one triangle in the unit circle', 'unit square in its circle', 'edge through the centre',
              'ring between two ellipses', 'ring with one sector missing', 'vertex at g = 1 + 2 tol', 'fan 200', 'tunnel')


def over_curved(fep):
    """A thin triangle (height 0.1) on a chord of the unit circle whose sagitta is 0.2: the projected midpoint of the chord
    passes the apex (0, 1) above (0, 0.9), so the three children that hold it, (V1, m12, m31), (m12, V2, m23) and (m12, m23, m31),
    turn over; (m31, m23, V3) does not."""
    return _ccw(np.array([[-0.6, 0.6, 0.0], [0.8, 0.8, 0.9]]), np.array([[0], [1], [2]])) + ([fep.Ellipse(0, 0, 1, 1, 1e-3)],)


def g_of(c, x, y):
    return np.sqrt(((x - c[0]) / c[2]) * ((x - c[0]) / c[2]) + ((y - c[1]) / c[3]) * ((y - c[1]) / c[3]))


def brute_surf_curve(coord, elem, surf, curves):
    """The rule by brute force for the boundary edges (B, A) = surf[:2]: how many elements hold both ends, which curves
    hold both ends."""
    x, y = coord
    out = []
    for B, A in np.asarray(surf[:2]).T.astype(np.int64):
        holders = int(((elem[:3] == A).any(axis=0) & (elem[:3] == B).any(axis=0)).sum())
        q = -1
        if holders == 1:
            for k, c in enumerate(curves):
                if abs(g_of(c, x[A], y[A]) - 1) <= c[4] and abs(g_of(c, x[B], y[B]) - 1) <= c[4]:
                    q = k
                    break
        out.append(q)
    return np.array(out, dtype=np.int64)


def run(fep, op, coord, elem, device, **kw):
    """The result of `op` as a dict of arrays ('coord_ext', 'elem_ext', ...)."""
    if op == 'refine':
        c, e = fep.refine_uniform(coord, elem, device=device, **kw)
        return {'coord_ext': c, 'elem_ext': e}
    return (fep.create_midpoints_P2 if op == 'P2' else fep.create_midpoints_P4)(coord, elem, device=device, **kw)


def same_bytes(a, b, what=''):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def curved_nodes(fep, op, coord, elem, curves):
    """(ids of the new nodes on curved edges, curve index of each), from the straight host enrichment's surf."""
    h = (fep.create_midpoints_P4 if op == 'P4' else fep.create_midpoints_P2)(coord, elem)
    q = brute_surf_curve(coord, elem, h['surf'], curves)
    rows = h['surf'][2:, q >= 0].astype(np.int64)
    return rows.ravel(), np.broadcast_to(q[q >= 0], rows.shape).ravel(), h['surf'], q


def p4_blend_weights():
    """w[n][k]: the weight of the offset of node k of a curved edge a -> b (k = 0: its midpoint, 1: the quarter point nearer
    a, 2: nearer b) in the move of the interior node n (0: nearest a, 1: nearest b, 2: nearest the third vertex):
    (l_a + l_b)^2 L(t), t = l_b / (l_a + l_b), L the quartic Lagrange basis on {0, 1/4, 1/2, 3/4, 1}, in rational
    arithmetic from the nodes' barycentric coordinates (1/2 at the nearest vertex, 1/4 at the others), rounded once."""
    tn = [Fraction(k, 4) for k in range(5)]
    w = []
    for la, lb in ((Fraction(1, 2), Fraction(1, 4)), (Fraction(1, 4), Fraction(1, 2)), (Fraction(1, 4), Fraction(1, 4))):
        s, t = la + lb, lb / (la + lb)
        row = []
        for k in (2, 1, 3):
            L = Fraction(1)
            for m in range(5):
                if m != k:
                    L *= (t - tn[m]) / (tn[k] - tn[m])
            row.append(float(s * s * L))
        w.append(row)
    assert w[2][1] == 0 and w[2][2] == 0
    return w


def p4_interior_rule(elem_ext, straight, curved):
    """The interior nodes of every P4 element by the rule of include/fep.h (fep_mesh_set_curves), from the straight
    enrichment and the edge nodes of the curved one: (2, 3, n_e), node nearest V1, V2, V3.  Vectorised over the elements;
    an edge that is not curved has the offset 0 and adds 0, so the sum runs over all three edges of every element, in the
    rule's order and with its operations."""
    w = p4_blend_weights()
    e = np.asarray(elem_ext, dtype=np.int64)
    out = straight[:, e[12:15]].copy()
    for s in range(3):
        d = [curved[:, e[r]] - straight[:, e[r]] for r in (3 + s, 6 + 2 * s, 7 + 2 * s)]
        a, b, c = s, (s + 1) % 3, (s + 2) % 3
        out[:, a] = out[:, a] + ((w[0][0] * d[0] + w[0][1] * d[1]) + w[0][2] * d[2])
        out[:, b] = out[:, b] + ((w[1][0] * d[0] + w[1][1] * d[1]) + w[1][2] * d[2])
        out[:, c] = out[:, c] + w[2][0] * d[0]
    return out


def check_curved(fep, name, coord, elem, curves, n_bnd, n_curved, device):
    """The assertions of one mesh for refine, P2 and P4 on the host (device=None) or a GPU.  Returns the curved results."""
    results = {}
    for op in OPS:
        what = (name, op)
        base = run(fep, op, coord, elem, device)
        same_bytes(run(fep, op, coord, elem, device, curves=None), base, what)
        same_bytes(run(fep, op, coord, elem, device, curves=[]), base, what)
        cur = run(fep, op, coord, elem, device, curves=curves)
        ids, q_of, surf, q = curved_nodes(fep, op, coord, elem, curves)
        assert surf.shape[1] == n_bnd and int((q >= 0).sum()) == n_curved, what
        assert ids.size == n_curved * (3 if op == 'P4' else 1)
        # tables
        assert sorted(cur) == sorted(list(base) + ([] if op == 'refine' else ['surf_curve'])), what
        for k in base:
            if k not in ('coord_ext', 'coord_mid'):
                assert cur[k].dtype == base[k].dtype and np.array_equal(cur[k], base[k]), (what, k)
        if op != 'refine':
            assert cur['surf_curve'].dtype == np.int64 and np.array_equal(cur['surf_curve'], q), what
        # coordinates: untouched away from the new nodes of curved edges ...
        cc, cb = cur['coord_ext'], base['coord_ext']
        assert cc.shape == cb.shape and cc.dtype == cb.dtype
        other = np.ones(cc.shape[1], dtype=bool)
        other[ids] = False
        if op == 'P4':                                                         # ... and of the P4 interior nodes, which follow the rule
            inner = cur['elem_ext'][12:15].astype(np.int64)
            other[inner] = False
            want = p4_interior_rule(cur['elem_ext'], cb, cc)
            assert cc[:, inner].tobytes() == want.tobytes(), (what, np.abs(cc[:, inner] - want).max())
            holds = np.isin(cur['elem_ext'][3:12], ids).any(axis=0)            # elements with a curved edge
            assert int(holds.sum()) == np.unique(surf_elements(cur['elem_ext'], surf[:, q >= 0])).size, what
            assert cc[:, inner[:, ~holds]].tobytes() == cb[:, inner[:, ~holds]].tobytes(), what
            if n_curved:
                assert (cc[:, inner[:, holds]] != cb[:, inner[:, holds]]).any(axis=(0, 1)).all(), what   # each such element: a node moved
        assert cc[:, other].tobytes() == cb[:, other].tobytes(), what
        if op != 'refine':
            n_n = coord.shape[1]
            assert cur['coord_mid'].tobytes() == cc[:, n_n:].tobytes()
        # ... and on the curve, on the ray of the straight point, at them
        for k, c in enumerate(curves):
            sel = ids[q_of == k]
            if not sel.size:
                continue
            xs, ys = cb[0, sel], cb[1, sel]
            g = g_of(c, xs, ys)
            stay = g == 0
            assert np.array_equal(cc[:, sel][:, stay], cb[:, sel][:, stay]), what
            assert np.isfinite(cc[:, sel]).all()
            mv = sel[~stay]
            gp = g_of(c, cc[0, mv], cc[1, mv])
            assert np.abs(gp - 1).max(initial=0) <= 16 * U * (1 + (abs(c[0]) + abs(c[1])) / min(c[2], c[3])), (what, np.abs(gp - 1).max())
            ex = c[0] + (xs[~stay] - c[0]) / g[~stay]
            ey = c[1] + (ys[~stay] - c[1]) / g[~stay]
            assert np.abs(cc[0, mv] - ex).max(initial=0) <= 4 * U * (abs(c[0]) + max(c[2], c[3])), what
            assert np.abs(cc[1, mv] - ey).max(initial=0) <= 4 * U * (abs(c[1]) + max(c[2], c[3])), what
            if n_curved:
                assert (cc[:, mv] != cb[:, mv]).any(), what                # the projection did something
        results[op] = cur
    return results


def surf_elements(elem_ext, surf):
    """The element that holds the midpoint (row 2) of each P4 surf column."""
    mids = np.asarray(elem_ext)[3:6]
    return np.array([int(np.flatnonzero((mids == m).any(axis=0))[0]) for m in surf[2].astype(np.int64)], dtype=np.int64)


def compare_device_host(name, dev, host):
    """Device results against host results: every array equal.  (One differing rounding in the square root or a division
    would show as 4 u (|c| + max(a, b)) per component at the new nodes of curved edges; on the MI355X there is none.)"""
    for op in OPS:
        d, h = dev[op], host[op]
        assert sorted(d) == sorted(h)
        for k in h:
            if k not in ('coord_ext', 'coord_mid'):
                assert d[k].dtype == h[k].dtype and np.array_equal(d[k], h[k]), (name, op, k)
        dc, hc = d['coord_ext'], h['coord_ext']
        assert dc.shape == hc.shape and dc.dtype == hc.dtype
        assert np.array_equal(dc, hc), (name, op)


# ---- the tunnel wall -------------------------------------------------------------------------------------------------------
def boundary_edges(elem):
    """Directed boundary edges (A, B) of a consistently oriented triangle mesh: walked by one element, never backwards."""
    a = np.concatenate([elem[0], elem[1], elem[2]]).astype(np.int64)
    b = np.concatenate([elem[1], elem[2], elem[0]]).astype(np.int64)
    n = int(max(a.max(), b.max())) + 1
    keep = ~np.isin(a * n + b, b * n + a)
    return a[keep], b[keep]


def wall_edges(coord, elem, curve):
    a, b = boundary_edges(elem)
    x, y = coord
    on = (np.abs(g_of(curve, x[a], y[a]) - 1) <= curve[4]) & (np.abs(g_of(curve, x[b], y[b]) - 1) <= curve[4])
    return a[on], b[on]


def polygon_area(coord, a, b):
    """Area enclosed by the closed loop of directed edges a -> b (shoelace)."""
    x, y = coord
    return abs(0.5 * np.sum(x[a] * y[b] - x[b] * y[a]))


def triangle_area(coord, elem):
    x, y = coord
    d = (x[elem[1]] - x[elem[0]]) * (y[elem[2]] - y[elem[0]]) - (x[elem[2]] - x[elem[0]]) * (y[elem[1]] - y[elem[0]])
    return d


def curved_loop_area(coord, node_rows, n_gauss):
    """Area enclosed by a closed loop of polynomial edges, 1/2 |sum of int (x y' - y x') dt|, by `n_gauss`-point Gauss per
    edge.  node_rows (n_nodes_per_edge, n_edges): the nodes of each edge at equally spaced parameters, start to end."""
    k = node_rows.shape[0]
    tn = np.linspace(0, 1, k)
    gx, gw = np.polynomial.legendre.leggauss(n_gauss)
    t, w = (gx + 1) / 2, gw / 2
    L = np.ones((k, t.size))
    dL = np.zeros((k, t.size))
    for i in range(k):
        for j in range(k):
            if j != i:
                L[i] *= (t - tn[j]) / (tn[i] - tn[j])
                term = np.full(t.size, 1 / (tn[i] - tn[j]))
                for m in range(k):
                    if m != i and m != j:
                        term *= (t - tn[m]) / (tn[i] - tn[m])
                dL[i] += term
    X, Y = coord[0][node_rows], coord[1][node_rows]                         # (k, n_edges)
    x, y, dx, dy = L.T @ X, L.T @ Y, dL.T @ X, dL.T @ Y                      # (n_gauss, n_edges)
    return abs(0.5 * np.sum(w[:, None] * (x * dy - y * dx)))

"""
Meshes and checkers for the mesh kernels at the sizes where their prefix sums change shape (test_scale_cases_host.py,
test_mesh_scale_gpu.py).  Every list the mesh kernels build (node -> element lists, the edge numbering, the marked-edge ranks,
the first-child offsets) comes from one recursive int32 prefix sum over tiles of kScanTile = 1024 entries
(csrc/fep_mesh.hip, scan_exclusive): one tile up to 1024 entries, two levels up to 1024^2, a third level above.  The meshes
here put each scanned length at those edges; the checkers are plain vectorised NumPy (np.unique, sorting, bincount) that
shares no code with the kernels or with their NumPy twin (midpoints.py, transfer.py), so they stay a reference at a million
elements, where the twin's dictionary walk takes minutes.  On integer coordinates every check is an exact equality.
"""
from collections import namedtuple
from importlib import import_module

import numpy as np

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

SCAN_TILE = 1024                                   # kScanTile of csrc/fep_mesh.hip (kBlock 256 x kScanItems 4)
SWEEPS_PER_READ = 4                                # kSweepsPerRead of csrc/fep_mesh.hip
EPS = np.finfo(np.float64).eps


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def strip(n):
    """(coord (2, n + 2), elem (3, n)): exactly n triangles on integer coordinates.  Cells [c, c + 1] x [0, 1] split as
    (b0, b1, t0), (b1, t1, t0), cut to n columns, unused nodes dropped and the ids compacted.  Both triangles are
    counter-clockwise; each one's strictly longest edge (squared length 2 against 1) is the diagonal it shares with its cell
    partner, so the closure of any marking ends after two propagation steps.  n_n = n + 2, n_edges = 2 n + 1, n_boundary =
    n + 2; midpoints, quarter points and doubled areas are exact doubles."""
    nc = n // 2 + 1
    x = np.concatenate([np.arange(nc + 1), np.arange(nc + 1)]).astype(np.float64)
    y = np.concatenate([np.zeros(nc + 1), np.ones(nc + 1)])
    c = np.arange(nc, dtype=np.int64)
    b0, b1, t0, t1 = c, c + 1, nc + 1 + c, nc + 2 + c
    elem = np.stack([np.stack([b0, b1, t0]), np.stack([b1, t1, t0])], axis=2).reshape(3, -1)[:, :n]
    used = np.unique(elem)
    new = np.full(2 * nc + 2, -1, dtype=np.int64)
    new[used] = np.arange(used.size)
    return np.ascontiguousarray(np.stack([x, y])[:, used]), np.ascontiguousarray(new[elem])


def strip_counts(n):
    """The closed forms of strip(n): (n_n, n_e, n_edges, n_boundary)."""
    return n + 2, n, 2 * n + 1, n + 2


def scanned_lengths(n):
    """The lengths scan_exclusive sees on strip(n): n_n + 1 (node -> element lists), n_e + 1 (base, bbase, m_cbase) and
    n_edges + 1 (m_erank)."""
    n_n, n_e, n_edges, _ = strip_counts(n)
    return {'n_n + 1': n_n + 1, 'n_e + 1': n_e + 1, 'n_edges + 1': n_edges + 1}


def scan_levels(length):
    """Levels of the recursion for `length` entries: 1 up to kScanTile, 2 up to kScanTile^2, 3 above (up to kScanTile^3)."""
    levels, tiles = 1, -(-length // SCAN_TILE)
    while tiles > 1:
        levels, tiles = levels + 1, -(-tiles // SCAN_TILE)
    return levels


def edge_sizes(limit):
    """The strips that put each scanned length at `limit` entries (or, where parity forbids that, at the largest length not
    above it) and at the first length past it, and n_e itself one past `limit`."""
    out = {limit + 1}
    for name in ('n_n + 1', 'n_e + 1', 'n_edges + 1'):
        n = 1
        while scanned_lengths(2 * n)[name] <= limit:                                # bracket, then bisect: largest n with length <= limit
            n *= 2
        lo, hi = n, 2 * n
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if scanned_lengths(mid)[name] <= limit else (lo, mid)
        out |= {lo, lo + 1}
    return sorted(out)


SMALL_SIZES = edge_sizes(SCAN_TILE)                # 511, 512, 1021 .. 1025: one tile | two
LARGE_SIZES = edge_sizes(SCAN_TILE ** 2)           # 524 287, 524 288, 1 048 573 .. 1 048 577: two levels | three
JITTER_N = 725                                     # 1 051 250 triangles, about 1.58 M edges


def jittered_square(N=JITTER_N, seed=7):
    """fep.square_mesh(N, 'P1', N) with the interior nodes moved by a seeded uniform +-0.2: unit cells, interior nodes of
    degree 6, no two edges of a triangle equally long."""
    m = import_module('fem-elastoplasticity_amd').square_mesh(N, 'P1', N)
    coord, elem = np.array(m['coordinates'], dtype=np.float64), np.ascontiguousarray(m['elements'], dtype=np.int64)
    x, y = coord
    inner = (x > 0) & (x < N) & (y > 0) & (y < N)
    coord[:, inner] += np.random.default_rng(seed).uniform(-0.2, 0.2, size=(2, int(inner.sum())))
    return coord, elem


def marking(kind, n_e, seed=5, coord=None, elem=None):
    """Marks (n_e) bool: 'none', 'all', 'random' (a seeded 30 %), 'first', 'last' (one element), 'disc' (centroid within a
    quarter of the mesh's width of its centre)."""
    m = np.zeros(n_e, dtype=bool)
    if kind == 'all':
        m[:] = True
    elif kind == 'random':
        m = np.random.default_rng(seed + n_e).random(n_e) < 0.3
    elif kind == 'first':
        m[0] = True
    elif kind == 'last':
        m[-1] = True
    elif kind == 'disc':
        c = coord[:, elem[:3]].mean(axis=1)
        mid, r = (coord.max(axis=1) + coord.min(axis=1)) / 2, (coord[0].max() - coord[0].min()) / 4
        m = (c[0] - mid[0]) ** 2 + (c[1] - mid[1]) ** 2 < r * r
    elif kind != 'none':
        raise ValueError(kind)
    return m


def max_sweeps(steps=2):
    """Limit of fep_mesh_mark's n_sweeps when the closure ends after `steps` propagation steps: every sweep carries the marks
    at least one step further, so the last change falls into the read that holds sweep `steps`, and one more read of
    kSweepsPerRead sweeps sees no change and ends the loop."""
    return (-(-steps // SWEEPS_PER_READ) + 1) * SWEEPS_PER_READ


# ---- the edge table -----------------------------------------------------------------------------------------------------------
EdgeTable = namedtuple('EdgeTable', 'edges he mult opposite key n')


def _vertices(elem):
    return np.ascontiguousarray(np.asarray(elem)[:3], dtype=np.int64)


def _key(a, b, n):
    return np.minimum(a, b) * n + np.maximum(a, b)


def edge_table(elem):
    """Edge k of a triangle runs from vertex k to vertex (k + 1) % 3.  Returns the unique undirected edges (2, n_edges) (lower
    id first, sorted), per half-edge its edge index `he` (3, n_e), per edge its multiplicity and whether it has exactly two
    half-edges that run opposite ways; `key`, `n`: the sorted keys lower * n + higher behind them."""
    elem = _vertices(elem)
    a, b = elem, elem[[1, 2, 0]]
    n = int(elem.max()) + 1
    key, inv, mult = np.unique(_key(a, b, n).ravel(), return_inverse=True, return_counts=True)
    inv = inv.ravel()
    forward = np.bincount(inv[(a < b).ravel()], minlength=key.size)
    return EdgeTable(np.stack([key // n, key % n]), inv.reshape(3, -1), mult, (mult == 2) & (forward == 1), key, n)


def _by_edge(t, values, what):
    """values (3, n_e), one per half-edge -> (n_edges): the value of each edge; fails unless all half-edges of an edge agree."""
    out = np.empty(t.mult.size, dtype=values.dtype)
    out[t.he] = values
    assert np.array_equal(out[t.he], values), f'{what}: not a function of the undirected edge'
    return out


def doubled_areas(coord, elem):
    x, y = coord
    a, b, c = _vertices(elem)
    return (x[b] - x[a]) * (y[c] - y[a]) - (x[c] - x[a]) * (y[b] - y[a])


def check_info(info, elem):
    """fep_mesh_info against the table.  Triangles that name a vertex twice are counted and take no further part; an edge of
    more than two elements is counted once and the header does not say how such a mesh is numbered, so n_edges is held to
    the table only on a mesh without one."""
    elem = _vertices(elem)
    degenerate = (elem[0] == elem[1]) | (elem[1] == elem[2]) | (elem[2] == elem[0])
    t = edge_table(elem[:, ~degenerate])
    assert info['n_e'] == elem.shape[1]
    assert info['n_degenerate'] == int(degenerate.sum()), (info, int(degenerate.sum()))
    assert info['n_nonmanifold'] == int((t.mult > 2).sum()), (info, int((t.mult > 2).sum()))
    assert info['n_inconsistent'] == int(((t.mult == 2) & ~t.opposite).sum()), (info, int(((t.mult == 2) & ~t.opposite).sum()))
    assert info['n_boundary_edges'] == int((t.mult == 1).sum()), (info, int((t.mult == 1).sum()))
    if info['n_nonmanifold'] == 0:
        assert info['n_edges'] == t.mult.size, (info, t.mult.size)
    return t


# ---- enrichment ---------------------------------------------------------------------------------------------------------------
def _same_coordinates(got, expr, parts, ulps, what):
    """got == expr(*parts) bit for bit (ulps = 0), or within `ulps` units in the last place of the largest coordinate of an
    extended-precision evaluation of expr."""
    if ulps == 0:
        assert np.array_equal(got, expr(*parts)), what
        return
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, 'the ulp bound needs an extended-precision reference'
    x = max(float(np.abs(p).max()) for p in parts)
    err = np.abs(got.astype(np.longdouble) - expr(*(p.astype(np.longdouble) for p in parts))).max()
    assert err <= ulps * np.spacing(x), (what, float(err), np.spacing(x))


def _check_surf(t, surf, elem, n_n, n_rows):
    """`surf` (n_rows, n_boundary), columns (B, A, nodes ...): exactly the boundary edges, each once, A -> B the walking
    direction of the one element that holds the edge.  Returns (surf as integers, the edge index of every column)."""
    s = np.asarray(surf)
    boundary = np.flatnonzero(t.mult == 1)
    assert s.shape == (n_rows, boundary.size), (s.shape, boundary.size)
    ids = s.astype(np.int64)
    assert np.array_equal(ids, s)
    B, A = ids[0], ids[1]
    assert ((A >= 0) & (A < n_n) & (B >= 0) & (B < n_n)).all()
    at = np.searchsorted(t.key, _key(A, B, t.n))
    assert (at < t.key.size).all() and np.array_equal(t.key[np.minimum(at, t.key.size - 1)], _key(A, B, t.n)), 'surf: not an edge'
    assert np.array_equal(np.sort(at), boundary), 'surf: not exactly the boundary edges, each once'
    start, end = _half_edge_value(t, elem)[at], _half_edge_value(t, elem[[1, 2, 0]])[at]
    assert np.array_equal(A, start) and np.array_equal(B, end), 'surf: walked backwards'
    return ids, at


def _half_edge_value(t, values):
    """(n_edges): the value of the last half-edge of each edge — THE half-edge of a boundary edge."""
    out = np.empty(t.mult.size, dtype=values.dtype)
    out[t.he] = values
    return out


def check_p2(h, coord, elem, t=None):
    """The dict of DeviceMesh.enrich('P2') / create_midpoints_P2 on an edge-manifold, consistently oriented mesh."""
    coord, elem = np.asarray(coord, dtype=np.float64), _vertices(elem)
    t = edge_table(elem) if t is None else t
    assert t.mult.max() <= 2 and t.opposite[t.mult == 2].all()
    n_n, n_e, n_edges = coord.shape[1], elem.shape[1], t.mult.size
    ext = np.asarray(h['elem_ext'])
    assert ext.shape == (6, n_e) and np.array_equal(ext[:3], elem)
    # include/fep.h: rows (V1, V2, V3, m23, m31, m12), so the node of edge k (vertex k -> k + 1) sits in row 3 + (k + 2) % 3
    ids = ext[[5, 3, 4]]
    by_edge = _by_edge(t, ids, 'P2 node ids')
    assert np.array_equal(np.sort(by_edge), np.arange(n_n, n_n + n_edges)), 'P2 node ids: not a bijection onto [n_n, n_n + n_edges)'
    cx = np.asarray(h['coord_ext'])
    assert cx.shape == (2, n_n + n_edges) and cx.dtype == np.float64
    assert np.array_equal(cx[:, :n_n], coord), 'old nodes moved'
    a, b = t.edges
    assert np.array_equal(cx[:, by_edge], (coord[:, a] + coord[:, b]) / 2), 'P2 midpoints'
    if 'coord_mid' in h:
        assert np.array_equal(h['coord_mid'], cx[:, n_n:])
    s, at = _check_surf(t, h['surf'], elem, n_n, 3)
    assert np.array_equal(s[2], by_edge[at]), 'surf: the node of its edge'
    ed = np.asarray(h['elem_ed'])
    assert ed.shape == (3, n_e) and np.array_equal(ed + n_n, ext[3:6]), 'elem_ed'
    el = np.asarray(h['edge_el'])
    assert el.shape == (2, n_edges) and np.array_equal(el, el.astype(np.int64)) and (el >= 0).all() and (el < n_e).all()
    el = el.astype(np.int64)[:, by_edge - n_n]                                        # in the order of the table's edges
    every = np.arange(n_edges)
    assert (t.he[:, el[0]] == every).any(axis=0).all(), 'edge_el row 0: an element that does not hold the edge'
    interior = t.mult == 2
    assert (t.he[:, el[1]] == every).any(axis=0)[interior].all() and (el[0] != el[1])[interior].all(), 'edge_el row 1'
    assert (el[1][~interior] == 0).all(), 'edge_el row 1 on the boundary'
    return t


def check_p4(h, coord, elem, ulps=0, t=None):
    """The dict of DeviceMesh.enrich('P4') / create_midpoints_P4.  ulps = 0: coordinates equal the header's expressions bit
    for bit (on coordinates where those are exact, any order of evaluation gives the same bits).  ulps = 2: within 2 ulp of
    the largest coordinate X of their exact value: each expression is a convex combination, so every term and partial sum is
    at most X in magnitude, and it takes at most three roundings (3 a, then two sums; the divisions by 2 and 4 are exact) of
    half an ulp of X each: 1.5 ulp, with the rest left to the extended-precision reference's own rounding."""
    coord, elem = np.asarray(coord, dtype=np.float64), _vertices(elem)
    t = edge_table(elem) if t is None else t
    assert t.mult.max() <= 2 and t.opposite[t.mult == 2].all()
    n_n, n_e, n_edges = coord.shape[1], elem.shape[1], t.mult.size
    n_new = 3 * n_e + 3 * n_edges
    ext = np.asarray(h['elem_ext'])
    assert ext.shape == (15, n_e) and np.array_equal(ext[:3], elem)
    # include/fep.h: rows 3..5 midpoints of edges 0, 1, 2; rows 6 + 2 k, 7 + 2 k the quarter points of edge k nearer its start
    # and nearer its end; rows 12..14 the interior nodes nearest V1, V2, V3
    mid, qa, qb, inner = ext[3:6], ext[6:12:2], ext[7:12:2], ext[12:15]
    new = ext[3:].ravel() - n_n
    assert new.min() >= 0 and new.max() < n_new
    count = np.bincount(new, minlength=n_new)
    assert (count > 0).all(), 'P4 node ids: an id of [n_n, n_n + 3 n_e + 3 n_edges) is missing'
    assert (count[inner - n_n] == 1).all(), 'P4 interior ids are shared'
    forward = elem < elem[[1, 2, 0]]
    rows = [_by_edge(t, mid, 'P4 midpoint ids'), _by_edge(t, np.where(forward, qa, qb), 'P4 quarter ids (swapped across the edge)'),
            _by_edge(t, np.where(forward, qb, qa), 'P4 quarter ids (swapped across the edge)')]
    for r in rows:                                 # with every id present this makes the 3 n_e + 3 n_edges ids distinct
        assert np.array_equal(count[r - n_n], t.mult)
    cx = np.asarray(h['coord_ext'])
    assert cx.shape == (2, n_n + n_new) and cx.dtype == np.float64
    assert np.array_equal(cx[:, :n_n], coord), 'old nodes moved'
    if 'coord_mid' in h:
        assert np.array_equal(h['coord_mid'], cx[:, n_n:])
    A, B = coord[:, elem], coord[:, elem[[1, 2, 0]]]                                  # (2, 3, n_e): start and end of edge k
    _same_coordinates(cx[:, mid], lambda a, b: (a + b) / 2, (A, B), ulps, 'P4 midpoints')
    _same_coordinates(cx[:, qa], lambda a, b: 3 * a / 4 + b / 4, (A, B), ulps, 'P4 quarter points nearer the start')
    _same_coordinates(cx[:, qb], lambda a, b: a / 4 + 3 * b / 4, (A, B), ulps, 'P4 quarter points nearer the end')
    for k in range(3):                             # nearest vertex k: V_k / 2 + the other two / 4, in the order V1, V2, V3
        w = [2 if j == k else 4 for j in range(3)]
        _same_coordinates(cx[:, inner[k]], lambda v1, v2, v3: v1 / w[0] + v2 / w[1] + v3 / w[2], tuple(A[:, j] for j in range(3)),
                          ulps, f'P4 interior node nearest vertex {k}')
    s, at = _check_surf(t, h['surf'], elem, n_n, 5)
    for r, values in enumerate((mid, qa, qb)):
        assert np.array_equal(s[2 + r], _half_edge_value(t, values)[at]), f'surf row {2 + r}'
    return t


# ---- refinement -------------------------------------------------------------------------------------------------------------
def uniform_codes(n_e):
    """Parents and corner codes of fep_mesh_refine_*'s children (include/fep.h): 4 i .. 4 i + 3 = (0, 3, 5), (3, 1, 4),
    (5, 4, 2), (3, 4, 5)."""
    return np.arange(4 * n_e) // 4, np.tile(np.array([[0, 3, 5], [3, 1, 4], [5, 4, 2], [3, 4, 5]], dtype=np.uint8).T, (1, n_e))


def check_children(coord, elem, coord_c, elem_c, parent, corners=None, exact=False, t=None):
    """A refinement (coord_c, elem_c, parent[, corners]) of the mesh (coord, elem): conforming, positively oriented, area
    preserving per parent (`exact`: to the bit), old nodes untouched; with corner codes also WHICH nodes the children hold.
    Returns the split edges (3, n_e) bool the codes imply (None without codes)."""
    coord, elem = np.asarray(coord, dtype=np.float64), _vertices(elem)
    coord_c, elem_c, parent = np.asarray(coord_c), np.asarray(elem_c), np.asarray(parent)
    n_n, n_e, n_child = coord.shape[1], elem.shape[1], elem_c.shape[1]
    assert elem_c.shape == (3, n_child) and parent.shape == (n_child,) and coord_c.dtype == np.float64
    assert elem_c.min() >= 0 and elem_c.max() < coord_c.shape[1]
    tc = edge_table(elem_c)
    # no hanging node: no edge of more than two children, and the two of an interior edge walk it opposite ways
    assert tc.mult.max() <= 2, 'an edge of more than two children'
    assert tc.opposite[tc.mult == 2].all(), 'two children walk an edge the same way'
    d = doubled_areas(coord_c, elem_c)
    assert (d > 0).all(), 'a child of non-positive area'
    step = np.diff(parent)
    assert parent[0] == 0 and parent[-1] == n_e - 1 and ((step == 0) | (step == 1)).all(), 'parent: not 0 .. n_e - 1 in order'
    sums, d0 = np.bincount(parent, weights=d, minlength=n_e), doubled_areas(coord, elem)
    if exact:
        assert np.array_equal(sums, d0), 'areas of the children of a parent'
    else:                                          # the bound marked_cases.check_conforming derives: 172 u X^2 = 86 eps X^2
        assert np.abs(sums - d0).max() <= 86 * EPS * max(float(np.abs(coord).max()), 1.0) ** 2
    assert np.array_equal(coord_c[:, :n_n], coord), 'old nodes moved'
    if corners is None:
        return None
    corners = np.asarray(corners)
    assert corners.shape == (3, n_child) and corners.max() <= 5
    t = edge_table(elem) if t is None else t
    code = corners.astype(np.int64)
    old = code < 3
    vertex_of_parent = elem[np.minimum(code, 2), parent[None, :]]
    assert np.array_equal(elem_c[old], vertex_of_parent[old]), 'code k < 3: not the parent\'s vertex k'
    k = np.where(old, 0, code - 3)
    a, b = elem[k, parent[None, :]], elem[(k + 1) % 3, parent[None, :]]
    new = ~old
    assert (elem_c[new] >= n_n).all(), 'code 3 + k on an old node'
    assert np.array_equal(coord_c[:, elem_c[new]], (coord[:, a[new]] + coord[:, b[new]]) / 2), 'code 3 + k: not the midpoint of edge k'
    at = (k[new], np.broadcast_to(parent, code.shape)[new])                           # (edge, parent) of every new child vertex
    split = np.zeros((3, n_e), dtype=bool)
    split[at] = True
    node = np.full((3, n_e), -1, dtype=np.int64)
    node[at] = elem_c[new]
    assert np.array_equal(node[at], elem_c[new]), 'two nodes on one edge of a parent'
    node_of_edge = _by_edge(t, node, 'split edges / their nodes (the two parents of an edge disagree)')
    assert np.array_equal(np.bincount(parent, minlength=n_e), 1 + split.sum(axis=0)), 'children per parent'
    assert n_child == n_e + int(split.sum())
    n_new = coord_c.shape[1] - n_n
    assert n_new == int((node_of_edge >= 0).sum()), 'new nodes != split undirected edges'
    assert np.array_equal(np.sort(node_of_edge[node_of_edge >= 0]), np.arange(n_n, n_n + n_new)), 'new node ids'
    return split


def reference_edge(coord, elem):
    """The slot of the longest edge: squared chord in walking order, slots compared 0, 1, 2 with a strict >."""
    x, y = np.asarray(coord, dtype=np.float64)
    elem = _vertices(elem)
    nxt = elem[[1, 2, 0]]
    dx, dy = x[nxt] - x[elem], y[nxt] - y[elem]
    length = dx * dx + dy * dy
    r = np.zeros(elem.shape[1], dtype=np.int64)
    best = length[0].copy()
    for k in (1, 2):
        longer = length[k] > best
        r[longer], best[longer] = k, length[k][longer]
    return r


def closure(coord, elem, marked, t=None):
    """The least fixpoint of include/fep.h's rule as split edges (3, n_e) bool: a marked element marks its three edges; an
    element with any marked edge marks its longest edge.  Elements meet through the table's edge indices (`he`: the
    neighbour table), one flag per undirected edge, all elements at once until nothing changes."""
    elem = _vertices(elem)
    t = edge_table(elem) if t is None else t
    marked = np.asarray(marked) != 0
    ref_edge = t.he[reference_edge(coord, elem), np.arange(elem.shape[1])]
    flag = np.zeros(t.mult.size, dtype=bool)
    flag[t.he[:, marked]] = True
    while True:
        touched = flag[t.he].any(axis=0)
        if flag[ref_edge[touched]].all():
            return flag[t.he]
        flag[ref_edge[touched]] = True


def closure_counts(state, t):
    """(n_child, n_new_nodes) of the split edges `state` (3, n_e): 1 + (split edges) children per element, one node per
    split undirected edge."""
    return state.shape[1] + int(state.sum()), int(_by_edge(t, state, 'closure').sum())


def check_marks(coord, elem, marked, split, parent, corners, t=None):
    """What the children of check_children must be for the marks `marked`: split exactly along the closure, four children of
    every marked element, an element without a split edge passed on as one child with codes (0, 1, 2)."""
    state = closure(coord, elem, marked, t)
    assert np.array_equal(split, state), 'split edges != closure of the marks'
    marked = np.asarray(marked) != 0
    per_parent = np.bincount(parent, minlength=marked.size)
    assert (per_parent[marked] == 4).all()
    whole = np.flatnonzero(~split.any(axis=0))
    first = np.searchsorted(parent, whole)
    assert (per_parent[whole] == 1).all() and np.array_equal(np.asarray(corners)[:, first], np.tile([[0], [1], [2]], (1, whole.size)))
    return state

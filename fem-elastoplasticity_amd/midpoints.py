"""
P1 -> P2 / P4 mesh enrichment with the reference's node numbering.

Mirrors `create_midpoints_P2` (tsx-tunnel/pythonFEM.py:1508-1626), `create_midpoints_P4` (TSX:1354-1505)
and the dispatcher `create_midpoints` (TSX:1629-1633): same names, same returned keys, same ids for the new
nodes (allocated in element-visit order, first element to see an edge creates its nodes), same local node
order — but the neighbour across an edge comes from an edge -> elements map built once (O(n_e)) instead
of two `np.where` scans of the whole element table per edge (O(n_e^2)).

Local orders: P2 rows 3..5 = midpoints of (V2V3, V3V1, V1V2); P4 rows 3..5 = midpoints of
(V1V2, V2V3, V3V1), rows 6..11 = quarter points (two per edge, nearer the edge's first vertex first),
rows 12..14 = interior nodes nearest V1, V2, V3.
"""
import collections
import ctypes as C
import math

import numpy as np

from .tables import LagrangeElementType, _coerce


class Ellipse(collections.namedtuple('Ellipse', 'cx cy a b tol', defaults=(1e-3,))):
    """An axis-aligned ellipse a mesh boundary follows: centre (cx, cy), semi-axes a (along x) and b (along y); a circle
    has a == b.  A vertex p is ON it iff |g(p) - 1| <= tol, g = sqrt(((x - cx) / a)**2 + ((y - cy) / b)**2).  Passed as
    `curves=[...]` (at most 4) to the enrichment and refinement functions: every node they create on a boundary edge with
    both ends on the same curve (the lowest index wins) is moved from its straight position along its ray from the centre
    onto the curve; interior edges and existing vertices are never moved, and the three interior nodes of a P4 element
    follow its curved edges by the blending rule of create_midpoints_P4 (include/fep.h, fep_mesh_set_curves)."""
    __slots__ = ()


MAX_CURVES = 4


def _curve_rows(curves):
    """`curves` (None, or a sequence of Ellipse / 5-tuples) -> None or a validated (n, 5) float64 array."""
    if curves is None or len(curves) == 0:
        return None
    rows = np.ascontiguousarray([tuple(Ellipse(*c)) for c in curves], dtype=np.float64)
    if rows.shape[0] > MAX_CURVES:
        raise ValueError(f'at most {MAX_CURVES} curves, got {rows.shape[0]}')
    if not np.isfinite(rows).all() or (rows[:, 2] <= 0).any() or (rows[:, 3] <= 0).any() or (rows[:, 4] < 0).any():
        raise ValueError('a curve is (cx, cy, a, b, tol) with finite values, a > 0, b > 0 and tol >= 0')
    return rows


def _g(c, x, y):
    """(g, dx, dy) of the point (x, y) for the curve row c — the operations of the kernels, in their order."""
    dx, dy = x - c[0], y - c[1]
    u, v = dx / c[2], dy / c[3]
    return math.sqrt(u * u + v * v), dx, dy


def _edge_curve(rows, pa, pb):
    """Index of the lowest curve that holds both ends of a boundary edge, -1 if none does."""
    for q, c in enumerate(rows):
        if abs(_g(c, pa[0], pa[1])[0] - 1) <= c[4] and abs(_g(c, pb[0], pb[1])[0] - 1) <= c[4]:
            return q
    return -1


def _project(c, p):
    """The straight point p moved onto the curve row c along its ray from the centre (p itself at the centre)."""
    g, dx, dy = _g(c, p[0], p[1])
    if g == 0:
        return p
    return np.array([c[0] + dx / g, c[1] + dy / g])


def _curve_rows_py(rows):
    return [tuple(float(v) for v in r) for r in rows]


def doubled_areas(coord, elem):
    """Doubled signed areas (x2 - x1)(y3 - y1) - (x3 - x1)(y2 - y1) of the vertex triangles of `elem`'s first three rows."""
    x, y = np.asarray(coord, dtype=np.float64)
    a, b, c = np.asarray(elem)[0:3]
    return (x[b] - x[a]) * (y[c] - y[a]) - (x[c] - x[a]) * (y[b] - y[a])


def area_stats(coord, elem, device=None):
    """[min doubled area, sum of areas, number of triangles with doubled area <= 0, n_e] of a triangle mesh's vertex rows:
    NumPy, or — `device`, a GPU index — fep_mesh_area_stats_host."""
    elem = np.asarray(elem)
    if device is None:
        d = doubled_areas(coord, elem)
        return np.array([d.min() if d.size else np.inf, (d / 2).sum(), np.count_nonzero(d <= 0), d.size], dtype=np.float64)
    from . import _lib
    coord = np.ascontiguousarray(coord, dtype=np.float64)
    e32 = np.ascontiguousarray(elem[0:3], dtype=np.int32)
    out = np.empty(4)
    _lib.check(_lib.lib().fep_mesh_area_stats_host(int(device), e32.shape[1], coord.shape[1], _lib.ptr(e32), _lib.ptr(coord),
                                                   _lib.ptr(out)), 'fep_mesh_area_stats_host')
    return out


def _edge_map(elem):
    """undirected edge (min, max) -> list of elements that contain both vertices, in element order."""
    m = {}
    n_e = elem.shape[1]
    for i in range(n_e):
        v = (int(elem[0, i]), int(elem[1, i]), int(elem[2, i]))
        for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
            m.setdefault((a, b) if a < b else (b, a), []).append(i)
    return m


def _neighbour(m, a, b, i):
    """the element other than `i` that contains the edge {a,b} (None on the boundary)."""
    for j in m[(a, b) if a < b else (b, a)]:
        if j != i:
            return j
    return None


def create_midpoints_P2(coord, elem, device=None, curves=None):
    """TSX:1508-1626.  Returns 'coord_mid', 'surf', 'coord_ext', 'elem_ext', 'elem_ed', 'edge_el'.
    `device` (a GPU index): the same dict from the library's kernels (fep_mesh_*), see DeviceMesh.
    `curves` (a sequence of Ellipse): the midpoints of boundary edges with both ends on a curve are moved onto it, and the
    dict gains 'surf_curve' (n_boundary_edges,): the curve index of each column of 'surf', -1 for a straight edge."""
    rows = _curve_rows(curves)
    if device is not None:
        with DeviceMesh(coord, elem, device) as m:
            if rows is not None:
                m.set_curves(curves)
            return m.enrich(LagrangeElementType.P2)
    coord = np.asarray(coord, dtype=float)
    elem = np.asarray(elem)
    n_e, n_n = elem.shape[1], coord.shape[1]
    m = _edge_map(elem)
    cv = _curve_rows_py(rows) if rows is not None else None
    surf_curve = []
    coord_mid = np.zeros((2, 3 * n_e))
    elem_mid = np.zeros((3, n_e))
    elem_ed = np.zeros((3, n_e))
    edge_el = np.zeros((2, 3 * n_e))
    surf = np.zeros((3, 3 * n_e))
    ind = 0
    ind_s = 0
    # slot s of an element = its edge (A, B); the neighbour takes the midpoint at the slot given by the
    # position of B among ITS vertices (TSX:1546-1554): first -> slot 2, second -> slot 0, third -> slot 1
    slot_of_pos = (2, 0, 1)
    for i in range(n_e):
        V = (int(elem[0, i]), int(elem[1, i]), int(elem[2, i]))
        for s, (A, B) in enumerate(((V[1], V[2]), (V[2], V[0]), (V[0], V[1]))):    # TSX:1530, 1561, 1591
            if elem_mid[s, i] != 0:
                continue
            coord_mid[:, ind] = (coord[:, A] + coord[:, B]) / 2
            elem_mid[s, i] = n_n + ind
            elem_ed[s, i] = ind
            edge_el[0, ind] = i
            j = _neighbour(m, A, B, i)
            if j is not None:
                edge_el[1, ind] = j
                vj = (int(elem[0, j]), int(elem[1, j]), int(elem[2, j]))
                sj = slot_of_pos[0 if B == vj[0] else (1 if B == vj[1] else 2)]
                elem_mid[sj, j] = n_n + ind
                elem_ed[sj, j] = ind
            else:
                surf[:, ind_s] = (B, A, n_n + ind)
                ind_s += 1
                if cv is not None:
                    q = _edge_curve(cv, coord[:, A], coord[:, B]) if len(m[(A, B) if A < B else (B, A)]) == 1 else -1
                    surf_curve.append(q)
                    if q >= 0:
                        coord_mid[:, ind] = _project(cv[q], coord_mid[:, ind])
            ind += 1
    coord_mid = coord_mid[:, 0:ind]
    out = {'coord_mid': coord_mid, 'surf': surf[:, 0:ind_s], 'coord_ext': np.concatenate([coord, coord_mid], axis=1),
           'elem_ext': np.array(np.concatenate([elem, elem_mid], axis=0), dtype=int),
           'elem_ed': elem_ed, 'edge_el': edge_el[:, 0:ind]}
    if cv is not None:
        out['surf_curve'] = np.array(surf_curve, dtype=np.int64)
    return out


# Blending weights of a P4 element's interior nodes for one curved edge a -> b (include/fep.h): (l_a + l_b)^2 L_k(t) at
# t = l_b / (l_a + l_b), L_k the quartic Lagrange basis on {0, 1/4, 1/2, 3/4, 1}, for the edge's midpoint and its quarter points.
_W_MID, _W_NEAR, _W_FAR, _W_OPP = 5.0 / 18.0, 10.0 / 27.0, -2.0 / 27.0, 1.0 / 4.0


def create_midpoints_P4(coord, elem, device=None, curves=None):
    """TSX:1354-1505.  Returns 'coord_mid', 'surf', 'coord_ext', 'elem_ext'.  `device` and `curves` as in
    create_midpoints_P2: the midpoint and the two quarter points of a curved edge are moved onto the curve, by the offsets
    d_m, d_a, d_b (midpoint, quarter point nearer the edge's first vertex a, nearer its second vertex b) from their straight
    positions.  The element's interior nodes follow, so that its map stays smooth enough for a quartic: for each curved edge
    a -> b of the element in turn (V1V2, V2V3, V3V1), the interior node nearest a moves by (5/18 d_m + 10/27 d_a) - 2/27 d_b,
    the one nearest b by (5/18 d_m - 2/27 d_a) + 10/27 d_b and the third by 1/4 d_m.  These are (l_a + l_b)^2 sum_k L_k(t) d_k
    at the node's barycentric coordinates l, t = l_b / (l_a + l_b), L_k the quartic Lagrange basis on the edge's five nodes."""
    rows = _curve_rows(curves)
    if device is not None:
        with DeviceMesh(coord, elem, device) as m:
            if rows is not None:
                m.set_curves(curves)
            return m.enrich(LagrangeElementType.P4)
    coord = np.asarray(coord, dtype=float)
    elem = np.asarray(elem)
    n_e, n_n = elem.shape[1], coord.shape[1]
    m = _edge_map(elem)
    cv = _curve_rows_py(rows) if rows is not None else None
    surf_curve = []
    coord_mid = np.zeros((2, 12 * n_e))
    elem_mid = np.zeros((12, n_e))
    surf = np.zeros((5, 3 * n_e))
    ind = -1
    ind_s = -1
    for i in range(n_e):
        V1, V2, V3 = int(elem[0, i]), int(elem[1, i]), int(elem[2, i])
        c1, c2, c3 = coord[:, V1], coord[:, V2], coord[:, V3]
        coord_mid[:, ind + 1] = c1 / 2 + c2 / 4 + c3 / 4                        # TSX:1374-1381
        coord_mid[:, ind + 2] = c1 / 4 + c2 / 2 + c3 / 4
        coord_mid[:, ind + 3] = c1 / 4 + c2 / 4 + c3 / 2
        elem_mid[9, i], elem_mid[10, i], elem_mid[11, i] = n_n + ind + 1, n_n + ind + 2, n_n + ind + 3
        inner = ind + 1
        ind += 3
        for s, (A, B) in enumerate(((V1, V2), (V2, V3), (V3, V1))):            # TSX:1386, 1424, 1463
            if elem_mid[s, i] != 0:
                continue
            cA, cB = coord[:, A], coord[:, B]
            coord_mid[:, ind + 1] = (cA + cB) / 2
            coord_mid[:, ind + 2] = 3 * cA / 4 + cB / 4
            coord_mid[:, ind + 3] = cA / 4 + 3 * cB / 4
            elem_mid[s, i] = n_n + ind + 1
            elem_mid[3 + 2 * s, i] = n_n + ind + 2
            elem_mid[4 + 2 * s, i] = n_n + ind + 3
            j = _neighbour(m, A, B, i)
            if j is not None:
                vj = (int(elem[0, j]), int(elem[1, j]), int(elem[2, j]))
                sj = 0 if B == vj[0] else (1 if B == vj[1] else 2)              # TSX:1405-1416
                elem_mid[sj, j] = n_n + ind + 1
                elem_mid[3 + 2 * sj, j] = n_n + ind + 3                         # the neighbour walks the edge backwards
                elem_mid[4 + 2 * sj, j] = n_n + ind + 2
            else:
                ind_s += 1
                surf[:, ind_s] = (B, A, n_n + ind + 1, n_n + ind + 2, n_n + ind + 3)
                if cv is not None:
                    q = _edge_curve(cv, cA, cB) if len(m[(A, B) if A < B else (B, A)]) == 1 else -1
                    surf_curve.append(q)
                    if q >= 0:
                        d = []
                        for r in (1, 2, 3):
                            straight = coord_mid[:, ind + r].copy()
                            coord_mid[:, ind + r] = _project(cv[q], straight)
                            d.append(coord_mid[:, ind + r] - straight)
                        a, b, c = inner + s, inner + (s + 1) % 3, inner + (s + 2) % 3
                        coord_mid[:, a] = coord_mid[:, a] + ((_W_MID * d[0] + _W_NEAR * d[1]) + _W_FAR * d[2])
                        coord_mid[:, b] = coord_mid[:, b] + ((_W_MID * d[0] + _W_FAR * d[1]) + _W_NEAR * d[2])
                        coord_mid[:, c] = coord_mid[:, c] + _W_OPP * d[0]
            ind += 3
    coord_mid = coord_mid[:, 0:ind + 1]
    out = {'coord_mid': coord_mid, 'surf': surf[:, 0:ind_s + 1], 'coord_ext': np.concatenate([coord, coord_mid], axis=1),
           'elem_ext': np.array(np.concatenate([elem, elem_mid], axis=0), dtype=int)}
    if cv is not None:
        out['surf_curve'] = np.array(surf_curve, dtype=np.int64)
    return out


def create_midpoints(elem_type, coord, elem, device=None, curves=None):
    """TSX:1629-1633 (returns None for element types without midpoints, like the reference)."""
    t = _coerce(elem_type)
    if t is LagrangeElementType.P2:
        return create_midpoints_P2(coord, elem, device=device, curves=curves)
    if t is LagrangeElementType.P4:
        return create_midpoints_P4(coord, elem, device=device, curves=curves)
    return None


# ---------------------------------------------------------------------------------------
# the same numbering on the GPU (include/fep.h, "mesh") and uniform refinement
# ---------------------------------------------------------------------------------------
_FEP_TYPE = {LagrangeElementType.P2: 2, LagrangeElementType.P4: 5}
_INFO = ('n_e', 'n_n', 'n_edges', 'n_boundary_edges', 'n_nonmanifold', 'n_inconsistent', 'n_degenerate')


class DeviceMesh:
    """A P1 triangle mesh analysed on GPU `device` (fep_mesh_create): half-edges matched, owners and prefix sums ready.
    `coord` (2, n_n) and `elem` (3, n_e) are host arrays, or — `on_device=True` — torch tensors of that GPU (float64 /
    int32, contiguous).  `info` holds the counts of fep_mesh_info.  The device path numbers edge-manifold, consistently
    oriented meshes only: on any other, `enrich` / `refine` raise ValueError and write nothing (the host functions,
    device=None, keep the reference's visit-order-dependent result for those)."""

    def __init__(self, coord, elem, device, on_device=False):
        from . import _lib
        self._lib, self._h, self.device, self.n_curves, self.marks = _lib, None, int(device), 0, None
        if on_device:
            if elem.dtype.itemsize != 4 or coord.dtype.itemsize != 8 or not (elem.is_contiguous() and coord.is_contiguous()):
                raise ValueError('device meshes are contiguous int32 / float64 tensors')
            n_e, n_n = int(elem.shape[1]), int(coord.shape[1])
            pe, pc, stream = elem.data_ptr(), coord.data_ptr(), self._stream()
            self._keep = (elem, coord)
        else:
            coord = np.ascontiguousarray(coord, dtype=np.float64)
            e64 = np.asarray(elem)
            if e64.ndim != 2 or e64.shape[0] != 3 or coord.ndim != 2 or coord.shape[0] != 2:
                raise ValueError(f'expected (2, n_n) coordinates and (3, n_e) vertex ids, got {coord.shape} and {e64.shape}')
            if e64.size and (e64.min() < -2 ** 31 or e64.max() >= 2 ** 31):
                raise _lib.FepError(-5, 'fep_mesh_create')
            e32 = np.ascontiguousarray(e64, dtype=np.int32)
            n_e, n_n = e32.shape[1], coord.shape[1]
            pe, pc, stream = _lib.ptr(e32), _lib.ptr(coord), None
        h = C.c_void_p()
        _lib.check(_lib.lib().fep_mesh_create(C.byref(h), self.device, stream, n_e, n_n, pe, pc, int(bool(on_device))),
                   'fep_mesh_create')
        self._h = h
        info = np.zeros(7, dtype=np.int64)
        _lib.check(_lib.lib().fep_mesh_info(h, info.ctypes.data_as(_lib.c_i64_p)), 'fep_mesh_info')
        self.info = dict(zip(_INFO, (int(v) for v in info)))

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if self._h is not None:
            self._lib.lib().fep_mesh_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _accepted(self):
        i = self.info
        if i['n_nonmanifold'] or i['n_inconsistent'] or i['n_degenerate']:
            raise ValueError(f"the device path numbers edge-manifold, consistently oriented meshes only: "
                             f"n_nonmanifold={i['n_nonmanifold']}, n_inconsistent={i['n_inconsistent']}, "
                             f"n_degenerate={i['n_degenerate']}; use the host functions (device=None) for this mesh")

    def set_curves(self, curves):
        """The curved boundaries of the next enrich / refine calls (fep_mesh_set_curves): a sequence of Ellipse, at most 4;
        None or an empty one clears them."""
        rows = _curve_rows(curves)
        n = 0 if rows is None else rows.shape[0]
        self._lib.check(self._lib.lib().fep_mesh_set_curves(self._h, n, self._lib.ptr(rows) if n else None), 'fep_mesh_set_curves')
        self.n_curves = n

    def surf_curve(self, elem_type):
        """Curve index (-1: straight) of every boundary edge, in the order of `elem_type`'s 'surf' columns; int64."""
        self._accepted()
        out = np.empty(self.info['n_boundary_edges'], dtype=np.int32)
        self._lib.check(self._lib.lib().fep_mesh_surf_curve_host(self._h, _FEP_TYPE[_coerce(elem_type)], self._lib.ptr(out)),
                        'fep_mesh_surf_curve_host')
        return out.astype(np.int64)

    def surf_curve_dev(self, elem_type):
        """Device-resident form: an int32 tensor written on the current stream."""
        import torch
        self._accepted()
        out = torch.empty(self.info['n_boundary_edges'], dtype=torch.int32, device=torch.device('cuda', self.device))
        self._lib.check(self._lib.lib().fep_mesh_surf_curve_dev(self._h, self._stream(), _FEP_TYPE[_coerce(elem_type)],
                                                                C.c_void_p(out.data_ptr())), 'fep_mesh_surf_curve_dev')
        return out

    def new_nodes(self, elem_type):
        t = _coerce(elem_type)
        return self.info['n_edges'] if t is LagrangeElementType.P2 else 3 * self.info['n_e'] + 3 * self.info['n_edges']

    def enrich(self, elem_type):
        """The dict of create_midpoints_P2 / _P4 (same keys, shapes, dtypes and bits), host arrays."""
        t = _coerce(elem_type)
        self._accepted()
        i, p2 = self.info, t is LagrangeElementType.P2
        n_tot = i['n_n'] + self.new_nodes(t)
        elem_ext = np.empty((6 if p2 else 15, i['n_e']), dtype=np.int32)
        coord_ext = np.empty((2, n_tot))
        surf = np.empty((3 if p2 else 5, i['n_boundary_edges']), dtype=np.int32)
        elem_ed = np.empty((3, i['n_e']), dtype=np.int32) if p2 else None
        edge_el = np.empty((2, i['n_edges']), dtype=np.int32) if p2 else None
        ptr = self._lib.ptr
        self._lib.check(self._lib.lib().fep_mesh_enrich_host(self._h, _FEP_TYPE[t], ptr(elem_ext), ptr(coord_ext), ptr(surf),
                                                             ptr(elem_ed), ptr(edge_el)), 'fep_mesh_enrich_host')
        out = {'coord_mid': coord_ext[:, i['n_n']:], 'surf': surf.astype(np.float64), 'coord_ext': coord_ext,
               'elem_ext': elem_ext.astype(int)}
        if p2:
            out['elem_ed'], out['edge_el'] = elem_ed.astype(np.float64), edge_el.astype(np.float64)
        if self.n_curves:
            out['surf_curve'] = self.surf_curve(t)
        return out

    def enrich_dev(self, elem_type):
        """Device-resident form: torch tensors (elem_ext int32, coord_ext, surf int32[, elem_ed, edge_el int32]) written on
        the current stream; nothing is synchronised."""
        import torch
        t = _coerce(elem_type)
        self._accepted()
        i, p2 = self.info, t is LagrangeElementType.P2
        dev = torch.device('cuda', self.device)
        n_tot = i['n_n'] + self.new_nodes(t)
        out = [torch.empty((6 if p2 else 15, i['n_e']), dtype=torch.int32, device=dev),
               torch.empty((2, n_tot), dtype=torch.float64, device=dev),
               torch.empty((3 if p2 else 5, i['n_boundary_edges']), dtype=torch.int32, device=dev)]
        if p2:
            out += [torch.empty((3, i['n_e']), dtype=torch.int32, device=dev),
                    torch.empty((2, i['n_edges']), dtype=torch.int32, device=dev)]
        ptrs = [C.c_void_p(a.data_ptr()) for a in out] + [None] * (5 - len(out))
        self._lib.check(self._lib.lib().fep_mesh_enrich_dev(self._h, self._stream(), _FEP_TYPE[t], *ptrs), 'fep_mesh_enrich_dev')
        return tuple(out)

    def refine(self):
        """One level of uniform refinement -> (coordinates (2, n_n + n_edges), elements (3, 4 n_e) int64), host arrays."""
        self._accepted()
        i = self.info
        child = np.empty((3, 4 * i['n_e']), dtype=np.int32)
        coord_ext = np.empty((2, i['n_n'] + i['n_edges']))
        self._lib.check(self._lib.lib().fep_mesh_refine_host(self._h, self._lib.ptr(child), self._lib.ptr(coord_ext)),
                        'fep_mesh_refine_host')
        return coord_ext, child.astype(np.int64)

    def refine_dev(self):
        """Device-resident form -> torch tensors (coordinates float64, elements int32) on the current stream."""
        import torch
        self._accepted()
        i = self.info
        dev = torch.device('cuda', self.device)
        child = torch.empty((3, 4 * i['n_e']), dtype=torch.int32, device=dev)
        coord_ext = torch.empty((2, i['n_n'] + i['n_edges']), dtype=torch.float64, device=dev)
        self._lib.check(self._lib.lib().fep_mesh_refine_dev(self._h, self._stream(), C.c_void_p(child.data_ptr()),
                                                            C.c_void_p(coord_ext.data_ptr())), 'fep_mesh_refine_dev')
        return coord_ext, child

    def mark(self, marked, on_device=False):
        """Closes the marks `marked` (n_e; non-zero = marked; a host array, or — `on_device` — a uint8 / bool tensor of this
        GPU) under the longest-edge rule and keeps them in the mesh for refine_marked (fep_mesh_mark; synchronises the
        stream).  Returns {'n_child', 'n_new_nodes', 'n_marked_elements' (elements with a marked edge), 'n_sweeps'}."""
        self._accepted()
        n_e = self.info['n_e']
        if on_device:
            if marked.dtype.itemsize != 1 or tuple(marked.shape) != (n_e,) or not marked.is_contiguous():
                raise ValueError(f'device marks are a contiguous uint8 / bool tensor of ({n_e},)')
            pm, stream, keep = C.c_void_p(marked.data_ptr()), self._stream(), marked
        else:
            keep = np.ascontiguousarray(np.asarray(marked) != 0, dtype=np.uint8)
            if keep.shape != (n_e,):
                raise ValueError(f'marks: one entry per element ({n_e},), got {keep.shape}')
            pm, stream = self._lib.ptr(keep), None
        out = np.zeros(4, dtype=np.int64)
        self._lib.check(self._lib.lib().fep_mesh_mark(self._h, stream, pm, int(bool(on_device)), out.ctypes.data_as(self._lib.c_i64_p)),
                        'fep_mesh_mark')
        self.marks = dict(zip(('n_child', 'n_new_nodes', 'n_marked_elements', 'n_sweeps'), (int(v) for v in out)))
        return dict(self.marks)

    def _marked(self):
        self._accepted()
        if self.marks is None:
            raise ValueError('refine_marked needs the marks: call mark() first')
        return self.marks['n_child'], self.info['n_n'] + self.marks['n_new_nodes']

    def refine_marked(self):
        """One level of longest-edge refinement of the marked elements -> (coordinates (2, n_n + n_new_nodes), elements
        (3, n_child) int64, parent (n_child) int64), host arrays, bit-equal to refine_marked(device=None)."""
        n_child, n_tot = self._marked()
        child = np.empty((3, n_child), dtype=np.int32)
        coord_ext = np.empty((2, n_tot))
        parent = np.empty(n_child, dtype=np.int32)
        ptr = self._lib.ptr
        self._lib.check(self._lib.lib().fep_mesh_refine_marked_host(self._h, ptr(child), ptr(coord_ext), ptr(parent)),
                        'fep_mesh_refine_marked_host')
        return coord_ext, child.astype(np.int64), parent.astype(np.int64)

    def refine_marked_dev(self):
        """Device-resident form -> torch tensors (coordinates float64, elements int32, parent int32) on the current stream."""
        import torch
        n_child, n_tot = self._marked()
        dev = torch.device('cuda', self.device)
        child = torch.empty((3, n_child), dtype=torch.int32, device=dev)
        coord_ext = torch.empty((2, n_tot), dtype=torch.float64, device=dev)
        parent = torch.empty(n_child, dtype=torch.int32, device=dev)
        self._lib.check(self._lib.lib().fep_mesh_refine_marked_dev(self._h, self._stream(), C.c_void_p(child.data_ptr()),
                                                                   C.c_void_p(coord_ext.data_ptr()), C.c_void_p(parent.data_ptr())),
                        'fep_mesh_refine_marked_dev')
        return coord_ext, child, parent

    def child_corners(self):
        """Corner codes (3, n_child) uint8 of refine_marked's children (fep_mesh_child_corners_host), a host array bit-equal
        to child_corners(coord, elem, marked)."""
        n_child, _ = self._marked()
        corners = np.empty((3, n_child), dtype=np.uint8)
        self._lib.check(self._lib.lib().fep_mesh_child_corners_host(self._h, self._lib.ptr(corners)), 'fep_mesh_child_corners_host')
        return corners

    def child_corners_dev(self):
        """Device-resident form -> a (3, n_child) uint8 tensor written on the current stream; nothing is synchronised."""
        import torch
        n_child, _ = self._marked()
        corners = torch.empty((3, n_child), dtype=torch.uint8, device=torch.device('cuda', self.device))
        self._lib.check(self._lib.lib().fep_mesh_child_corners_dev(self._h, self._stream(), C.c_void_p(corners.data_ptr())),
                        'fep_mesh_child_corners_dev')
        return corners


def area_stats_dev(coord_d, elem_d, device, out=None):
    """fep_mesh_area_stats_dev on torch tensors of GPU `device` (coord (2, n_n) float64, elem (3, n_e) int32, contiguous),
    on the current stream -> a float64 tensor of 4 (`out`, or a new one); nothing is synchronised."""
    import torch
    from . import _lib
    if elem_d.dtype != torch.int32 or coord_d.dtype != torch.float64 or elem_d.shape[0] != 3 or coord_d.shape[0] != 2 \
            or not (elem_d.is_contiguous() and coord_d.is_contiguous()):
        raise ValueError('area statistics take contiguous (3, n_e) int32 / (2, n_n) float64 tensors')
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=torch.device('cuda', device))
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(_lib.lib().fep_mesh_area_stats_dev(int(device), stream, int(elem_d.shape[1]), int(coord_d.shape[1]),
                                                  C.c_void_p(elem_d.data_ptr()), C.c_void_p(coord_d.data_ptr()),
                                                  C.c_void_p(out.data_ptr())), 'fep_mesh_area_stats_dev')
    return out


def _folded(level, stats):
    return ValueError(f'refinement level {level}: {int(stats[2])} of {int(stats[3])} triangles have a non-positive area '
                      f'(smallest doubled area {stats[0]:.3e}) after projection onto the curves')


def refine_uniform(coord, elem, levels=1, device=None, curves=None):
    """Uniform (red) refinement of a P1 triangle mesh, `levels` times -> (coordinates, elements (3, 4**levels n_e) int64).
    No counterpart in the reference.  One level = the P2 enrichment: the new vertices are the P2 midside nodes, with
    create_midpoints_P2's ids and coordinates (old nodes keep their ids and coordinates), and with its rows
    (V1, V2, V3, m23, m31, m12) the children 4i .. 4i + 3 of element i are (V1, m12, m31), (m12, V2, m23), (m31, m23, V3),
    (m12, m23, m31).  Orientation is preserved.  Without `curves` boundaries are refined as polygons.  `curves` (a sequence
    of Ellipse, e.g. the tunnel's hole): at every level the new vertex of a boundary edge with both ends on a curve is moved
    onto it, so the boundary converges to the curve; every level is then checked with the area statistics
    (fep_mesh_area_stats_dev on the GPU, NumPy on the host) and a level with a child of non-positive area raises
    ValueError naming the level and the count.  `device` (a GPU index): the levels are chained on the GPU without a host
    round trip (DeviceMesh; edge-manifold, consistently oriented meshes only), bit-equal to the host form without curves."""
    if levels < 0:
        raise ValueError('levels must be >= 0')
    rows = _curve_rows(curves)
    if device is not None and levels > 0:
        import torch
        stats = torch.empty((levels, 4), dtype=torch.float64, device=torch.device('cuda', device)) if rows is not None else None
        m = DeviceMesh(coord, elem, device)
        try:
            for lv in range(levels):
                if rows is not None:
                    m.set_curves(curves)
                c_d, e_d = m.refine_dev()
                if rows is not None:
                    area_stats_dev(c_d, e_d, device, out=stats[lv])
                m.close()
                if lv + 1 < levels:
                    m = DeviceMesh(c_d, e_d, device, on_device=True)
        finally:
            m.close()
        if rows is not None:
            for lv, st in enumerate(stats.cpu().numpy()):
                if st[2] > 0:
                    raise _folded(lv + 1, st)
        return c_d.cpu().numpy(), e_d.cpu().numpy().astype(np.int64)
    coord, elem = np.asarray(coord, dtype=float), np.asarray(elem).astype(np.int64)
    for lv in range(levels):
        h = create_midpoints_P2(coord, elem, curves=curves)
        V1, V2, V3, m23, m31, m12 = h['elem_ext']
        elem = np.stack([np.stack([V1, m12, m31]), np.stack([m12, V2, m23]), np.stack([m31, m23, V3]),
                         np.stack([m12, m23, m31])], axis=2).reshape(3, -1).astype(np.int64)
        coord = h['coord_ext']
        if rows is not None:
            st = area_stats(coord, elem)
            if st[2] > 0:
                raise _folded(lv + 1, st)
    return coord, elem


# ---------------------------------------------------------------------------------------
# refinement of marked triangles: conforming longest-edge bisection (Rivara's 4T-LE; include/fep.h, fep_mesh_mark)
# ---------------------------------------------------------------------------------------
def _half_edges(elem):
    """(nbr (3, n_e): 3 j + edge of j across edge k of i, -1 on the boundary; owned (3, n_e) bool) of an edge-manifold,
    consistently oriented mesh without degenerate triangles — ValueError on any other, as the device path."""
    n_e = elem.shape[1]
    half = {}
    for i in range(n_e):
        v = (int(elem[0, i]), int(elem[1, i]), int(elem[2, i]))
        if v[0] == v[1] or v[1] == v[2] or v[2] == v[0]:
            raise ValueError(f'marked refinement: element {i} names a vertex twice')
        for k in range(3):
            if half.setdefault((v[k], v[(k + 1) % 3]), 3 * i + k) != 3 * i + k:
                raise ValueError('marked refinement numbers edge-manifold, consistently oriented meshes only: '
                                 f'two elements walk the edge {(v[k], v[(k + 1) % 3])} the same way')
    nbr = np.full((3, n_e), -1, dtype=np.int64)
    for (a, b), code in half.items():
        nbr[code % 3, code // 3] = half.get((b, a), -1)
    owned = (nbr < 0) | (np.arange(n_e)[None, :] < nbr // 3)
    return nbr, owned


def reference_edges(coord, elem):
    """The reference (longest) edge of every triangle: edge k runs from vertex k to vertex (k + 1) % 3, its squared length
    is dx dx + dy dy of the vertex chord in the element's own walking direction, and the slots are compared in the order
    0, 1, 2 with a strict >, so the lowest slot wins a tie."""
    x, y = np.asarray(coord, dtype=np.float64)
    elem = np.asarray(elem)
    L = []
    for k in range(3):
        dx, dy = x[elem[(k + 1) % 3]] - x[elem[k]], y[elem[(k + 1) % 3]] - y[elem[k]]
        L.append(dx * dx + dy * dy)
    r = np.zeros(elem.shape[1], dtype=np.int64)
    best = L[0].copy()
    for k in (1, 2):
        longer = L[k] > best
        r[longer] = k
        best[longer] = L[k][longer]
    return r


def _closed_marks(nbr, ref, marked):
    """Own-half-edge bits (n_e) uint8 of the least fixpoint: a marked element sets all three, and an element with any
    marked edge (own bit or the neighbour's) sets its reference edge.  A work list; the fixpoint does not depend on the order."""
    n_e = ref.size
    bits = np.where(marked, 7, 0).astype(np.uint8)
    todo = [int(i) for i in np.flatnonzero(marked)]
    while todo:
        i = todo.pop()
        for k in range(3):                                   # every own bit may be new to the neighbour across it
            nb = int(nbr[k, i])
            if nb < 0 or not (bits[i] >> k) & 1:
                continue
            j = nb // 3
            want = bits[j] | (1 << int(ref[j]))
            if want != bits[j]:
                bits[j] = want
                todo.append(j)
    return bits


def _marked_edges(coord, elem, marked):
    """What _refine_marked_host and child_corners share: (coord float64, elem int64, nbr, owned, ref, state), state (3, n_e)
    bool = edge k of element i is marked under the closed marks (own bit or the neighbour's)."""
    coord = np.asarray(coord, dtype=np.float64)
    elem = np.asarray(elem).astype(np.int64)
    n_e = elem.shape[1]
    marked = np.asarray(marked)
    if marked.shape != (n_e,):
        raise ValueError(f'marks: one entry per element ({n_e},), got {marked.shape}')
    marked = marked != 0
    nbr, owned = _half_edges(elem)
    ref = reference_edges(coord, elem)
    bits = _closed_marks(nbr, ref, marked)
    state = np.zeros((3, n_e), dtype=bool)
    for k in range(3):
        j, kj = nbr[k] // 3, nbr[k] % 3
        state[k] = ((bits >> k) & 1).astype(bool) | ((nbr[k] >= 0) & (((bits[j] >> kj) & 1) != 0))
    return coord, elem, nbr, owned, ref, state


def child_corners(coord, elem, marked):
    """Corner codes (3, n_child) uint8 of refine_marked(coord, elem, marked)'s children (include/fep.h, "state transfer across
    refinement"): corners[k, ch] says what vertex row k of child ch is in its parent — 0, 1, 2 the parent's vertex row,
    3, 4, 5 the node on the parent's edge 0, 1, 2.  With r the reference edge, a = r, b = (r + 1) % 3, c = (r + 2) % 3,
    m = 3 + a, p = 3 + b, q = 3 + c the child rows (a, m, q), (q, m, c) | (a, m, c) and (m, b, p), (m, p, c) | (m, b, c) of
    refine_marked hold exactly those codes; an element without a marked edge gets (0, 1, 2).  The codes do not depend on
    curves.  The twin of DeviceMesh.child_corners, bit-equal to it."""
    coord, elem, nbr, owned, ref, state = _marked_edges(coord, elem, marked)
    out = []
    for i in range(elem.shape[1]):
        if not state[:, i].any():
            out.append((0, 1, 2))
            continue
        a, b, c = ((int(ref[i]) + s) % 3 for s in range(3))
        m, p, q = 3 + a, 3 + b, 3 + c
        out += ([(a, m, q), (q, m, c)] if state[c, i] else [(a, m, c)]) + ([(m, b, p), (m, p, c)] if state[b, i] else [(m, b, c)])
    return np.ascontiguousarray(np.array(out, dtype=np.uint8).T)


def _refine_marked_host(coord, elem, marked, rows):
    coord, elem, nbr, owned, ref, state = _marked_edges(coord, elem, marked)
    n_e, n_n = elem.shape[1], coord.shape[1]
    cv = _curve_rows_py(rows) if rows is not None else None
    # the P2 edge order: owners in element order, their owned slots in the visit order 1, 2, 0
    new_of = np.full((3, n_e), -1, dtype=np.int64)
    new_xy = []
    for i in range(n_e):
        for k in (1, 2, 0):
            if not (owned[k, i] and state[k, i]):
                continue
            A, B = int(elem[k, i]), int(elem[(k + 1) % 3, i])
            mid = (coord[:, A] + coord[:, B]) / 2
            if nbr[k, i] < 0 and cv is not None:
                q = _edge_curve(cv, coord[:, A], coord[:, B])
                if q >= 0:
                    mid = _project(cv[q], mid)
            new_of[k, i] = n_n + len(new_xy)
            new_xy.append(mid)
            if nbr[k, i] >= 0:
                new_of[nbr[k, i] % 3, nbr[k, i] // 3] = new_of[k, i]
    child, parent = [], []
    for i in range(n_e):
        if not state[:, i].any():
            child.append((int(elem[0, i]), int(elem[1, i]), int(elem[2, i])))
            parent.append(i)
            continue
        r = int(ref[i])
        a, b, c = (int(elem[(r + s) % 3, i]) for s in range(3))
        m, p, q = (int(new_of[(r + s) % 3, i]) for s in range(3))
        rows_i = ([(a, m, q), (q, m, c)] if q >= 0 else [(a, m, c)]) + ([(m, b, p), (m, p, c)] if p >= 0 else [(m, b, c)])
        child += rows_i
        parent += [i] * len(rows_i)
    coord_ext = np.concatenate([coord, np.array(new_xy, dtype=np.float64).reshape(-1, 2).T], axis=1)
    return coord_ext, np.ascontiguousarray(np.array(child, dtype=np.int64).T), np.array(parent, dtype=np.int64)


def refine_marked(coord, elem, marked, device=None, curves=None):
    """One level of conforming longest-edge bisection (Rivara's 4T-LE) of the elements `marked` (n_e; non-zero = marked)
    -> (coordinates (2, n_n + new), elements (3, n_child) int64, parent (n_child) int64).  No counterpart in the reference.
    The rule (include/fep.h, fep_mesh_mark): a marked element marks its three edges; an element with any marked edge must
    have its reference edge (reference_edges: the longest, lowest slot on a tie) marked — the least fixpoint, which does not
    depend on the order of evaluation.  Every marked edge gets one node, numbered n_n + its rank among the marked edges in
    the P2 edge order, at the coordinates of create_midpoints_P2's midside node (moved onto `curves` by the same rule), so
    that with every element marked the coordinates equal refine_uniform's.  With a = vertex r (r the reference edge),
    b, c the next two and m, p, q the nodes of ab, bc, ca, an element with marked edges becomes (a, m, q), (q, m, c) — or
    (a, m, c) without q — followed by (m, b, p), (m, p, c) — or (m, b, c) without p; one without stays as it is.  Children
    follow their parents in element order; orientation is preserved.  `device` (a GPU index): the kernels (DeviceMesh.mark,
    .refine_marked), bit-equal to this loop.  With `curves` the result is checked with the area statistics and a child of
    non-positive area raises ValueError."""
    rows = _curve_rows(curves)
    if device is not None:
        with DeviceMesh(coord, elem, device) as m:
            if rows is not None:
                m.set_curves(curves)
            m.mark(marked)
            out = m.refine_marked()
    else:
        out = _refine_marked_host(coord, elem, marked, rows)
    if rows is not None:
        st = area_stats(out[0], out[1], device=device)
        if st[2] > 0:
            raise _folded(1, st)
    return out


def mark_plastic(ind_p, elem, n_q, rings=1):
    """Marks for refine_marked from a step's plastic flags: `ind_p` (n_e n_q), element by element as the drivers' steps
    return them.  An element is marked if any of its n_q integration points is plastic; then, `rings` times, so is every
    element that shares a vertex (rows 0..2 of `elem`) with a marked one.  Returns a bool (n_e) array."""
    elem = np.asarray(elem)
    n_e = elem.shape[1]
    flags = np.asarray(ind_p).reshape(-1) != 0
    if flags.size != n_e * n_q:
        raise ValueError(f'{flags.size} flags for {n_e} elements of {n_q} integration points')
    marked = flags.reshape(n_e, n_q).any(axis=1)
    n_n = int(elem[0:3].max()) + 1
    for _ in range(rings):
        touched = np.zeros(n_n, dtype=bool)
        touched[elem[0:3][:, marked]] = True
        marked = touched[elem[0:3]].any(axis=0)
    return marked

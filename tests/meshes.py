"""
Meshes for the element-route tests (test_element_route_gpu.py, test_elem_ref.py, test_parity_gpu.py,
test_sharding_gpu.py): the structured rectangles of every type, P4 included (a P1 rectangle raised through
create_midpoints_P4, the reference's numbering), Delaunay triangulations raised to P2 / P4, and the transformations the
tests apply to them (jitter with curved edges, random renumbering, mixed orientation, trailing elements dropped).
"""
import re
from importlib import import_module

import numpy as np

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from elem_ref import reverse_elements

fep = import_module('fem-elastoplasticity_amd')


def raise_p1(t, elem, coord):
    """A P1 mesh as t (P1, P2, P4): midside / interior nodes from create_midpoints_P2 / _P4."""
    if t == 'P1':
        return np.asarray(elem, dtype=np.int64), np.asarray(coord, dtype=float)
    m = (fep.create_midpoints_P2 if t == 'P2' else fep.create_midpoints_P4)(coord, elem)
    return np.ascontiguousarray(m['elem_ext'], dtype=np.int64), np.ascontiguousarray(m['coord_ext'])


def rect(t, nx, ny, size_x=10.0, size_y=10.0):
    """(elements, coordinates) of the structured nx x ny cell rectangle of type t; P4 is the P1 rectangle raised."""
    if t == 'P4':
        m = fep.rect_mesh(nx, ny, 'P1', size_x, size_y)
        return raise_p1('P4', m['elements'], m['coordinates'])
    m = fep.rect_mesh(nx, ny, t, size_x, size_y)
    return m['elements'], m['coordinates'].copy()


def square(t, n, size=10.0):
    return rect(t, n, n, size, size)


def delaunay(t, M, rng, size=10.0):
    """Delaunay triangulation of an (M+1)^2 grid with its interior points jittered by up to 0.35 of the spacing, as t."""
    from scipy.spatial import Delaunay
    g = np.stack(np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing='xy')).reshape(2, -1).astype(float)
    inner = (g[0] > 0) & (g[0] < M) & (g[1] > 0) & (g[1] < M)
    g[:, inner] += rng.uniform(-0.35, 0.35, size=(2, int(inner.sum())))
    coord = g * (size / M)
    elem = Delaunay(coord.T).simplices.T.astype(np.int64)
    return raise_p1(t, elem, coord)


def jitter(elem, coord, amount, rng):
    """Every node off the bounding box's edges moved by up to `amount` times the smallest edge of its elements in each
    direction — midside and interior nodes too, so that P2 / Q2 / P4 elements get curved edges."""
    coord = np.array(coord, dtype=float, copy=True)
    x, y = coord
    lo, hi = coord.min(axis=1), coord.max(axis=1)
    n_p = elem.shape[0]
    nv = 4 if n_p in (4, 8) else 3
    h = np.full(coord.shape[1], np.inf)
    for a in range(nv):                                                     # element edges between vertices
        b = (a + 1) % nv
        le = np.hypot(x[elem[a]] - x[elem[b]], y[elem[a]] - y[elem[b]])
        for r in range(n_p):
            np.minimum.at(h, elem[r], le)
    scale = np.where(np.isfinite(h), h, 0.0) / {3: 1, 6: 2, 4: 1, 8: 2, 15: 4}[n_p]   # spacing between nodes
    inner = (x > lo[0]) & (x < hi[0]) & (y > lo[1]) & (y < hi[1])
    coord[:, inner] += amount * scale[inner] * rng.uniform(-1, 1, size=(2, int(inner.sum())))
    return coord


def renumber(elem, coord, rng):
    """Random node and element numbering."""
    perm = rng.permutation(coord.shape[1])                                  # new node i is old node perm[i]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    return np.ascontiguousarray(inv[elem][:, rng.permutation(elem.shape[1])]), np.ascontiguousarray(coord[:, perm])


def mixed_orientation(elem, rng):
    """Half of the elements (at random) locally renumbered to the reverse orientation (det < 0, same shape)."""
    return reverse_elements(elem, rng.random(elem.shape[1]) < 0.5)


def drop_last(elem, k):
    """The mesh without its last k elements (their nodes stay: nodes of no element)."""
    return np.ascontiguousarray(elem[:, :elem.shape[1] - k]) if k else elem


def named(t, name, rng):
    """The named meshes of the element-route tests (test_element_route_gpu.py, model_step_cases.py) -> (elem, coord,
    typical element size h, state kind of the element-route test)."""
    n = {'P1': 24, 'P2': 14, 'Q1': 24, 'Q2': 12, 'P4': 8}[t]
    if name.startswith('structured'):
        nx, ny, k = [int(v) for v in re.match(r'structured_(\d+)x(\d+)-(\d+)', name).groups()]
        elem, coord = rect(t, nx, ny)
        return drop_last(elem, k), coord, 10 / max(nx, ny), ('plain', 'wide', 'tsx', 'accept', 'plain')[nx % 5]
    if name in ('strip1', 'strip2'):
        nx = {'P1': 301, 'P2': 151, 'Q1': 601, 'Q2': 149, 'P4': 61}[t]
        elem, coord = rect(t, nx, int(name[-1]), 10.0, 10.0 * int(name[-1]) / nx)
        return elem, coord, 10 / nx, 'accept' if name == 'strip1' else 'wide'
    if name == 'aniso':                                            # cells 1 : 1000
        elem, coord = rect(t, 10, 10, 10.0, 0.01)
        return elem, coord, 1e-3, 'plain'
    if name == 'delaunay':
        elem, coord = renumber(*delaunay(t, n, rng), rng)
        return elem, coord, 10 / n, 'tsx'
    elem, coord = square(t, n)
    coord = jitter(elem, coord, 0.15 if name == 'curved' else 0.1, rng)
    if name == 'renumbered':
        elem, coord = renumber(elem, coord, rng)
        return elem, coord, 10 / n, 'wide'
    if name == 'mixed':
        return mixed_orientation(elem, rng), coord, 10 / n, 'accept'
    return elem, coord, 10 / n, 'plain'

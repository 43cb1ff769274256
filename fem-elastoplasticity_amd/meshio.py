"""
On-disk mesh / CSV input and output of the tsx-tunnel flavour.

  load_tsx_mesh        tsx-tunnel/pythonFEM.py:1687-1690: `coord.csv` (2 rows: x, y) and `elem.csv` (3 rows of 1-based
                       vertex ids) -> (coordinates (2, n_n) float64, elements (n_p, n_e) int64 0-based), with the P2 / P4
                       midpoints added as the reference's `create_midpoints` does (TSX:1629-1633 dispatches on the type;
                       P1 — for which the reference returns None, SURVEY C11 — gives the vertices as read);
                       `refine` refines the P1 mesh uniformly first (refine_uniform: no counterpart in the reference)
  prepare_tsx_mesh     the same steps on arrays: refine, renumber along a Morton curve, raise to the element type
  dump_free_dof_csv    the dumps the reference keeps beside its driver (k_tangent_qq.csv, f0q.csv, fq.csv: tangent and
                       load / residual vectors restricted to the free DOFs, dense, comma separated) from this package's
                       results, for side-by-side comparison
"""
import os

import numpy as np

import time

from .mesh import renumber_for_locality
from .midpoints import create_midpoints, refine_uniform
from .tables import LagrangeElementType, _coerce


def prepare_tsx_mesh(coords, elem, element_type='P1', refine=0, renumber=False, device=None, curves=None):
    """P1 triangles (`coords` (2, n_n), `elem` (3, n_e) 0-based) -> the mesh a driver runs on: refined `refine` times
    (refine_uniform), then — `renumber` — numbered along a Morton curve (renumber_for_locality, on the host: refinement
    appends each level's nodes at the end, which scatters a node's neighbours over memory), then raised to
    `element_type` (create_midpoints).  `device` (a GPU index) runs refinement and enrichment on the GPU, None on the host.
    `curves` (a sequence of Ellipse, e.g. tsx_tunnel.TSX_HOLE): the new nodes of boundary edges with both ends on a curve are
    moved onto it, at every refinement level and in the enrichment (refine_uniform, create_midpoints).
    Returns (coordinates float64, elements int64, node_of_input, seconds): node_of_input[n] = the id of input node n in
    the result (vertices keep their ids under refinement and enrichment; None when not renumbered), seconds =
    {'refine', 'renumber', 'enrich'}."""
    t = _coerce(element_type)
    if t not in (LagrangeElementType.P1, LagrangeElementType.P2, LagrangeElementType.P4):
        raise ValueError('triangle meshes: element_type must be P1, P2 or P4')
    coords, elem = np.asarray(coords, dtype=np.float64), np.asarray(elem)
    if elem.shape[0] != 3:
        raise ValueError(f'refine / renumber start from the P1 mesh: (3, n_e) vertex ids, got {elem.shape}')
    n_in = coords.shape[1]
    clock = [time.perf_counter()]
    if refine:
        coords, elem = refine_uniform(coords, elem, levels=refine, device=device, curves=curves)
    clock.append(time.perf_counter())
    node_of_input = None
    if renumber:
        elem, coords, node_perm, _ = renumber_for_locality(elem, coords)
        inv = np.empty_like(node_perm)
        inv[node_perm] = np.arange(node_perm.size)
        node_of_input = inv[:n_in]
    clock.append(time.perf_counter())
    if t is not LagrangeElementType.P1:
        ext = create_midpoints(t, coords, elem, device=device, curves=curves)
        coords, elem = ext['coord_ext'], ext['elem_ext']
    clock.append(time.perf_counter())
    seconds = dict(zip(('refine', 'renumber', 'enrich'), (b - a for a, b in zip(clock[:-1], clock[1:]))))
    return np.asarray(coords, dtype=np.float64), np.asarray(elem, dtype=np.int64), node_of_input, seconds


def load_tsx_mesh(directory='.', element_type='P1', coord_file='coord.csv', elem_file='elem.csv', refine=0, device=None,
                  curves=None):
    """(coordinates, elements) of the CSV mesh in `directory`, elements 0-based (TSX:1687-1688), midpoints per TSX:1690.
    `refine` > 0: the P1 mesh is refined uniformly that many times before the midpoints are added; `device` (a GPU
    index) runs refinement and midpoints on the GPU (None: on the host); `curves` as in prepare_tsx_mesh."""
    coords = np.genfromtxt(os.path.join(directory, coord_file), delimiter=',', ndmin=2)
    elem = np.genfromtxt(os.path.join(directory, elem_file), delimiter=',', dtype=int, ndmin=2) - 1
    if coords.shape[0] != 2 or elem.shape[0] != 3:
        raise ValueError(f'expected a 2-row coordinate file and a 3-row element file, got {coords.shape} and {elem.shape}')
    if elem.min() < 0 or elem.max() >= coords.shape[1]:
        raise IndexError('element file refers to nodes the coordinate file does not hold (ids are 1-based on disk)')
    t = _coerce(element_type)
    if refine or device is not None:
        return prepare_tsx_mesh(coords, elem, t, refine=refine, device=device, curves=curves)[:2]
    if t in (LagrangeElementType.P2, LagrangeElementType.P4):
        ext = create_midpoints(t, coords, elem, curves=curves)
        return np.asarray(ext['coord_ext'], dtype=np.float64), np.asarray(ext['elem_ext'], dtype=np.int64)
    if t is not LagrangeElementType.P1:
        raise ValueError('the CSV mesh holds triangles: element_type must be P1, P2 or P4')
    return coords.astype(np.float64), elem.astype(np.int64)


def dump_free_dof_csv(directory, Q, K=None, F0=None, F=None):
    """Writes k_tangent_qq.csv (K[Q][:, Q] dense), f0q.csv (F0[Q]) and fq.csv (F[Q]) — the formats of the files the
    reference ships in tsx-tunnel/ — for whichever of K (sparse, DOF order), F0, F ((2, n_n) or DOF order) is given.
    `Q` is the (2, n_n) boolean mask of free DOFs (TSX:1695-1699)."""
    os.makedirs(directory, exist_ok=True)
    qf = np.asarray(Q, dtype=bool).flatten(order='F')
    if K is not None:
        np.savetxt(os.path.join(directory, 'k_tangent_qq.csv'), K.tocsr()[qf][:, qf].toarray(), delimiter=',')
    for name, v in (('f0q.csv', F0), ('fq.csv', F)):
        if v is not None:
            v = np.asarray(v, dtype=float)
            v = v.flatten(order='F') if v.ndim == 2 else v
            np.savetxt(os.path.join(directory, name), v[qf], delimiter=',')

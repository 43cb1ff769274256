"""
State transfer across refinement: nodal fields (the displacement) and per-integration-point fields (plastic strain,
materials, initial-strain fields) from the parents to the children of refine_marked / refine_uniform, for P1, P2 and P4
triangles.  The NumPy twin of the kernels behind fep_transfer_nodes_* and fep_transfer_points_* (include/fep.h, "state
transfer across refinement") and the wrappers that run them.  The twin performs the operations of the header in the order
written there, one IEEE double operation each, so its arrays equal the kernels' byte for byte (but for the sign bit of a NaN);
it needs neither the library nor a GPU.

  transfer_tables      per element type: the shapes, the weights W and the nearest-point table (tables.py)
  uniform_corners      corner codes and parents of refine_uniform's children (those of refine_marked: child_corners)
  transfer_nodes_np    u (n_n_parent, n_comp) -> (n_n_child, n_comp) through the parent's basis; old vertices keep their values
  transfer_points_np   q (n_rows, n_e n_q) -> (n_rows, n_child n_q): a bitwise copy of the nearest parent point
  transfer_nodes / transfer_points            the twin (device=None) or the *_host entry points
  transfer_nodes_dev / transfer_points_dev    torch tensors on the current stream; nothing is read back or synchronised
"""
import ctypes as C

import numpy as np

from .tables import ELEMENT_SHAPE, UNIFORM_CORNERS, LagrangeElementType, _coerce, transfer_tables

_FEP_TYPE = {LagrangeElementType.P1: 1, LagrangeElementType.P2: 2, LagrangeElementType.P4: 5}
_TABLES = {}                                        # element type -> transfer_tables
_DEV_TABLES = {}                                    # (device, element type) -> the tables as tensors of that GPU


def _tri(elem_type):
    t = _coerce(elem_type)
    if t not in _FEP_TYPE:
        raise ValueError(f'state transfer covers P1, P2 and P4 triangles, not {t}')
    return t


def _tables(t):
    if t not in _TABLES:
        _TABLES[t] = transfer_tables(t)
    return _TABLES[t]


def uniform_corners(n_e, device=None):
    """(corners (3, 4 n_e) uint8, parent (4 n_e)) of refine_uniform's children: 4 i .. 4 i + 3 are (0, 3, 5), (3, 1, 4),
    (5, 4, 2), (3, 4, 5) and parent = child // 4 — a constant table, no kernel.  NumPy arrays (parent int64), or — `device`,
    a GPU index — torch tensors of that GPU (parent int32, what the *_dev forms take)."""
    n_e = int(n_e)
    if device is None:
        return (np.ascontiguousarray(np.tile(np.array(UNIFORM_CORNERS, dtype=np.uint8).T, (1, n_e))),
                np.arange(4 * n_e, dtype=np.int64) // 4)
    import torch
    dev = torch.device('cuda', int(device))
    table = torch.tensor(UNIFORM_CORNERS, dtype=torch.uint8, device=dev).t()
    return table.repeat(1, n_e).contiguous(), torch.arange(4 * n_e, dtype=torch.int32, device=dev) // 4


def _child_shapes(tab, parent, corners, n_e):
    """(shape index per child, -1 for a child with a parent outside [0, n_e), a code above 5 or a triple that is no shape;
    parent with the bad ones set to 0)."""
    parent = np.asarray(parent).astype(np.int64).ravel()
    c = np.asarray(corners).astype(np.int64)
    if c.shape != (3, parent.size):
        raise ValueError(f'corners: (3, n_child) = (3, {parent.size}), got {c.shape}')
    ok = (parent >= 0) & (parent < n_e) & (c >= 0).all(axis=0) & (c <= 5).all(axis=0)
    code = np.where(ok, c[0] + 6 * c[1] + 36 * c[2], 0)
    s = np.where(ok, tab['shape_of_code'][code].astype(np.int64), -1)
    return s, np.where(s >= 0, parent, 0)


def transfer_nodes_np(elem_type, elem_parent, elem_child, parent, corners, u, n_n_child=None):
    """The nodal rule of include/fep.h on host arrays.  `elem_parent` (n_p, n_e), `elem_child` (n_p, n_child) 0-based,
    `parent` (n_child), `corners` (3, n_child), `u` (n_n_parent, n_comp) or (n_n_parent,) -> (n_n_child, n_comp) or
    (n_n_child,).  For child ch of parent e and shape s, local node j:  acc = 0.0, then acc = acc + W[s, j, a] * u[elem_parent[a, e]]
    for a = 0 .. n_p - 1.  A child node is written once, by the lowest (child element, local node) pair that holds it; a node
    of no child element gets NaN; a bad child (_child_shapes, or a parent element naming a node outside u) gives NaN to the
    nodes it owns.  An old vertex keeps its value (-0.0 becomes +0.0)."""
    t = _tri(elem_type)
    tab = _tables(t)
    n_p = ELEMENT_SHAPE[t][0]
    elem_parent = np.asarray(elem_parent).astype(np.int64).reshape(n_p, -1)
    elem_child = np.asarray(elem_child).astype(np.int64).reshape(n_p, -1)
    u_in = np.asarray(u, dtype=np.float64)
    u2 = u_in.reshape(u_in.shape[0], -1)
    n_e, n_child, n_n_parent, n_comp = elem_parent.shape[1], elem_child.shape[1], u2.shape[0], u2.shape[1]
    if n_n_child is None:
        n_n_child = int(elem_child.max()) + 1 if elem_child.size else 0
    n_n_child = int(n_n_child)
    s, e = _child_shapes(tab, parent, corners, n_e)
    if s.size != n_child:
        raise ValueError(f'parent: one entry per child ({n_child},), got {s.size}')
    bad = s < 0
    nodes_of = elem_parent[:, e] if n_e else np.zeros((n_p, n_child), dtype=np.int64)     # (n_p, n_child)
    bad = bad | ((nodes_of < 0) | (nodes_of >= n_n_parent)).any(axis=0)
    nodes_of = np.where(bad[None, :], 0, nodes_of)
    W, shape = tab['W'], np.where(bad, 0, s)
    ch = np.arange(n_child, dtype=np.int64)
    no_owner = np.iinfo(np.int64).max
    owner = np.full(n_n_child, no_owner, dtype=np.int64)
    held = (elem_child >= 0) & (elem_child < n_n_child)
    for j in range(n_p):
        np.minimum.at(owner, elem_child[j][held[j]], (ch * n_p + j)[held[j]])
    out = np.full((n_n_child, n_comp), np.nan)
    with np.errstate(all='ignore'):
        for j in range(n_p):
            acc = np.zeros((n_child, n_comp))
            if n_n_parent:
                for a in range(n_p):
                    acc = acc + W[shape, j, a][:, None] * u2[nodes_of[a]]
            acc[bad] = np.nan
            mine = np.flatnonzero(held[j])
            mine = mine[owner[elem_child[j, mine]] == mine * n_p + j]
            out[elem_child[j, mine]] = acc[mine]
    return out if u_in.ndim > 1 else out[:, 0]


def transfer_points_np(elem_type, parent, corners, q, n_e=None):
    """The point rule of include/fep.h on host arrays: `q` (n_rows, n_e n_q) or (n_e n_q,) -> (n_rows, n_child n_q) or
    (n_child n_q,), out[:, ch n_q + k] = q[:, e n_q + near[s, k]], a copy (any dtype goes through unchanged); a bad child
    (_child_shapes) gets NaN in all its points."""
    t = _tri(elem_type)
    tab = _tables(t)
    n_q = ELEMENT_SHAPE[t][1]
    q_in = np.asarray(q)
    q2 = q_in.reshape(1, -1) if q_in.ndim == 1 else q_in
    n_e = q2.shape[1] // n_q if n_e is None else int(n_e)
    if q2.shape[1] != n_e * n_q:
        raise ValueError(f'point field: (n_rows, n_e n_q) with n_q = {n_q}, got {q2.shape}')
    s, e = _child_shapes(tab, parent, corners, n_e)
    src = e[:, None] * n_q + tab['near'][np.where(s < 0, 0, s)].astype(np.int64)          # (n_child, n_q)
    if n_e == 0:
        out = np.full((q2.shape[0], src.size), np.nan, dtype=np.float64)
    else:
        out = np.array(q2[:, src.ravel()])
        if (s < 0).any():
            out = out.astype(np.float64) if out.dtype.kind != 'f' else out
            out[:, np.repeat(s < 0, n_q)] = np.nan
    return out[0] if q_in.ndim == 1 else out


def _i32(a):
    a = np.asarray(a)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        from . import _lib
        raise _lib.FepError(-5, 'state transfer')
    return np.ascontiguousarray(a, dtype=np.int32)


def transfer_nodes(elem_type, elem_parent, elem_child, parent, corners, u, n_n_child=None, device=None):
    """transfer_nodes_np (device=None), or — `device`, a GPU index — the same arrays from fep_transfer_nodes_host."""
    if device is None:
        return transfer_nodes_np(elem_type, elem_parent, elem_child, parent, corners, u, n_n_child=n_n_child)
    from . import _lib
    t = _tri(elem_type)
    tab = _tables(t)
    n_p = ELEMENT_SHAPE[t][0]
    ep, ec = _i32(np.asarray(elem_parent).reshape(n_p, -1)), _i32(np.asarray(elem_child).reshape(n_p, -1))
    par, cor = _i32(np.asarray(parent).ravel()), np.ascontiguousarray(corners, dtype=np.uint8)
    u_in = np.asarray(u, dtype=np.float64)
    u2 = np.ascontiguousarray(u_in.reshape(u_in.shape[0], -1))
    if n_n_child is None:
        n_n_child = int(ec.max()) + 1 if ec.size else 0
    if cor.shape != (3, ec.shape[1]) or par.shape != (ec.shape[1],):
        raise ValueError(f'parent (n_child,) and corners (3, n_child) with n_child = {ec.shape[1]}, got {par.shape} and {cor.shape}')
    if not 1 <= u2.shape[1] <= 4:
        raise ValueError(f'nodal fields have 1 to 4 components, got {u2.shape[1]}')
    out = np.empty((int(n_n_child), u2.shape[1]))
    ptr = _lib.ptr
    _lib.check(_lib.lib().fep_transfer_nodes_host(int(device), _FEP_TYPE[t], u2.shape[1], ep.shape[1], u2.shape[0], ec.shape[1],
                                                  int(n_n_child), ptr(ep), ptr(ec), ptr(par), ptr(cor), ptr(tab['shape_of_code']),
                                                  ptr(tab['W']), ptr(u2), ptr(out)), 'fep_transfer_nodes_host')
    return out if u_in.ndim > 1 else out[:, 0]


def transfer_points(elem_type, parent, corners, q, device=None):
    """transfer_points_np (device=None), or — `device`, a GPU index — the same arrays from fep_transfer_points_host
    (float64 fields)."""
    if device is None:
        return transfer_points_np(elem_type, parent, corners, q)
    from . import _lib
    t = _tri(elem_type)
    tab = _tables(t)
    n_q = ELEMENT_SHAPE[t][1]
    q_in = np.asarray(q, dtype=np.float64)
    q2 = np.ascontiguousarray(q_in.reshape(1, -1) if q_in.ndim == 1 else q_in)
    par, cor = _i32(np.asarray(parent).ravel()), np.ascontiguousarray(corners, dtype=np.uint8)
    if q2.shape[1] % n_q or cor.shape != (3, par.size):
        raise ValueError(f'point field (n_rows, n_e n_q) with n_q = {n_q} and corners (3, n_child), got {q2.shape} and {cor.shape}')
    out = np.empty((q2.shape[0], par.size * n_q))
    ptr = _lib.ptr
    _lib.check(_lib.lib().fep_transfer_points_host(int(device), _FEP_TYPE[t], q2.shape[0], q2.shape[1] // n_q, par.size, ptr(par),
                                                   ptr(cor), ptr(tab['shape_of_code']), ptr(tab['near']), ptr(q2), ptr(out)),
               'fep_transfer_points_host')
    return out[0] if q_in.ndim == 1 else out


def _dev_tables(t, device):
    """The tables of `t` on GPU `device`: uploaded once per (device, element type) and kept."""
    import torch
    key = (int(device), t)
    if key not in _DEV_TABLES:
        dev = torch.device('cuda', int(device))
        _DEV_TABLES[key] = {k: torch.from_numpy(v).to(dev) for k, v in _tables(t).items()}
    return _DEV_TABLES[key]


def _check_dev(name, a, dtype, shape):
    if a.dtype != dtype or tuple(a.shape) != tuple(shape) or not a.is_contiguous() or not a.is_cuda:
        raise ValueError(f'{name}: a contiguous {dtype} tensor of {tuple(shape)} on the GPU, got {a.dtype} {tuple(a.shape)}')


def transfer_nodes_dev(elem_type, elem_parent, elem_child, parent, corners, u, n_n_child, out=None):
    """fep_transfer_nodes_dev on torch tensors of one GPU, on its current stream: `elem_parent` (n_p, n_e), `elem_child`
    (n_p, n_child), `parent` (n_child) int32, `corners` (3, n_child) uint8, `u` (n_n_parent, n_comp) or (n_n_parent n_comp,)
    with n_comp = 2 (the drivers' interleaved U) float64 -> `out` or a new tensor of u's form for n_n_child nodes."""
    import torch
    from . import _lib
    t = _tri(elem_type)
    n_p = ELEMENT_SHAPE[t][0]
    device = u.device.index
    tab = _dev_tables(t, device)
    n_e, n_child, n_n_child = int(elem_parent.shape[1]), int(elem_child.shape[1]), int(n_n_child)
    n_comp = 2 if u.dim() == 1 else int(u.shape[1])
    n_n_parent = int(u.shape[0]) // n_comp if u.dim() == 1 else int(u.shape[0])
    _check_dev('elem_parent', elem_parent, torch.int32, (n_p, n_e))
    _check_dev('elem_child', elem_child, torch.int32, (n_p, n_child))
    _check_dev('parent', parent, torch.int32, (n_child,))
    _check_dev('corners', corners, torch.uint8, (3, n_child))
    _check_dev('u', u, torch.float64, u.shape)
    shape = (n_n_child * n_comp,) if u.dim() == 1 else (n_n_child, n_comp)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=u.device)
    _check_dev('out', out, torch.float64, shape)
    p = lambda a: C.c_void_p(a.data_ptr())                                          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(_lib.lib().fep_transfer_nodes_dev(device, stream, _FEP_TYPE[t], n_comp, n_e, n_n_parent, n_child, n_n_child,
                                                 p(elem_parent), p(elem_child), p(parent), p(corners), p(tab['shape_of_code']),
                                                 p(tab['W']), p(u), p(out)), 'fep_transfer_nodes_dev')
    return out


def transfer_points_dev(elem_type, parent, corners, q, out=None):
    """fep_transfer_points_dev on torch tensors of one GPU, on its current stream: `parent` (n_child) int32, `corners`
    (3, n_child) uint8, `q` (n_rows, n_e n_q) or (n_e n_q,) float64 -> `out` or a new tensor (n_rows, n_child n_q) or
    (n_child n_q,)."""
    import torch
    from . import _lib
    t = _tri(elem_type)
    n_q = ELEMENT_SHAPE[t][1]
    device = q.device.index
    tab = _dev_tables(t, device)
    n_child = int(parent.shape[0])
    n_rows = 1 if q.dim() == 1 else int(q.shape[0])
    n_int = int(q.shape[-1])
    if n_int % n_q:
        raise ValueError(f'point field: n_e n_q columns with n_q = {n_q}, got {n_int}')
    _check_dev('parent', parent, torch.int32, (n_child,))
    _check_dev('corners', corners, torch.uint8, (3, n_child))
    _check_dev('q', q, torch.float64, q.shape)
    shape = (n_child * n_q,) if q.dim() == 1 else (n_rows, n_child * n_q)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=q.device)
    _check_dev('out', out, torch.float64, shape)
    p = lambda a: C.c_void_p(a.data_ptr())                                          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(_lib.lib().fep_transfer_points_dev(device, stream, _FEP_TYPE[t], n_rows, n_int // n_q, n_child, p(parent), p(corners),
                                                  p(tab['shape_of_code']), p(tab['near']), p(q), p(out)), 'fep_transfer_points_dev')
    return out

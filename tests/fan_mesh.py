"""
Meshes with one node of high degree, for the tests of the node-degree limits (test_high_degree_gpu.py,
test_host_sanitizers.py, test_parity_gpu.py's patch-vs-COO cases).

fan_mesh(k): a closed fan of k triangles around a centre node (id 0) on a rim of k nodes at radius 1, plus an outer ring
of 2k triangles to k nodes at radius 2, so that the rim nodes are ordinary (5 elements each) and only the centre is not.
The centre's CSR row holds k + 1 node-pair blocks for P1, 3k + 1 for P2 and 10k + 1 for P4 (midpoints from
create_midpoints_P2 / create_midpoints_P4, the reference's numbering).  Every triangle is counter-clockwise.

Limits these meshes sit at (fem-elastoplasticity_amd/csrc/fep_host.h):
  P1 k = 15 / 16     a block of the node route's packed descriptor counts up to 15 contributions: the centre's diagonal
                     block has k, so k >= 16 takes the element route
  P1 k = 255 / 256   row_tiles: at most 256 blocks per node row (FEP_ERANGE above)
  P2 k = 85 / 86     the same limit (3k + 1 = 256 / 259)
  P4 k = 25 / 26     the same limit (251 / 261)
"""
from importlib import import_module

import numpy as np


def fan_p1(k, jitter=0.1, seed=0):
    """(elements (3, 3k) int64, coordinates (2, 2k + 1)): the P1 fan of k triangles with its outer ring.  `jitter`: the
    rim and ring nodes move by up to that fraction of the angular step along the circle and of the ring spacing radially."""
    rng = np.random.default_rng(seed)
    h = 2 * np.pi / k
    t_rim = h * np.arange(k) + jitter * h * rng.uniform(-0.5, 0.5, k)
    t_out = h * (np.arange(k) + 0.5) + jitter * h * rng.uniform(-0.5, 0.5, k)
    r_rim = 1 + jitter * rng.uniform(-0.2, 0.2, k)
    r_out = 2 + jitter * rng.uniform(-0.2, 0.2, k)
    coord = np.concatenate([[[0.0], [0.0]], [r_rim * np.cos(t_rim), r_rim * np.sin(t_rim)],
                            [r_out * np.cos(t_out), r_out * np.sin(t_out)]], axis=1)
    i = np.arange(k)
    rim, rim1 = 1 + i, 1 + (i + 1) % k
    out, out1 = 1 + k + i, 1 + k + (i + 1) % k
    elem = np.concatenate([np.stack([np.zeros(k, dtype=np.int64), rim, rim1]),      # the fan
                           np.stack([rim, out, rim1]), np.stack([rim1, out, out1])], axis=1)
    x, y = coord[:, elem]
    area2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    assert (area2 > 0).all(), 'jitter too large: a triangle turned over'
    return elem, coord


def fan_mesh(k, t='P1', jitter=0.1, shuffle=False, seed=0):
    """(elements (n_p, n_e), coordinates (2, n_n)) of the fan of k triangles as element type t (P1, P2, P4).  shuffle:
    random node and element numbering (the centre is then not node 0; `centre_of` finds it)."""
    elem, coord = fan_p1(k, jitter, seed)
    if t == 'P2' or t == 'P4':
        from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
        mp = import_module('fem-elastoplasticity_amd').midpoints
        m = (mp.create_midpoints_P2 if t == 'P2' else mp.create_midpoints_P4)(coord, elem)
        elem, coord = m['elem_ext'], m['coord_ext']
    elif t != 'P1':
        raise ValueError(t)
    if shuffle:
        rng = np.random.default_rng(seed + 1)
        perm = rng.permutation(coord.shape[1])                  # new id of old node n: inv[n]
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        elem, coord = inv[elem][:, rng.permutation(elem.shape[1])], coord[:, perm]
    return np.ascontiguousarray(elem, dtype=np.int64), np.ascontiguousarray(coord)


def centre_of(elem):
    """The node in the most elements (the fan's centre)."""
    return int(np.bincount(elem[:3].ravel()).argmax())


def row_blocks(elem, node):
    """Node-pair blocks in `node`'s CSR row: the distinct nodes of its elements (itself included)."""
    return int(np.unique(elem[:, (elem == node).any(axis=0)]).size)

"""
The Elasticity2D flavour end to end (EL:1052-1179): the square with a corner cut-out under self-weight and a traction
on its top side, one linear solve.  Mesh, elastic K (the hot path at U = 0), both load vectors (fep_load_volume_*,
fep_load_traction_*), lifting of the prescribed displacement, solve on the free DOFs, stored energy.
"""
from contextlib import closing

import numpy as np

from .hotpath import MeshContext, load_traction
from .mesh import assemble_mesh_el
from .newton import make_ops
from .tables import LagrangeElementType, _coerce, element_tables, surface_tables


def solve_elasticity2d(element_type='P1', level=1, linear_solver='amg', volume_force=(0, -1), traction_force=(0, 450),
                       young=206900, poisson=0.29, size_xy=10, size_hole=5, device=None, pcg_rtol=1e-13, log=None):
    """Drop-in for the driver `elasticity_fem` (EL:1052-1179) with its constants as arguments.  Returns a dict with
    'U' (2, n_n), 'energy' = 0.5 u.K u - (f_t + f_V).u (what the reference prints as "Stored energy"), 'f_V', 'f_t'
    (2, n_n), 'K' (csr on the full pattern), 'iterations' (CG iterations, None for 'direct') and 'mesh'.

    `linear_solver`: 'direct' (SciPy sparse LU on the host, as in solve_strip_footing), 'pcg' (block-Jacobi CG) or
    'amg' (multigrid CG), both entirely on the device: K u_d, the load vectors, the right-hand side and the energy are
    device vectors (fep_solver_spmv_dev) until the final copy.  `volume_force` is applied as a uniform field (no
    per-point array); `traction_force` on every edge of the top side ('neumann_nodes')."""
    t = _coerce(element_type)
    mesh = assemble_mesh_el(level, t, size_xy, size_hole)                                 # EL:1094
    elem = mesh['elements'] - 1                                                           # EL:389
    coord, Q = mesh['coordinates'], mesh['Q']
    d1, d2, wf = element_tables(t)
    ctx = MeshContext(elem, coord, d1, d2, wf, device=device)
    ctx.set_materials(young / (2 * (1 + poisson)), young / (3 * (1 - 2 * poisson)), 1.0, 1.0)
    with closing(ctx), closing(make_ops(ctx, Q.flatten(order='F'), linear_solver, pcg_rtol)) as ops:
        K = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']                          # EL:1118 (elastic at U = 0)
        ops.setup_amg(K, coord)                                                           # linear_solver='amg' only
        # load vectors (EL:1126-1138)
        edges = mesh['neumann_nodes'].astype(np.int64)
        hatp_s, dhatp1_s, wf_s = surface_tables(t)
        t_int = np.repeat(np.asarray(traction_force, dtype=float).reshape(2, 1), edges.shape[1] * wf_s.size, axis=1)
        f_t2 = load_traction(edges, coord, t_int, hatp_s, dhatp1_s, wf_s, device=ctx.device)
        f_t = ops.vec(f_t2.flatten(order='F'))
        f_V = ops.load_volume(volume_force)
        f_ext = f_t + f_V
        ud = ops.vec((0.5 * mesh['dirichlet_nodes']).flatten(order='F'))                  # EL:1140
        u = ud + ops.solve(K, f_ext - ops.matvec(K, ud))                                  # EL:1146-1160
        energy = 0.5 * float(u @ ops.matvec(K, u)) - float(f_ext @ u)                     # EL:1172
        out = {'U': ops.host(u).reshape((2, -1), order='F').copy(), 'energy': energy,
               'f_V': ops.host(f_V).reshape((2, -1), order='F').copy(), 'f_t': f_t2, 'K': ops.csr(K),
               'iterations': None if not ops.pcg_iters else int(ops.pcg_iters[-1]), 'mesh': mesh}
    if log:
        log(f'Stored energy: {energy!r}')
    return out


def elasticity_fem(element_type=LagrangeElementType.P1, level=1, draw=True, linear_solver='amg', device=None):
    """The reference's signature (EL:1052-1054); `draw` is ignored (no plotting here).  Prints the stored energy as the
    reference does and, unlike it, returns the result of `solve_elasticity2d`."""
    res = solve_elasticity2d(element_type, level, linear_solver=linear_solver, device=device)
    print(f'Stored energy: {res["energy"]}')
    return res

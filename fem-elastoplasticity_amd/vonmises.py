"""
The second material model end to end (no counterpart in the reference): von Mises plasticity with linear kinematic
hardening on the Elasticity2D flavour's cut-out square, loaded through a traction on its top side that runs a
load - unload - reverse cycle.  With hardening the yield surface travels with the plastic strain (back stress a * p),
so yielding in the reverse direction starts early: the Bauschinger effect, and a closed load cycle dissipates work.
"""
from contextlib import closing

import numpy as np

from .hotpath import load_traction
from .mesh import assemble_mesh_el
from .newton import _context_maker, _load_history_loop, make_ops
from .tables import _coerce, element_tables, surface_tables


def cycle_factors(steps_per_quarter):
    """Load factors 0 -> 1 -> -1 -> 0 in 4 * steps_per_quarter equal steps (the starting 0 is not a step)."""
    n = int(steps_per_quarter)
    up = np.arange(1, n + 1) / n
    return np.concatenate([up, 1 - np.arange(1, 2 * n + 1) / n, -1 + up])


def solve_cutout_cyclic(element_type='P1', level=1, peak_traction=(0, 200), steps_per_quarter=4, young=206900, poisson=0.29,
                        sigma_y=450, hardening=10000, linear_solver='amg', f_ext=None, zetas=None, context_factory=None,
                        device=None, pcg_rtol=1e-11, log=None, plane_stress=False):
    """A load cycle on the cut-out square (mesh.assemble_mesh_el: P1, Q1, Q2).  The DOFs outside the mesh's 'Q' are held
    at zero; the external load is `f_ext` (2, n_n) when given, else the traction `peak_traction` on the top side
    (load_traction), times the load factors `zetas` (default: cycle_factors(steps_per_quarter)).  Materials: shear and
    bulk from `young` / `poisson`, yield radius Y = sqrt(2/3) * `sigma_y`, and `hardening` is the modulus a of the back
    stress a * p.  Per load factor a Newton iteration from the last accepted state (newton._load_history_loop: at most 25
    iterates, converged below 1e-10, no sub-stepping), then the accepting call that updates the plastic strain.
    `plane_stress=True` runs the plate in plane stress (the 'vmps' model: s33 = 0, the thickness strain free) instead of
    the default plane strain ('vm': a thick prism).

    Returns a dict: 'zeta' (the accepted factors), 'U' (list of (2, n_n)), 'n_plast', 'newton_its', 'pcg_iters', 'Ep',
    'f_ext' (2, n_n), 'mesh', 'failed_at' (index of the step that did not converge, or None) and 'work' =
    sum_k (zeta_k + zeta_{k-1})/2 * f_ext . (U_k - U_{k-1}), the work of the external load over the accepted steps.
    `context_factory(elements, coordinates, dhatp1, dhatp2, wf)` may supply another object with MeshContext's
    `set_model / set_materials / step / geometry / close` (the tests run the loop on their CPU restatement that way)."""
    t = _coerce(element_type)
    mesh = assemble_mesh_el(level, t)
    elem = mesh['elements'] - 1
    coord, Q = mesh['coordinates'], mesh['Q']
    ctx = _context_maker(context_factory, device)(elem, coord, *element_tables(t))
    ctx.set_model('vmps' if plane_stress else 'vm')
    ctx.set_materials(young / (2 * (1 + poisson)), young / (3 * (1 - 2 * poisson)), float(hardening),
                      np.sqrt(2 / 3) * sigma_y)
    if f_ext is None:
        edges = mesh['neumann_nodes'].astype(np.int64)
        hatp_s, dhatp1_s, wf_s = surface_tables(t)
        t_int = np.repeat(np.asarray(peak_traction, dtype=float).reshape(2, 1), edges.shape[1] * wf_s.size, axis=1)
        f_ext = load_traction(edges, coord, t_int, hatp_s, dhatp1_s, wf_s, device=getattr(ctx, 'device', device))
    f_ext = np.array(f_ext, dtype=np.float64).reshape(2, -1)
    zetas = cycle_factors(steps_per_quarter) if zetas is None else np.asarray(zetas, dtype=float).ravel()
    hist = {'zeta': [], 'U': [], 'n_plast': [], 'newton_its': [], 'n_calls': 0}
    with closing(ctx), closing(make_ops(ctx, Q.flatten(order='F'), linear_solver, pcg_rtol)) as ops:
        K_elast = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']                    # elastic at U = 0: crit = -Y
        ops.setup_amg(K_elast, coord)                                                     # linear_solver='amg' only

        def accepted(r, zeta, U, its):
            hist['U'].append(ops.host(U).reshape((2, -1), order='F').copy())
            hist['n_plast'].append(int(r['n_smooth']))
            hist['newton_its'].append(its)
            if log:
                log(f'zeta={zeta:.6g} its={its} n_plast={hist["n_plast"][-1]} max|U|={np.abs(hist["U"][-1]).max():.10g}')

        _, Ep = _load_history_loop(ops, K_elast, ops.vec(f_ext.flatten(order='F')), zetas, hist, accepted=accepted)
        hist['Ep'] = np.array(ops.host(Ep))
        hist['pcg_iters'] = ops.pcg_iters
    work, z_old, U_old = 0.0, 0.0, np.zeros_like(f_ext)
    for z, U in zip(hist['zeta'], hist['U']):
        work += 0.5 * (z + z_old) * float(np.sum(f_ext * (U - U_old)))
        z_old, U_old = z, U
    hist.update(work=work, f_ext=f_ext, mesh=mesh)
    return hist

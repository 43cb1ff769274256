"""
The second material model end to end (no counterpart in the reference): von Mises plasticity with linear kinematic
hardening on the Elasticity2D flavour's cut-out square, loaded through a traction on its top side that runs a
load - unload - reverse cycle.  With hardening the yield surface travels with the plastic strain (back stress a * p),
so yielding in the reverse direction starts early: the Bauschinger effect, and a closed load cycle dissipates work.
"""
from contextlib import closing

import numpy as np

from .hardening import check_curve, hardening_curve
from .hotpath import load_traction
from .mesh import assemble_mesh_el
from .newton import _context_maker, _load_history_loop, make_ops
from .tables import LagrangeElementType, _coerce, element_tables, surface_tables


def cycle_factors(steps_per_quarter):
    """Load factors 0 -> 1 -> -1 -> 0 in 4 * steps_per_quarter equal steps (the starting 0 is not a step)."""
    n = int(steps_per_quarter)
    up = np.arange(1, n + 1) / n
    return np.concatenate([up, 1 - np.arange(1, 2 * n + 1) / n, -1 + up])


def solve_cutout_cyclic(element_type='P1', level=1, peak_traction=(0, 200), steps_per_quarter=4, young=206900, poisson=0.29,
                        sigma_y=450, hardening=10000, linear_solver='amg', f_ext=None, zetas=None, context_factory=None,
                        device=None, pcg_rtol=1e-11, log=None, plane_stress=False, adapt_at=None, mark='zz', theta=0.5,
                        isotropic=None):
    """A load cycle on the cut-out square (mesh.assemble_mesh_el: P1, Q1, Q2).  The DOFs outside the mesh's 'Q' are held
    at zero; the external load is `f_ext` (2, n_n) when given, else the traction `peak_traction` on the top side
    (load_traction), times the load factors `zetas` (default: cycle_factors(steps_per_quarter)).  Materials: shear and
    bulk from `young` / `poisson`, yield radius Y = sqrt(2/3) * `sigma_y`, and `hardening` is the modulus a of the back
    stress a * p.  Per load factor a Newton iteration from the last accepted state (newton._load_history_loop: at most 25
    iterates, converged below 1e-10, no sub-stepping), then the accepting call that updates the plastic strain.
    `plane_stress=True` runs the plate in plane stress (the 'vmps' model: s33 = 0, the thickness strain free) instead of
    the default plane strain ('vm': a thick prism).
    `isotropic` adds isotropic hardening (the 'vmi' model, plane strain only: ValueError with `plane_stress`), `hardening`
    staying the kinematic modulus a: a number is a linear modulus d sigma_y / d eps_p_bar, a pair of arrays (eps_p_bar, sigma_y)
    a uniaxial table (hardening.hardening_curve; its first stress is then the initial yield stress and `sigma_y` is not
    used).  The yield surface grows with the accumulated plastic flow, so reverse yielding comes later than with the same
    modulus put into the back stress: cyclic hardening instead of the Bauschinger effect.  Row 3 of 'Ep' is then the
    accumulated multiplier, returned as 'kappa' too, with 'eps_p_bar' = sqrt(2/3) kappa.

    Returns a dict: 'zeta' (the accepted factors), 'U' (list of (2, n_n)), 'n_plast', 'newton_its', 'pcg_iters', 'Ep',
    'f_ext' (2, n_n), 'mesh', 'failed_at' (index of the step that did not converge, or None), 'retries' (indices of the steps
    that took the second attempt, the one that starts with an elastic correction) and 'work' =
    sum_k (zeta_k + zeta_{k-1})/2 * f_ext . (U_k - U_{k-1}), the work of the external load over the accepted steps.
    `context_factory(elements, coordinates, dhatp1, dhatp2, wf)` may supply another object with MeshContext's
    `set_model / set_materials / step / geometry / close` (the tests run the loop on their CPU restatement that way).

    `adapt_at` (P1 only; no `f_ext`): a sequence of indices into the load factors.  After the accepted step k in it the mesh is
    refined in the middle of the history and the state goes along (transfer.py; DESIGN.md section 4, "State transfer across
    refinement"): the marks come from `mark` — 'zz', the recovered-stress indicator of that step's stress with bulk marking of
    the fraction `theta`, or a callable (hist, coord, elem) -> bool (n_e) — then refine_marked with the corner codes,
    transfer_nodes on U and transfer_points on the plastic strain, a new context (same model and materials), new ops and,
    with 'amg', a new hierarchy; Q by assemble_mesh_el's rule on the new coordinates, the top-side edges from the child mesh,
    the traction on them, and the history goes on from the transferred state: first the factor of step k once more, an
    accepted step of its own that lets the new mesh come to equilibrium at that load ('zeta' and the per-step lists hold one
    entry more per refinement, at the index the row's 'equilibration' names; a failure there reports 'failed_at' = k), then
    the remaining factors.  With device vectors ('pcg', 'amg') indicator,
    marking, refinement and both transfers stay on the GPU: only the counts of the marking come back before the new mesh is
    read to build its context.  The result then also holds 'adapt': per refinement {'step', 'n_e', 'n_n', 'n_marked',
    'n_child', 'eta' (sqrt of the indicator's total; None for a callable), 'parent', 'corners', 'coords', 'elem' (the child
    mesh), 's' (the step's stress on the parent), 'U', 'Ep' (the transferred state)}; every 'U' has the size of the mesh it was
    accepted on, 'work' is summed per segment with that segment's 'f_ext' from the transferred U on, and 'mesh', 'f_ext' are
    the last mesh's.  Without `adapt_at` the run is what it was, bit for bit."""
    t = _coerce(element_type)
    shear, bulk = young / (2 * (1 + poisson)), young / (3 * (1 - 2 * poisson))
    model, Y, curve = 'vmps' if plane_stress else 'vm', np.sqrt(2 / 3) * sigma_y, None
    if isotropic is not None:
        if plane_stress:
            raise ValueError('isotropic hardening runs in plane strain only (the plane-stress model has no hardening curve)')
        if np.ndim(isotropic) == 0:                        # R = sqrt(2/3) h eps_p_bar = (2/3) h kappa
            curve = (np.zeros(1), np.array([2 * float(isotropic) / 3]))
        else:
            Y, *curve = hardening_curve(*isotropic)
        model, curve = 'vmi', check_curve(*curve, shear=shear, a=float(hardening), Y=Y)
    if adapt_at is not None:
        if t is not LagrangeElementType.P1:
            raise ValueError(f'adapt_at refines P1 meshes only (marked refinement has no {t.name} form)')
        if f_ext is not None:
            raise ValueError('adapt_at computes the traction again on every mesh: pass peak_traction, not f_ext')
        zetas = cycle_factors(steps_per_quarter) if zetas is None else np.asarray(zetas, dtype=float).ravel()
        return _with_kappa(_cutout_adaptive(assemble_mesh_el(level, t), zetas, adapt_at, mark, theta, peak_traction,
                                            (model, (shear, bulk, float(hardening), Y), curve),
                                            linear_solver, context_factory, device, pcg_rtol, log), curve)
    mesh = assemble_mesh_el(level, t)
    elem = mesh['elements'] - 1
    coord, Q = mesh['coordinates'], mesh['Q']
    ctx = _context_maker(context_factory, device)(elem, coord, *element_tables(t))
    ctx.set_model(model)
    ctx.set_materials(shear, bulk, float(hardening), Y)
    if curve is not None:
        ctx.set_hardening(*curve)
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
    return _with_kappa(hist, curve)


def _with_kappa(hist, curve):
    """The accumulated multiplier of a run with isotropic hardening (row 3 of the state) under its own names."""
    if curve is not None and 'Ep' in hist:
        hist['kappa'] = hist['Ep'][3].copy()
        hist['eps_p_bar'] = np.sqrt(2 / 3) * hist['kappa']
    return hist


# ---------------------------------------------------------------------------------------
# refinement in the middle of the load history (solve_cutout_cyclic, adapt_at)
# ---------------------------------------------------------------------------------------
def _top_edges(coord, elem):
    """(2, n) boundary edges of a P1 mesh with both ends on the top side y == max y, in the element's walking direction,
    ordered by x."""
    n_n = coord.shape[1]
    a, b = elem[[0, 1, 2]].ravel(), elem[[1, 2, 0]].ravel()
    top = coord[1].max()
    on = (coord[1, a] == top) & (coord[1, b] == top)
    a, b = a[on], b[on]
    _, first, count = np.unique(np.minimum(a, b) * n_n + np.maximum(a, b), return_index=True, return_counts=True)
    keep = first[count == 1]
    keep = keep[np.argsort(np.minimum(coord[0, a[keep]], coord[0, b[keep]]), kind='stable')]
    return np.array([a[keep], b[keep]], dtype=np.int64)


def _p1_traction(edges, coord, traction):
    """The uniform `traction` on straight two-node edges, summed on the host: half an edge per end node (what load_traction
    gives for P1, for a run without a GPU)."""
    d = coord[:, edges[1]] - coord[:, edges[0]]
    half = np.sqrt(d[0] * d[0] + d[1] * d[1]) / 2
    f = np.zeros(coord.shape)
    for r in range(2):
        np.add.at(f[r], edges[0], half * traction[r])
        np.add.at(f[r], edges[1], half * traction[r])
    return f


def _cutout_adaptive(mesh, zetas, adapt_at, mark, theta, peak_traction, model, linear_solver, context_factory, device, pcg_rtol, log):
    """solve_cutout_cyclic(adapt_at=...): the history in segments, one mesh, context, ops and load vector per segment, the
    state carried from one to the next by the transfer of transfer.py."""
    from .estimate import _check_theta
    from .newton import _DeviceOps
    zz = isinstance(mark, str)
    if (zz and mark != 'zz') or not (zz or callable(mark)):
        raise ValueError(f"mark: 'zz' or a callable (hist, coord, elem) -> bool (n_e), got {mark!r}")
    if zz:
        theta = _check_theta(theta)
    cuts = sorted({int(k) for k in adapt_at})
    if cuts and (cuts[0] < 0 or cuts[-1] >= len(zetas)):
        raise ValueError(f'adapt_at: indices into the {len(zetas)} load factors, got {cuts}')
    t = LagrangeElementType.P1
    tables, surf = element_tables(t), surface_tables(t)
    traction = np.asarray(peak_traction, dtype=float).reshape(2)
    coord = np.array(mesh['coordinates'], dtype=np.float64)
    elem = np.asarray(mesh['elements'] - 1).astype(np.int64)
    Q, edges = mesh['Q'], mesh['neumann_nodes'].astype(np.int64)
    dirichlet = mesh['dirichlet_nodes']
    hist = {'zeta': [], 'U': [], 'n_plast': [], 'newton_its': [], 'n_calls': 0, 'adapt': [], 'failed_at': None}
    pcg_iters, work, z_old, start, carried = None, 0.0, 0.0, 0, None
    stops = [k + 1 for k in cuts] + [len(zetas)]
    for seg, stop in enumerate(stops):
        ctx = _context_maker(context_factory, device)(elem, coord, *tables)
        ctx.set_model(model[0])
        ctx.set_materials(*model[1])
        if model[2] is not None:                            # every segment's context runs on the same hardening curve
            ctx.set_hardening(*model[2])
        if context_factory is None:
            t_int = np.repeat(traction.reshape(2, 1), edges.shape[1] * surf[2].size, axis=1)
            f_ext = load_traction(edges, coord, t_int, *surf, device=ctx.device)
        else:
            f_ext = _p1_traction(edges, coord, traction)
        with closing(ctx), closing(make_ops(ctx, Q.flatten(order='F'), linear_solver, pcg_rtol)) as ops:
            K_elast = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']
            ops.setup_amg(K_elast, coord)
            on_device = isinstance(ops, _DeviceOps)
            kept = {}

            def accepted(r, zeta, U, its):
                hist['U'].append(ops.host(U).reshape((2, -1), order='F').copy())
                hist['n_plast'].append(int(r['n_smooth']))
                hist['newton_its'].append(its)
                kept['s'] = r['s']                                                        # the ops' own array: not copied
                if log:
                    log(f'zeta={zeta:.6g} its={its} n_plast={hist["n_plast"][-1]} max|U|={np.abs(hist["U"][-1]).max():.10g}')

            U0 = Ep0 = None
            if carried is not None:
                U0, Ep0 = carried if on_device else (ops.vec(carried[0]), np.ascontiguousarray(carried[1], dtype=np.float64))
            n_before, n_retried = len(hist['zeta']), len(hist.get('retries', ()))
            # The transferred state is admissible but not in equilibrium against the new test functions.  A segment therefore
            # begins by repeating the factor it was refined at: an accepted step of its own, with the plastic flow the finer
            # mesh asks for at that load.  (Going straight on to a smaller factor leaves the Newton iteration to unload and
            # to equilibrate at once, and it then cycles between active sets.)
            seg_zetas = zetas[start:stop] if seg == 0 else np.concatenate([zetas[start - 1:start], zetas[start:stop]])
            if seg > 0:
                hist['adapt'][-1]['equilibration'] = n_before
            U, Ep = _load_history_loop(ops, K_elast, ops.vec(f_ext.flatten(order='F')), seg_zetas, hist, accepted=accepted,
                                       U=U0, Ep=Ep0, accept_want=('s', 'ind_p'))
            if ops.pcg_iters is not None:
                pcg_iters = (pcg_iters or []) + list(ops.pcg_iters)
            U_old = np.zeros_like(f_ext) if not hist['adapt'] else hist['adapt'][-1]['U']
            for z, Uk in zip(hist['zeta'][n_before:], hist['U'][n_before:]):
                work += 0.5 * (z + z_old) * float(np.sum(f_ext * (Uk - U_old)))
                z_old, U_old = z, Uk
            shift = start - (1 if seg > 0 else 0)                                         # to an index into the load factors
            hist['retries'][n_retried:] = [k + shift for k in hist['retries'][n_retried:]]
            if hist['failed_at'] is not None:
                hist['failed_at'] += shift
            if hist['failed_at'] is not None or seg == len(stops) - 1:
                hist['Ep'] = np.array(ops.host(Ep))
                break
            row, coord, elem, carried = _refine_with_state(ctx, ops, on_device, context_factory, hist, coord, elem, kept['s'], U, Ep,
                                                           mark, theta, model[1])
            row['step'] = stop - 1
            hist['adapt'].append(row)
            if log:
                log(f'adapt after step {row["step"]}: {row["n_e"]} -> {row["n_child"]} elements, {row["n_marked"]} marked')
        Q = coord > 0                                                                     # assemble_mesh_el's rule
        Q[0, coord[1, :] == 0] = 0
        dirichlet = np.zeros(coord.shape)
        dirichlet[0, coord[1, :] == 0] = 1
        edges = _top_edges(coord, elem)
        start = stop
    if hist['adapt']:
        mesh = {'coordinates': coord, 'elements': elem + 1, 'neumann_nodes': edges.astype(np.float64), 'dirichlet_nodes': dirichlet,
                'Q': Q}
    hist.update(work=work, f_ext=f_ext, mesh=mesh, pcg_iters=pcg_iters)
    return hist


def _refine_with_state(ctx, ops, on_device, context_factory, hist, coord, elem, s, U, Ep, mark, theta, materials):
    """Marks from the stress `s` of the step just accepted, marked refinement with its corner codes, and the transfer of the
    displacement `U` and the plastic strain `Ep` onto the children.  -> (the row of hist['adapt'], child coordinates, child
    elements, the transferred (U, Ep) as the next segment's ops take them).  With device vectors nothing but the counts of
    fep_mesh_mark comes back to the host before everything is enqueued; the row is read back afterwards."""
    from .estimate import mark_bulk
    from .midpoints import DeviceMesh, child_corners, refine_marked
    from .transfer import transfer_nodes, transfer_nodes_dev, transfer_points, transfer_points_dev
    t = LagrangeElementType.P1
    n_e, zz, eta = elem.shape[1], isinstance(mark, str), None

    def user_marks():
        marked = np.asarray(mark(hist, coord, elem)) != 0
        if marked.shape != (n_e,):
            raise ValueError(f'mark: one entry per element ({n_e},), got {marked.shape}')
        return marked

    if on_device:
        torch = ops.torch
        coord_d = torch.from_numpy(np.ascontiguousarray(coord)).to(ops.dev)
        elem_d = torch.from_numpy(np.ascontiguousarray(elem, dtype=np.int32)).to(ops.dev)
        with DeviceMesh(coord_d, elem_d, ctx.device, on_device=True) as m:
            if zz:
                eta2, stats, _ = ctx.estimate_dev(s.contiguous())
                marked, _ = mark_bulk(eta2, theta)
                counts = m.mark(marked, on_device=True)
            else:
                marked = user_marks()
                counts = m.mark(marked)
            c_d, e_d, p_d = m.refine_marked_dev()
            cor_d = m.child_corners_dev()
            U_c = transfer_nodes_dev(t, elem_d, e_d, p_d, cor_d, U, int(c_d.shape[1]))
            Ep_c = transfer_points_dev(t, p_d, cor_d, Ep.contiguous())
            if zz:
                eta = float(np.sqrt(float(stats.cpu()[0])))
                marked = marked.cpu().numpy()
            c, e = c_d.cpu().numpy(), e_d.cpu().numpy().astype(np.int64)
            parent, corners = p_d.cpu().numpy().astype(np.int64), cor_d.cpu().numpy()
        carried = (U_c, Ep_c)
        U_h, Ep_h = U_c.cpu().numpy(), Ep_c.cpu().numpy()
    else:
        mesh_device = None if context_factory is not None else ctx.device
        if zz:
            est = ops.estimate(s, {'type': t, 'elem': elem, 'coords': coord, 'materials': materials})
            if est['n_nonfinite']:
                raise ValueError(f"adapt_at: {est['n_nonfinite']} of {n_e} error indicators are not finite")
            eta = float(np.sqrt(est['total']))
            marked = np.asarray(mark_bulk(est['eta2'], theta, device=mesh_device)[0], dtype=bool)
        else:
            marked = user_marks()
        if mesh_device is None:
            c, e, parent = refine_marked(coord, elem, marked)
            corners = child_corners(coord, elem, marked)
        else:
            with DeviceMesh(coord, elem, mesh_device) as m:
                m.mark(marked)
                c, e, parent = m.refine_marked()
                corners = m.child_corners()
        counts = {'n_child': int(e.shape[1])}
        U_h = transfer_nodes(t, elem, e, parent, corners, np.asarray(ops.host(U)).reshape(-1, 2), n_n_child=c.shape[1],
                             device=mesh_device).reshape(-1)
        Ep_h = transfer_points(t, parent, corners, np.asarray(ops.host(Ep)), device=mesh_device)
        carried = (U_h, Ep_h)
    row = {'step': None, 'n_e': n_e, 'n_n': int(coord.shape[1]), 'n_marked': int(np.count_nonzero(marked)),
           'n_child': int(counts['n_child']), 'eta': eta, 'parent': parent, 'corners': corners, 'coords': c, 'elem': e,
           's': np.array(ops.host(s)), 'U': U_h.reshape((2, -1), order='F').copy(), 'Ep': np.array(Ep_h)}
    return row, c, e, carried

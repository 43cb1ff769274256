"""Closed-form load cycles through the whole stack on the GPU (tests/plastic_exact_cases.py): fep.MeshContext under
newton._load_history_loop for every material model and element type, with the host forms ('direct') and the device ops
('amg'), against closed forms that share nothing with newton.py; refinement in the middle of a history; the unloading steps
that need the loop's second attempt.

Bounds.  'direct': MARGIN (the project's 8x rule) times the CPU look-alike's recorded error against the same closed form
(PLASTIC_EXACT_CPU, re-measured by test_plastic_exact_host.py).  'amg': the standing 1e-9 of test_vm_gpu.py and
test_transfer_gpu.py for that solver (there against a CPU run, here against the closed form)."""
import functools
from importlib import import_module

import numpy as np
import pytest

import plastic_exact_cases as pc

pytestmark = pytest.mark.gpu

SOLVERS = ('direct', 'amg')
KRYLOV = 1e-9
newton = import_module(pc.fep.__name__ + '.newton')
vonmises = import_module(pc.fep.__name__ + '.vonmises')
midpoints = import_module(pc.fep.__name__ + '.midpoints')
transfer = import_module(pc.fep.__name__ + '.transfer')


def _gpu_context(*a):
    return pc.fep.MeshContext(*a)


@functools.lru_cache(maxsize=None)
def _gpu_runs(case, model, t, solver):
    """Every history and mesh size of the combination on fep.MeshContext -> list of (name, size, problem, hist, rows)."""
    out = []
    for name in pc.HISTORIES[case, model]:
        rows = pc.exact(case, model, name)
        for size in pc.sizes(t):
            prob = pc.problem(case, t, size)
            ctx = pc.make_context(_gpu_context, case, model, name, prob['elem'], prob['coord'], t)
            try:
                out.append((name, size, prob, pc.run(newton, ctx, prob, pc.loads(case, model, name), solver), rows))
            finally:
                ctx.close()
    return out


@pytest.mark.parametrize('solver', SOLVERS)
@pytest.mark.parametrize('case,model,t', pc.CASES)
def test_gpu_follows_the_closed_form(case, model, t, solver):
    """Every history runs to its end.  Per step the plastic count is the closed form's, 0 or n_int, all of it in n_smooth (the
    Mohr-Coulomb edge and the Drucker-Prager cone are no apex), and ind_p is uniform.  U and the plastic state of every step
    are the closed form's within the bound of the solver (module docstring).

    Measured on an MI355X against the closed form, the largest (U, state) error over the element types and mesh sizes:
                   'direct'              'amg'
        S vm     4.3e-15  5.1e-14     4.5e-15  4.5e-14
        S vmi    2.8e-14  1.1e-13     1.9e-14  1.3e-13
        S vmps   3.2e-15  4.5e-14     4.8e-15  6.0e-14
        C dp     4.0e-13  2.4e-11     4.0e-13  2.4e-11      (P4; the other types 3e-14 and 1e-12 at the most)
        C mc     1.7e-11  5.9e-10     1.7e-11  5.9e-10      (P4; the other types 9e-13 and 4e-11 at the most)
    The Krylov runs are as close to the closed form as the direct ones: four to six orders inside their standing 1e-9, except
    the state of Mohr-Coulomb on P4, where the CPU look-alike with the direct solve has the same 6e-10."""
    e_u = e_p = 0.0
    for name, size, prob, hist, rows in _gpu_runs(case, model, t, solver):
        assert hist['failed_at'] is None and len(hist['U']) == len(rows), (name, size, hist['failed_at'])
        n = prob['n_int']
        assert hist['counts'] == [(n * r['plastic'], 0) for r in rows], (name, size, hist['counts'])
        assert all(f.all() == f.any() == r['plastic'] for f, r in zip(hist['ind_p'], rows))
        assert (hist['pcg_iters'] is None) == (solver == 'direct')
        u, p = pc.errors(case, hist, rows, prob['coord'])
        print(f'{case} {model} {t} {solver} {name} {size}: U {u:.2e}  state {p:.2e}  retries {hist["retries"]}')
        e_u, e_p = max(e_u, u), max(e_p, p)
    rec_u, rec_p = pc.PLASTIC_EXACT_CPU[case, model, t]
    b_u, b_p = (pc.MARGIN * rec_u, pc.MARGIN * rec_p) if solver == 'direct' else (KRYLOV, KRYLOV)
    print(f'[plastic exact] {case} {model} {t} {solver}: U {e_u:.2e} (<= {b_u:.1e})  state {e_p:.2e} (<= {b_p:.1e})')
    assert e_u <= b_u and e_p <= b_p


@pytest.mark.parametrize('solver', SOLVERS)
@pytest.mark.parametrize('t', pc.TYPES)
def test_stall_history_completes(t, solver):
    """The 'vmi' cycle whose step 13 the loop used to give up on (P1, P4 on the CPU look-alike) runs to its end with both
    solvers.  Which steps take the second attempt is decided by the rounding of the converged state, so only this is asserted
    of them: a retry happens at an elastic step directly after a plastic one, and no other step took more than the 25 iterates
    of one attempt.  (A first attempt may end early: with 'amg' the conjugate gradients can break down on a tangent of the
    alternating iterates, which ends the attempt with a NaN stopping quantity.)"""
    for name, size, prob, hist, rows in _gpu_runs('S', 'vmi', t, solver):
        assert hist['failed_at'] is None and len(hist['U']) == len(rows)
        assert all(k > 0 and rows[k - 1]['plastic'] and not rows[k]['plastic'] for k in hist['retries']), hist['retries']
        assert all(hist['newton_its'][k] <= 25 for k in range(len(rows)) if k not in hist['retries'])
        print(f'vmi {t} {solver} {name} {size}: retries {hist["retries"]}  its {hist["newton_its"]}')


# ---------------------------------------------------------------------------------------
# refinement in the middle of the history
# ---------------------------------------------------------------------------------------
def _refine_p1(ctx, ops, hist, e1, c1, marked, U, Ep, model):
    """P1: the driver's own refinement step (vonmises._refine_with_state), host or device vectors as the ops are."""
    on_device = isinstance(ops, newton._DeviceOps)
    s = ops.step(U, Ep, want=('s',))['s']
    row, cc, ec, carried = vonmises._refine_with_state(ctx, ops, on_device, None, hist, c1, e1, s, U, Ep,
                                                       lambda h, c, e: marked, 0.5, pc.materials('S', model))
    return cc, ec, row['parent'], carried, row['Ep']


def _refine_p2(ctx, ops, prob, e1, c1, marked, U, Ep):
    """P2: DeviceMesh.refine_marked / child_corners and transfer_nodes / transfer_points, in their host-array forms for host
    vectors and in their device forms for device vectors."""
    on_device = isinstance(ops, newton._DeviceOps)
    with midpoints.DeviceMesh(c1, e1, ctx.device) as m:
        m.mark(marked)
        if not on_device:
            cc, ec, parent = m.refine_marked()
            corners = m.child_corners()
            child_elem, child_coord = pc.raised('P2', ec, cc)
            U_c = transfer.transfer_nodes('P2', prob['elem'], child_elem, parent, corners, np.asarray(U).reshape(-1, 2),
                                          n_n_child=child_coord.shape[1], device=ctx.device).reshape(-1)
            Ep_c = transfer.transfer_points('P2', parent, corners, np.asarray(Ep), device=ctx.device)
            return cc, ec, parent, (U_c, Ep_c), Ep_c
        torch = ops.torch
        c_d, e_d, p_d = m.refine_marked_dev()
        cor_d = m.child_corners_dev()
        cc, ec, parent = c_d.cpu().numpy(), e_d.cpu().numpy().astype(np.int64), p_d.cpu().numpy().astype(np.int64)
        child_elem, child_coord = pc.raised('P2', ec, cc)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(ops.dev)            # noqa: E731
        U_c = transfer.transfer_nodes_dev('P2', up(prob['elem']), up(child_elem), p_d, cor_d, U, child_coord.shape[1])
        Ep_c = transfer.transfer_points_dev('P2', p_d, cor_d, Ep.contiguous())
        return cc, ec, parent, (U_c, Ep_c), Ep_c.cpu().numpy()


@pytest.mark.parametrize('solver', SOLVERS)
@pytest.mark.parametrize('model,t', pc.REFINED)
def test_refined_history_stays_on_the_closed_form(model, t, solver):
    """After the plastic step REFINE_AFTER the left half of the mesh is marked, refined on the GPU, and U and the plastic state
    go to the children: with the host forms under 'direct', with device vectors under 'amg'.  The transferred U is the step's
    linear field on the children — within the parent run's own error plus the per-entry bound of
    test_transfer_host.test_polynomials_are_reproduced — every child point carries a parent point's state bit for bit, and the
    remaining steps, run from that state by _load_history_loop(U=, Ep=), stay on the closed form within the solver's bound
    ('direct': MARGIN times PLASTIC_EXACT_REFINED_CPU, the look-alike's error on the same refined history).  On the 33 children
    of 'vm' P1 the multigrid-preconditioned conjugate gradients break down on the fully plastic tangent (the V-cycle is
    indefinite there): the five plastic steps of the rest of the history are the loop's second attempts,
    solved with the block-Jacobi preconditioner, and land on the closed form like the others (U 3.1e-15, state 6.7e-15)."""
    name, k = pc.REFINE_HISTORY[model], pc.REFINE_AFTER
    rows, zetas = pc.exact('S', model, name), pc.loads('S', model, name)
    e1, c1, marked = pc.refine_parent()
    prob = pc.problem('S', t, on=pc.raised(t, e1, c1))
    ctx = pc.make_context(_gpu_context, 'S', model, name, prob['elem'], prob['coord'], t)
    ops = None
    try:
        first = pc.run(newton, ctx, prob, zetas[:k + 1], solver, keep_ops=True)
        ops = first['ops']
        assert first['failed_at'] is None and rows[k]['plastic']
        U, Ep = first['state']
        if t == 'P1':
            cc, ec, parent, carried, Ep_c = _refine_p1(ctx, ops, first, e1, c1, marked, U, Ep, model)
        else:
            cc, ec, parent, carried, Ep_c = _refine_p2(ctx, ops, prob, e1, c1, marked, U, Ep)
        U_c = np.array(ops.host(carried[0])).reshape((2, -1), order='F')
    finally:
        if ops is not None:
            ops.close()
        ctx.close()
    assert ec.shape[1] > e1.shape[1] and (np.bincount(parent) == 1).any()
    child = pc.problem('S', t, on=pc.raised(t, ec, cc))
    pc.check_child_state(t, parent, first['Ep'][-1], Ep_c)
    Ux = pc.displacement('S', rows[k], child['coord'])
    parent_err = pc.errors('S', first, rows[:k + 1], prob['coord'])
    err_c = float(np.abs(U_c - Ux).max() / np.abs(Ux).max())
    ctx2 = pc.make_context(_gpu_context, 'S', model, name, child['elem'], child['coord'], t)
    try:
        rest = pc.run(newton, ctx2, child, zetas[k + 1:], solver, U=carried[0], Ep=carried[1])
    finally:
        ctx2.close()
    assert rest['failed_at'] is None and len(rest['U']) == len(rows) - k - 1
    assert rest['counts'] == [(child['n_int'] * r['plastic'], 0) for r in rows[k + 1:]]
    rest_err = pc.errors('S', rest, rows[k + 1:], child['coord'])
    e_u, e_p = max(parent_err[0], rest_err[0]), max(parent_err[1], rest_err[1])
    rec_u, rec_p = pc.PLASTIC_EXACT_REFINED_CPU[model, t]
    b_u, b_p = (pc.MARGIN * rec_u, pc.MARGIN * rec_p) if solver == 'direct' else (KRYLOV, KRYLOV)
    print(f'[plastic exact] refined {model} {t} {solver}: transferred U {err_c:.2e} (<= {parent_err[0] + pc.transfer_scale(t):.2e})  '
          f'U {e_u:.2e} (<= {b_u:.1e})  state {e_p:.2e} (<= {b_p:.1e})  retries {first["retries"]} {rest["retries"]}')
    assert err_c <= parent_err[0] + pc.transfer_scale(t)
    assert e_u <= b_u and e_p <= b_p

"""
The GPU solver's iterates against the float64 restatement of tests/amg_ref.py: the first conjugate-gradient iterates of
the multigrid solve (V-cycle: level-0 block Jacobi and Chebyshev passes on the single-precision K, node-block transfers,
numeric Galerkin refresh, 3x3 and coarsest inverses, tail_kernel) and of the block-Jacobi solve, full solves, the
independence of `check_every`, and the device-side power iteration of the set-up.  CG corrects a wrong preconditioner
(it only costs iterations), so the iterates x_1 .. x_4 are compared, not solutions.

Tolerances: the kernels do their arithmetic in double on the operands the restatement rounds the same way, so the two
differ by summation order and by the pivoting of the coarsest inverse only; each bound is next to its measured value.
node3_kernel's four-nodes-per-lane-group form (coarse levels of 262 144 nodes and more) and product_kernel's one-lane form
are compared in the same way by test_solver_forms_gpu.py, on a hierarchy made for them (amg_ref.singleton_hierarchy).
"""
import numpy as np
import pytest
import scipy.sparse.linalg as sspl

import amg_ref
from conftest import dp_materials, needs_ablation_build, relerr

pytestmark = pytest.mark.gpu

K_ITERS = 4
# Worst differences measured on the MI355X over every case, matrix, right-hand side and k of this module, bounds at most
# 100x above them (a restatement without the single-precision rounding would be ~1e-7 away):
ITER_TOL = 5e-12            # multigrid x_k: 7.2e-14 (P1-64 without the tail, plastic tangent, x_4)
RELRES_TOL = 3e-12          # multigrid relres_k: 3.6e-14
JACOBI_TOL = 1e-13          # block-Jacobi x_k and relres_k: 1.9e-15 (no single precision, no coarse inverse: rounding only)

# (element type, cells per side, coarse_nodes of setup_amg (None: its default), whether tail_kernel runs with the refresh)
CASES = [('P1', 64, 30, True), ('P2', 16, 30, True), ('Q1', 32, 30, True), ('Q2', 12, 30, True), ('P1', 64, None, False)]
CASE_IDS = ['P1-64', 'P2-16', 'Q1-32', 'Q2-12', 'P1-64-no-tail']

_PROBLEMS = {}


def _problem(fep, et, n):
    """mesh, context, {'elastic': K_elast, 'plastic': tangent 4 load steps into the footing run}, free DOFs; cached."""
    if (et, n) not in _PROBLEMS:
        mesh = fep.square_mesh(n, et, 10)
        ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'], element_type=et)
        ctx.set_materials(*dp_materials(ctx.n_int))
        K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
        h = fep.solve_strip_footing(et, n_cells=n, max_steps=4)
        r = ctx.step(h['U'][-1], h['Ep'], want=('K',))
        assert r['n_smooth'] + r['n_apex'] > 0
        _PROBLEMS[et, n] = (mesh, ctx, {'elastic': K_el, 'plastic': r['K']}, mesh['Q'].flatten(order='F'))
    return _PROBLEMS[et, n]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for _, ctx, _, _ in _PROBLEMS.values():
        ctx.close()
    _PROBLEMS.clear()


def _rhs(qf):
    """random on the free DOFs; the same with large values on the constrained DOFs (ignored: r = Q b); one interior node"""
    rng = np.random.default_rng(17)
    b = np.where(qf, rng.normal(size=qf.size), 0.0)
    bc = np.where(qf, b, 1e6 * rng.normal(size=qf.size))
    both_free = np.flatnonzero(qf[0::2] & qf[1::2])
    node = both_free[both_free.size // 2]
    b1 = np.zeros(qf.size)
    b1[2 * node:2 * node + 2] = (1.0, -0.5)
    return {'random': b, 'constrained': bc, 'one-node': b1}


def _iterate_errors(sol, K, qf, M, cg, precond):
    """Device solves with max_iter = 1 .. K_ITERS for every right-hand side against the restated CG's iterates:
    [(label, relerr of x_k, relative relres_k difference)].  Asserts the bookkeeping of every solve."""
    out = []
    for name, b in _rhs(qf).items():
        ref = cg(K, qf, b, M, max_iter=K_ITERS, keep=True)
        assert ref['state'] == 0 and len(ref['history']) == K_ITERS
        for k in range(1, K_ITERS + 1):
            x = sol.solve_host(K, b, rtol=1e-14, max_iter=k, precond=precond)
            assert (sol.last['state'], sol.last['iters']) == (0, k), (name, k, sol.last)
            assert np.all(x[~qf] == 0.0)
            xr, rr = ref['history'][k - 1]
            out.append(((name, k), relerr(x, xr), abs(sol.last['relres'] - rr) / rr))
        if name == 'constrained':             # the constrained entries are ignored bit for bit
            assert np.array_equal(x, sol.solve_host(K, _rhs(qf)['random'], rtol=1e-14, max_iter=K_ITERS, precond=precond))
    return out


def _assert_errors(errs, what, x_tol=ITER_TOL, relres_tol=RELRES_TOL):
    worst_x = max(errs, key=lambda e: e[1])
    worst_r = max(errs, key=lambda e: e[2])
    assert worst_x[1] <= x_tol, (what, worst_x)
    assert worst_r[2] <= relres_tol, (what, worst_r)


def _amg_solver(fep, ctx, qf, K_el, mesh, coarse_nodes, refresh):
    sol = fep.KrylovSolver(ctx, qf)
    kw = {} if coarse_nodes is None else {'coarse_nodes': coarse_nodes}
    sol.setup_amg(K_el, mesh['coordinates'], refresh=refresh, **kw)
    assert sol.amg_refresh is refresh and sol.amg_hierarchy is not None
    return sol


def vcycle_errors(fep, et, n, coarse_nodes, tail, refresh):
    mesh, ctx, Ks, qf = _problem(fep, et, n)
    sol = _amg_solver(fep, ctx, qf, Ks['elastic'], mesh, coarse_nodes, refresh)
    # which bottom of the cycle this case exercises (vcycle_chebyshev's `kt`)
    assert amg_ref.tail_runs(sol.amg_levels, refresh=refresh) is (tail and refresh), sol.amg_levels
    errs = []
    for mat, K in Ks.items():
        M = amg_ref.VCycle(K, qf, sol.amg_hierarchy, refresh=refresh)
        errs += [((mat,) + lab, ex, er) for lab, ex, er in _iterate_errors(sol, K, qf, M, amg_ref.pcg, 'amg')]
    sol.close()
    return errs


@pytest.mark.parametrize('refresh', [True, False], ids=['refresh', 'stale'])
@pytest.mark.parametrize('et,n,coarse_nodes,tail', CASES, ids=CASE_IDS)
def test_multigrid_iterates_match_the_float64_restatement(fep, et, n, coarse_nodes, tail, refresh):
    """x_1 .. x_4 and relres_1 .. relres_4 of fep_solver_amg_pcg_dev on K_elast and on a plastic tangent (with the refresh
    the coarse operators then differ from the pushed ones), for three right-hand sides."""
    _assert_errors(vcycle_errors(fep, et, n, coarse_nodes, tail, refresh), (et, n, refresh))


def jacobi_errors(fep, et, n):
    mesh, ctx, Ks, qf = _problem(fep, et, n)
    sol = fep.KrylovSolver(ctx, qf)
    errs = []
    for mat, K in Ks.items():
        M = amg_ref.block_jacobi(K, qf)
        errs += [((mat,) + lab, ex, er) for lab, ex, er in _iterate_errors(sol, K, qf, M, amg_ref.pcg_single_reduction, 'jacobi')]
    sol.close()
    return errs


@pytest.mark.parametrize('et,n', [('P1', 64), ('P2', 16), ('Q1', 32), ('Q2', 12)])
def test_block_jacobi_iterates_match_the_float64_restatement(fep, et, n):
    """fep_solver_pcg_dev (single-reduction CG, block_jacobi_kernel's symmetrised 2x2 inverses of the double K)."""
    _assert_errors(jacobi_errors(fep, et, n), (et, n), JACOBI_TOL, JACOBI_TOL)


@pytest.mark.parametrize('et,n', [('P1', 64), ('Q2', 12)])
def test_full_multigrid_solves_match_the_restated_pcg(fep, et, n):
    """To rtol = 1e-10 on the plastic tangent with the refresh: the iteration counts of device and restatement within one,
    the device's solution and the restatement's iterate of the same count to 1e-12, near SuperLU's solution."""
    mesh, ctx, Ks, qf = _problem(fep, et, n)
    K = Ks['plastic']
    sol = _amg_solver(fep, ctx, qf, Ks['elastic'], mesh, 30, True)
    b = _rhs(qf)['random']
    x = sol.solve_host(K, b, rtol=1e-10)
    it = sol.last['iters']
    assert sol.last['state'] == 1 and it > K_ITERS
    ref = amg_ref.pcg(K, qf, b, amg_ref.VCycle(K, qf, sol.amg_hierarchy), max_iter=it + 1, rtol=1e-10, keep=True)
    assert ref['state'] == 1 and abs(it - ref['iters']) <= 1, (sol.last, ref['iters'])
    assert relerr(x, ref['history'][it - 1][0]) <= 1e-12     # measured 1.5e-14 (same counts: 50 and 54 iterations)
    direct = np.zeros(qf.size)
    direct[qf] = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
    assert relerr(x, direct) <= 1e-5                        # (relres 1e-10 x condition number ~1e5)
    sol.close()


@pytest.mark.parametrize('precond', ['amg', 'jacobi'])
def test_check_every_does_not_change_the_solve(fep, precond):
    """How often the host reads the device state (and how many iterations next_batch enqueues past convergence, which run
    frozen) changes nothing: x, iters and relres bit-identical for check_every 1, 2, 7 and the default."""
    mesh, ctx, Ks, qf = _problem(fep, 'P1', 64)
    sol = _amg_solver(fep, ctx, qf, Ks['elastic'], mesh, 30, True)
    K = Ks['plastic']
    b = _rhs(qf)['random']
    runs = []
    for ce in (1, 2, 7, 0):
        x = sol.solve_host(K, b, rtol=1e-10, check_every=ce, precond=precond)
        assert sol.last['state'] == 1
        runs.append((x, sol.last['iters'], sol.last['relres']))
    for x, it, rr in runs[1:]:
        assert np.array_equal(x, runs[0][0]) and it == runs[0][1] and rr == runs[0][2]
    sol.close()


@pytest.mark.parametrize('et,n', [('P1', 64), ('Q2', 12)])
def test_device_power_iteration_is_the_host_one(fep, et, n):
    """KrylovSolver._rho_dev (the mesh level's eigenvalue estimate of the set-up Newton drivers run) against solver._rho on
    the masked operator: the same 15 steps from the same start, the products on the device."""
    mesh, ctx, Ks, qf = _problem(fep, et, n)
    sol = fep.KrylovSolver(ctx, qf)
    K = Ks['elastic']
    A = amg_ref.solver._masked_operator(K, qf.astype(np.float64))
    Di = amg_ref.solver._block_diag_inverse(A, 2)
    host = amg_ref.solver._rho(A, Di)
    dev = sol._rho_dev(K.data)(A, Di)
    assert abs(dev - host) <= 1e-14 * host, (dev, host)       # measured <= 2.2e-16: summation order of the products
    sol.close()


# measurement switches of the -DFEP_ABLATION build, each against the restatement with the matching switch
ABLATIONS = [('FEP_AMG_SMOOTHER', 'jacobi', {'smoother': 'jacobi'}), ('FEP_AMG_FP32', '0', {'fp32': False}),
             ('FEP_AMG_TAIL', '0', {}), ('FEP_AMG_BLOCK_TRANSFERS', '0', {'fp32_transfers': False})]


@pytest.mark.parametrize('var,value,kw', ABLATIONS, ids=[a[0] for a in ABLATIONS])
def test_ablation_variants_match_the_float64_restatement(fep, var, value, kw, monkeypatch):
    """The V-cycle variants behind FEP_AMG_* (two damped block-Jacobi sweeps, no single-precision copies, the bottom of the
    cycle as separate launches, double-precision CSR transfers) against the restatement with the same switch."""
    needs_ablation_build(fep)
    monkeypatch.setenv(var, value)
    mesh, ctx, Ks, qf = _problem(fep, 'P1', 64)
    sol = _amg_solver(fep, ctx, qf, Ks['elastic'], mesh, 30, True)
    # P1-64 runs the tail in the product; each of these switches leaves it out
    assert not amg_ref.tail_runs(sol.amg_levels, fp32=kw.get('fp32', True), tail=var != 'FEP_AMG_TAIL',
                                 block_transfers=kw.get('fp32_transfers', True), smoother=kw.get('smoother', 'chebyshev'))
    errs = []
    for mat, K in Ks.items():
        M = amg_ref.VCycle(K, qf, sol.amg_hierarchy, **kw)
        errs += [((mat,) + lab, ex, er) for lab, ex, er in _iterate_errors(sol, K, qf, M, amg_ref.pcg, 'amg')]
    sol.close()
    _assert_errors(errs, var)

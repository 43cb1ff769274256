"""
The solver kernels of fep_solver.hip off the footing's squares: the cases of tests/solver_cases.py (tsx tunnel P1 / P2 / P4,
renumbered Delaunay triangulations, fans with a row of ~250 blocks, nodes of no element, and three small rectangles at the
edges of spmv_kernel's 128 nodes per workgroup) against the float64 restatement of tests/amg_ref.py, iterate by iterate as
test_vcycle_gpu.py does on squares, with that module's helpers.  K_elast and the tangent both come from ctx.step, so device
and restatement read the same values.  tests/test_solver_cases_host.py checks on the CPU that the restatement alone meets
every condition asserted on the inputs here, and measures the ulp sensitivities the bounds below are derived from.

Bounds.  test_vcycle_gpu's own (ITER_TOL 5e-12, RELRES_TOL 3e-12, JACOBI_TOL 1e-13) come from measurements on squares; a row of
251 blocks sums 30 times more terms than any row there.  A case's bound is the larger of the module's bound and 30 x that
case's ulp sensitivity (solver_cases.bound: largest relerr of x_1 .. x_4 of the restatement between K and K with every value
moved by one unit of rounding; 30 is the ratio the squares' bounds keep to their measured values, rounded down), and never
above 1e-9: the restatement without the single-precision roundings is 5e-8 to 2e-5 away on these meshes.  spmv has a derived
bound per entry (test_spmv_per_entry).

Per case: nodes per level | V-cycle form compared | ulp sensitivity on the CPU (V-cycle, block Jacobi) | bounds used
(multigrid x_k, relres_k; block Jacobi) | worst values measured on the MI355X (multigrid x_k, relres_k; block Jacobi x_k or
relres_k):
  tsx-P1         476, 54, 9         refresh  8.3e-15 9.6e-16   5e-12 3e-12 1e-13      5.2e-15 5.5e-15 2.3e-15
  tsx-P2         1839, 72, 9        refresh  3.2e-14 3.1e-15   5e-12 3e-12 1e-13      1.6e-14 2.4e-14 3.8e-15
  tsx-P4         7226, 82, 9        refresh  3.6e-14 1.2e-15   5e-12 3e-12 1e-13      1.0e-14 1.8e-14 2.0e-15
  delaunay40-P1  1681, 172, 15      refresh  2.6e-14 1.3e-15   5e-12 3e-12 1e-13      1.7e-14 2.0e-14 1.5e-15
  delaunay14-P2  841, 46, 8         refresh  9.6e-15 1.3e-15   5e-12 3e-12 1e-13      6.8e-15 5.1e-15 2.8e-15
  delaunay8-P4   1089, 23           refresh  2.5e-14 1.9e-15   5e-12 3e-12 1e-13      7.2e-15 5.6e-15 2.1e-15
  delaunay50-P1  2601, 263, 21      refresh  1.3e-14 1.3e-15   5e-12 3e-12 1e-13      1.2e-14 7.0e-15 1.7e-15
  delaunay58-P1  3481, 346, 25      refresh  2.6e-14 1.2e-15   5e-12 3e-12 1e-13      9.9e-15 7.4e-15 1.2e-15
  delaunay62-P1  3969, 392, 27      refresh  3.0e-14 1.5e-15   5e-12 3e-12 1e-13      8.8e-15 1.1e-14 3.1e-15
  delaunay72-P1  5329, 524, 32, 6   refresh  5.3e-14 1.1e-15   5e-12 3e-12 1e-13      8.6e-15 7.1e-15 1.5e-15
  fan250-P1      501, 251           stale    2.0e-13 1.3e-14   6e-12 6e-12 3.9e-13    1.1e-13 2.0e-13 2.0e-14
  fan84-P2       589, 203, 169      stale    9.7e-14 8.4e-15   5e-12 3e-12 2.5e-13    3.9e-14 2.3e-14 3.9e-15
  fan24-P4       625, 205, 193      stale    2.9e-14 2.1e-15   5e-12 3e-12 1e-13      3.0e-14 1.3e-14 1.9e-15
  orphans-P1     441, 59, 17        refresh  1.1e-14 1.9e-15   5e-12 3e-12 1e-13      8.4e-15 1.1e-14 2.9e-15
  rect-15x7      128 nodes          -        -       1.2e-15   -           1e-13      -       -       1.3e-15
  rect-42x2      129 nodes          -        -       1.2e-15   -           1e-13      -       -       2.2e-15
  rect-1x1       4 nodes            -        -       4.3e-14   -           1.3e-12    -       -       8.0e-15
('stale': the coarsest level exceeds the 256 DOFs of dense_inverse_kernel, fep_solver_amg_enable_refresh answers FEP_ERANGE
and setup_amg continues with the operators of K_elast; the tail needs the refresh, so it is off there.)

Full solves to rtol = 1e-10 (iterations of device = restatement; x against the restated iterate; against SuperLU): tsx-P4 377,
2.8e-14, 6.2e-11; delaunay58-P1 62, 1.6e-14, 4.5e-11; fan250-P1 109, 2.0e-14, 1.1e-11; orphans-P1 43, 1.1e-15, 6.7e-12.  spmv: at most
0.19 of its per-entry bound.  Power iteration: device and host equal to 2.2e-16.

node3_kernel's four-nodes-per-lane-group form (coarse levels of 262 144 nodes and more) and product_kernel's one-lane form
are compared in the same way by test_solver_forms_gpu.py, on a hierarchy made for them (amg_ref.singleton_hierarchy).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as sspl

import amg_ref
import solver_cases as sc
from conftest import dp_materials, relerr
from test_vcycle_gpu import ITER_TOL, JACOBI_TOL, K_ITERS, RELRES_TOL, _assert_errors, _iterate_errors, _rhs

pytestmark = pytest.mark.gpu

_PROBLEMS = {}
_SOLVERS = {}


def _problem(fep, name):
    """context, {'elastic': K_elast, 'plastic': the tangent at solver_cases.displacement}, free DOFs, coordinates; cached."""
    if name not in _PROBLEMS:
        elem, coord, et = sc.mesh(name)
        ctx = fep.MeshContext(elem, coord, element_type=et)
        ctx.set_materials(*dp_materials(ctx.n_int))
        K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
        r = ctx.step(sc.displacement(name), np.zeros((4, ctx.n_int)), want=('K',))
        assert 0 < r['n_smooth'] + r['n_apex'] < ctx.n_int
        _PROBLEMS[name] = (ctx, {'elastic': K_el, 'plastic': r['K']}, sc.free_dofs(name), coord)
    return _PROBLEMS[name]


def _amg_solver(fep, name):
    """The case's solver after setup_amg(refresh=True) on K_elast; cached (a solve leaves no state behind that the next one
    reads: test_full_solves asserts bit-identical repeats)."""
    if name not in _SOLVERS:
        ctx, Ks, qf, coord = _problem(fep, name)
        sol = fep.KrylovSolver(ctx, qf)
        sol.setup_amg(Ks['elastic'], coord, coarse_nodes=sc.CASES[name]['coarse_nodes'], refresh=True)
        _SOLVERS[name] = sol
    return _SOLVERS[name]


@pytest.fixture(scope='module', autouse=True)
def _close_everything():
    yield
    for sol in _SOLVERS.values():
        sol.close()
    for ctx, _, _, _ in _PROBLEMS.values():
        ctx.close()
    _SOLVERS.clear()
    _PROBLEMS.clear()


def _worst(errs):
    return max(e[1] for e in errs), max(e[2] for e in errs)


@pytest.mark.parametrize('name', list(sc.CASES))
def test_multigrid_iterates_match_the_float64_restatement(fep, name):
    """x_1 .. x_4 and relres_1 .. relres_4 of fep_solver_amg_pcg_dev on K_elast and on the plastic tangent, three right-hand
    sides, against amg_ref.VCycle in the form the table records for the case."""
    c = sc.CASES[name]
    ctx, Ks, qf, coord = _problem(fep, name)
    sol = _amg_solver(fep, name)
    assert sol.amg_refresh is c['refresh'] and sol.amg_hierarchy is not None
    errs = []
    for mat, K in Ks.items():
        M = amg_ref.VCycle(K, qf, sol.amg_hierarchy, refresh=c['refresh'])
        errs += [((mat,) + lab, ex, er) for lab, ex, er in _iterate_errors(sol, K, qf, M, amg_ref.pcg, 'amg')]
    x_tol, r_tol = sc.bound(ITER_TOL, c['sens_vcycle']), sc.bound(RELRES_TOL, c['sens_vcycle'])
    print('\n[measured] %s multigrid x_k %.2e (bound %.1e) relres_k %.2e (bound %.1e)' % ((name,) + sum(zip(_worst(errs), (x_tol, r_tol)), ())))
    _assert_errors(errs, name, x_tol, r_tol)


@pytest.mark.parametrize('name', list(sc.ALL))
def test_block_jacobi_iterates_match_the_float64_restatement(fep, name):
    """fep_solver_pcg_dev: block_jacobi_kernel, spmv_kernel with its partial sums, the single-reduction CG."""
    ctx, Ks, qf, coord = _problem(fep, name)
    sol = fep.KrylovSolver(ctx, qf)
    errs = []
    for mat, K in Ks.items():
        M = amg_ref.block_jacobi(K, qf)
        errs += [((mat,) + lab, ex, er) for lab, ex, er in _iterate_errors(sol, K, qf, M, amg_ref.pcg_single_reduction, 'jacobi')]
    sol.close()
    tol = sc.bound(JACOBI_TOL, sc.ALL[name]['sens_jacobi'])
    print('\n[measured] %s block Jacobi x_k %.2e relres_k %.2e (bound %.1e)' % ((name,) + _worst(errs) + (tol,)))
    _assert_errors(errs, name, tol, tol)


@pytest.mark.parametrize('name', list(sc.CASES))
def test_hierarchy_takes_the_recorded_form(fep, name):
    """The form of the cycle each case is in the table for: refresh or the fallback, tail_kernel or the separate launches."""
    c = sc.CASES[name]
    ctx, Ks, qf, coord = _problem(fep, name)
    sol = _amg_solver(fep, name)
    assert sol.amg_refresh is c['refresh']
    assert amg_ref.tail_runs(sol.amg_levels, refresh=sol.amg_refresh) is c['tail'], sol.amg_levels
    nodes = (sol.amg_levels[0][0] // 2,) + tuple(n // 3 for n, _ in sol.amg_levels[1:])
    assert nodes == c['nodes']
    if c['kind'] == 'fan':
        # the coarsest level is beyond dense_inverse_kernel: setup_amg got FEP_ERANGE, pushed the levels again and went on
        # with the operators of K_elast (usable: the iterate and full-solve tests run on this solver); no refresh to call
        import torch
        assert sol.amg_levels[-1][0] > 256
        k = torch.from_numpy(np.array(Ks['plastic'].data)).to(sol._dev)
        rc = fep.lib().fep_solver_amg_refresh_dev(sol._h, C.c_void_p(torch.cuda.current_stream(sol._dev).cuda_stream),
                                                  C.c_void_p(k.data_ptr()))
        assert rc == -6                                                   # FEP_ESTATE
        x = sol.solve_host(Ks['plastic'], _rhs(qf)['random'], rtol=1e-10)
        assert sol.last['state'] == 1 and sol.last['precond'] == 'amg' and np.isfinite(x).all()
    if name == 'delaunay62-P1':                   # the tail is off for the 8 nodes over kTailNodes alone
        assert sol.amg_levels[-2][0] // 3 == amg_ref.TAIL_NODES + 8 and sol.amg_levels[-1][0] <= amg_ref.TAIL_COARSE
        assert sol.amg_levels[-1][0] % 3 == 0 and len(sol.amg_levels) == 3
    if name == 'delaunay72-P1':
        assert len(sol.amg_levels) == 4
    if name == 'delaunay8-P4':                    # one transfer only: no smoothed coarse level for the tail to take
        assert len(sol.amg_levels) == 2


@pytest.mark.parametrize('name', sc.FULL_SOLVES)
def test_full_solves_match_the_restated_pcg(fep, name):
    """To rtol = 1e-10 on the plastic tangent: the iteration counts of device and restatement within one, the device's
    solution and the restatement's iterate of the same count to 1e-12, near SuperLU's solution (the assertions of
    test_vcycle_gpu.test_full_multigrid_solves_match_the_restated_pcg); bit-identical on a second call and for check_every
    1, 7 and the default; exactly 0 on constrained DOFs, the nodes of no element among them."""
    c = sc.CASES[name]
    ctx, Ks, qf, coord = _problem(fep, name)
    K = Ks['plastic']
    sol = _amg_solver(fep, name)
    b = _rhs(qf)['random']
    x = sol.solve_host(K, b, rtol=1e-10)
    it, rr = sol.last['iters'], sol.last['relres']
    assert sol.last['state'] == 1 and it > K_ITERS
    for ce in (0, 1, 7):
        assert np.array_equal(x, sol.solve_host(K, b, rtol=1e-10, check_every=ce)), ce
        assert (sol.last['state'], sol.last['iters'], sol.last['relres']) == (1, it, rr), ce
    assert np.all(x[~qf] == 0.0)
    orphans = sc.orphan_nodes(name)
    assert np.all(x.reshape(-1, 2)[orphans] == 0.0) and (name != 'orphans-P1' or orphans.size > 0)
    M = amg_ref.VCycle(K, qf, sol.amg_hierarchy, refresh=c['refresh'])
    ref = amg_ref.pcg(K, qf, b, M, max_iter=it + 1, rtol=1e-10, keep=True)
    direct = np.zeros(qf.size)
    direct[qf] = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
    print('\n[measured] %s full solve: iterations %d (restatement %d), x against the restated iterate %.2e, against SuperLU %.2e'
          % (name, it, ref['iters'], relerr(x, ref['history'][min(it, len(ref['history'])) - 1][0]), relerr(x, direct)))
    assert ref['state'] == 1 and abs(it - ref['iters']) <= 1, (sol.last, ref['iters'])
    assert relerr(x, ref['history'][it - 1][0]) <= 1e-12
    assert relerr(x, direct) <= 1e-5


def _exact_rows(K, x):
    """((K x)_i, sum_j |K_ij| |x_j|) in extended precision, the products summed per row."""
    ld = np.longdouble
    prod = K.data.astype(ld) * x[K.indices].astype(ld)
    nonempty = np.flatnonzero(np.diff(K.indptr) > 0)
    y, s = np.zeros(K.shape[0], dtype=ld), np.zeros(K.shape[0], dtype=ld)
    if nonempty.size:
        y[nonempty] = np.add.reduceat(prod, K.indptr[:-1][nonempty])
        s[nonempty] = np.add.reduceat(np.abs(prod), K.indptr[:-1][nonempty])
    return y, s


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('name', list(sc.ALL))
def test_spmv_per_entry(fep, name, masked):
    """|y_i - (K x)_i| <= (2 deg_i + 2) u sum_j |K_ij| |x_j| with deg_i the blocks of the node's row and u = 2^-53: the
    standard bound of a sum of 4 deg_i products in any order (the kernel's 8 lanes and their butterfly are one such order),
    the right side in extended precision.  Rows of constrained DOFs are exactly 0 when masked; an empty row is exactly 0."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    ctx, Ks, qf, coord = _problem(fep, name)
    K = Ks['plastic']
    sol = fep.KrylovSolver(ctx, qf)
    x = np.random.default_rng(29).normal(size=ctx.n_dof)
    if masked:
        x[~qf] = 0.0
    y = sol.spmv(K.data, x, masked=masked).cpu().numpy()
    sol.close()
    ip, _ = ctx.pattern()
    assert np.array_equal(ip, K.indptr)
    deg = np.repeat(np.diff(ip)[0::2] // 2, 2)
    assert np.array_equal(deg[0::2], sc.row_blocks(name))
    exact, scale = _exact_rows(K, x)
    if masked:
        assert np.all(y[~qf] == 0.0)
        exact[~qf] = 0.0
    assert np.all(y[deg == 0] == 0.0)
    err = np.abs(y.astype(np.longdouble) - exact)
    limit = (2 * deg + 2) * np.longdouble(2.0 ** -53) * scale
    worst = float(np.max(np.where(scale > 0, err / np.where(scale > 0, limit, 1), 0.0)))
    print('\n[measured] %s spmv %s: worst error / bound %.3f' % (name, 'masked' if masked else 'plain', worst))
    bad = np.flatnonzero(err > limit)
    assert bad.size == 0, (name, bad[:5], err[bad[:5]], limit[bad[:5]])


@pytest.mark.parametrize('name', ['tsx-P4', 'fan250-P1'])
def test_device_power_iteration_is_the_host_one(fep, name):
    """KrylovSolver._rho_dev against solver._rho on the masked operator, as test_vcycle_gpu's test on squares."""
    ctx, Ks, qf, coord = _problem(fep, name)
    sol = fep.KrylovSolver(ctx, qf)
    K = Ks['elastic']
    A = amg_ref.solver._masked_operator(K, qf.astype(np.float64))
    Di = amg_ref.solver._block_diag_inverse(A, 2)
    host = amg_ref.solver._rho(A, Di)
    dev = sol._rho_dev(K.data)(A, Di)
    sol.close()
    print('\n[measured] %s power iteration: device %.17g host %.17g' % (name, dev, host))
    assert abs(dev - host) <= 1e-14 * host, (dev, host)


def test_nodes_of_no_element(fep):
    """A node of no element has two empty rows in ctx.pattern(), fep_solver_create accepts them, and block_jacobi_kernel,
    which finds no diagonal block there, takes the identity: with those DOFs left FREE the first block-Jacobi iterate is
    the restatement's (x_1 = alpha b on the node; K is singular under that mask, one iterate is all it is good for)."""
    name = 'orphans-P1'
    ctx, Ks, qf, coord = _problem(fep, name)
    orphans = sc.orphan_nodes(name)
    assert orphans.size > 0
    ip, ix = ctx.pattern()
    for n in orphans:
        assert ip[2 * n] == ip[2 * n + 1] == ip[2 * n + 2]
    assert not np.isin(ix // 2, orphans).any()
    K = Ks['plastic']
    assert np.array_equal(K.indptr, ip)
    free = qf.copy()
    free.reshape(-1, 2)[orphans] = True
    sol = fep.KrylovSolver(ctx, free)
    assert sol.n_free == int(free.sum())
    b = _rhs(free)['random']
    assert np.all(b.reshape(-1, 2)[orphans] != 0.0)
    x = sol.solve_host(K, b, rtol=1e-14, max_iter=1, precond='jacobi')
    assert (sol.last['state'], sol.last['iters']) == (0, 1)
    sol.close()
    ref = amg_ref.pcg_single_reduction(K, free, b, amg_ref.block_jacobi(K, free), max_iter=1, keep=True)
    assert ref['state'] == 0
    xr = ref['history'][0][0]
    assert np.all(xr.reshape(-1, 2)[orphans] != 0.0)
    ratio = x.reshape(-1, 2)[orphans] / b.reshape(-1, 2)[orphans]            # alpha, whatever the node
    assert np.abs(ratio - ratio.ravel()[0]).max() <= 4 * 2.0 ** -53 * abs(ratio.ravel()[0])
    assert relerr(x, xr) <= JACOBI_TOL
    # under the table's mask those nodes are constrained: every solve leaves exactly 0 there (test_full_solves_... too)
    sol = fep.KrylovSolver(ctx, qf)
    x = sol.solve_host(K, _rhs(qf)['constrained'], rtol=1e-10, precond='jacobi')
    assert sol.last['state'] == 1 and np.all(x.reshape(-1, 2)[orphans] == 0.0)
    sol.close()

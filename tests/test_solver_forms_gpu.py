"""
The kernel forms fep_solver.hip picks by size, which no hierarchy of the other solver tests is large enough to reach:
  - node3_kernel<MODE, AV, 4>, four nodes per lane group, taken by vcycle_chebyshev on a coarse level of at least
    128 * 2048 = 262 144 nodes (`big`; amg_ref.node3_four_pass);
  - product_kernel<1>, one lane per output entry, taken by product_apply for a refresh product of fewer than three terms per
    entry (amg_ref.product_lanes).
Both are reached on meshes of 2.6 * 10^5 nodes with amg_ref.singleton_hierarchy: its first transfer gives every mesh node an
aggregate of its own and is not smoothed, so level 1 has the mesh's node count and node-block pattern and both products of
transfer 0 have at most one term per entry; ordinary smoothed aggregation continues below.  The device's CG iterates x_1 ..
x_4 are compared with the float64 restatement (amg_ref.VCycle on the same level dicts), as in test_vcycle_gpu.py and
test_solver_shapes_gpu.py and with their helpers.  K_elast and the plastic tangent both come from ctx.step.
tests/test_solver_cases_host.py checks on the CPU that the restatement alone meets every condition asserted on the inputs
here, measures the ulp sensitivities and checks that the restatement without the single-precision roundings is at least
100 x the bounds away.

Cases (solver_cases.FORMS; rectangles of fep.rect_mesh, the bottom row fixed vertically and the left column horizontally: a
row fixed in both directions would leave one isolated node per fixed node on every level, fep_aggregate_host makes each an
aggregate of its own and the coarsest level would pass the 256 DOFs of the refresh):
  P1-511x513  262 143 nodes   the control: one node below the threshold, the one-pass form on the same kind of hierarchy
  P1-512x512  262 144 nodes   exactly the threshold, every workgroup full
  P1-517x508  262 636 nodes = 2051 * 128 + 108: the last workgroup's wave 3 holds 12 nodes (pass 0 full, pass 1 half)
  P2-256      263 169 nodes = 2056 * 128 + 1: 9 and 19 blocks per node (two and three trips of the 8-lane loop per pass),
              one node in the last workgroup

Bounds: the rule of test_solver_shapes_gpu.py.  A case's bound is the larger of ITER_TOL / RELRES_TOL and 30 x the case's ulp
sensitivity (solver_cases.bound), never above 1e-9.

Per case: nodes per level | ulp sensitivity on the CPU | bounds used (x_k, relres_k) | worst values measured on the MI355X
(x_k, relres_k):
  P1-511x513  262143, 262143, 29242, 2431, 157, 12   9.6e-13   2.9e-11 2.9e-11   6.2e-12 1.3e-12
  P1-512x512  262144, 262144, 29242, 2491, 173, 13   1.1e-12   3.3e-11 3.3e-11   2.6e-12 8.4e-13
  P1-517x508  262636, 262636, 29410, 2441, 158, 13   2.1e-12   6.3e-11 6.3e-11   9.2e-13 7.5e-13
  P2-256      263169, 263169, 16513, 703, 37         2.8e-12   8.4e-11 8.4e-11   5.0e-13 1.3e-13
(The sensitivities are a hundred times those of test_solver_shapes_gpu.py's meshes: a hundred times the nodes, and a V-cycle
that converges slowly on these matrices — relres_4 is 0.3 to 1.1.  The restatement without the single-precision roundings
is 7e-7 to 2e-6 away in x_k and 2e-7 to 7e-7 in relres_k.)  tail_kernel runs in the three P1 cases and not in P2-256 (703 nodes
on the last smoothed level).

Full solve (P1-517x508, K_elast, b = Q K x): 45 iterations on device and restatement, x against the restated iterate 8.4e-13
(sensitivity of that iterate 4.9e-13, bound 1.5e-11), against the known solution 1.2e-7.

Shown to fail (arithmetic of the forms changed in a scratch build, never an index or a guard):
  - node3_kernel, PASSES > 1 only: the fold of pass 3 reads pass 0's first accumulator.  The iterate test fails on P1-512x512,
    P1-517x508 and P2-256 (x_k 0.52, 0.53, 0.58 against bounds of 3.3e-11 to 8.4e-11; relres_k 2.2 to 3.2); the control
    P1-511x513 stays at 6.2e-12 and test_vcycle_gpu.py passes whole.
  - product_kernel<1> only: the last term of an entry times 1.000001.  The iterate test fails on all four cases, the control
    included (x_k 1.6e-6 to 2.7e-6, relres_k 4.9e-7 to 1.9e-6); test_vcycle_gpu.py passes whole: none of its hierarchies
    has a product of fewer than three terms per entry.
"""
import re

import numpy as np
import pytest

import amg_ref
import solver_cases as sc
from conftest import dp_materials, needs_ablation_build, relerr
from test_vcycle_gpu import ITER_TOL, K_ITERS, RELRES_TOL, _assert_errors, _iterate_errors, _rhs

pytestmark = pytest.mark.gpu

_CASES = {}
_PLAN_LINE = re.compile(r'(\d+) -> (\d+) DOFs \(A P: (\d+) entries, (\d+) terms; R \(A P\): (\d+), (\d+)\)')


def _case(fep, name):
    """The case's context, matrices ({'elastic': K_elast, 'plastic': the tangent at solver_cases.displacement}), free DOFs,
    coordinates, singleton hierarchy of K_elast, solver with that hierarchy pushed and the refresh on, and the restated
    V-cycle of either matrix; cached (a solve leaves no state behind that the next one reads: the full solve asserts a
    bit-identical repeat)."""
    if name not in _CASES:
        elem, coord, et = sc.mesh(name)
        assert coord.shape[1] == sc.FORMS[name]['n_nodes']
        ctx = fep.MeshContext(elem, coord, element_type=et)
        ctx.set_materials(*dp_materials(ctx.n_int))
        K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
        r = ctx.step(sc.displacement(name), np.zeros((4, ctx.n_int)), want=('K',))
        assert 0 < r['n_smooth'] + r['n_apex'] < ctx.n_int
        qf = sc.free_dofs(name)
        Ks = {'elastic': K_el, 'plastic': r['K']}
        levels = amg_ref.singleton_hierarchy(K_el, qf, coord, coarse_nodes=sc.FORMS_COARSE_NODES)
        sol = fep.KrylovSolver(ctx, qf)
        amg_ref.push_hierarchy(sol, levels)
        _CASES[name] = dict(ctx=ctx, Ks=Ks, qf=qf, coord=coord, levels=levels, sol=sol,
                            M={mat: amg_ref.VCycle(K, qf, levels) for mat, K in Ks.items()})
    return _CASES[name]


@pytest.fixture(scope='module', autouse=True)
def _close_everything():
    yield
    for c in _CASES.values():
        c['sol'].close()
        c['ctx'].close()
    _CASES.clear()


def _worst(errs):
    return max(e[1] for e in errs), max(e[2] for e in errs)


@pytest.mark.parametrize('name', list(sc.FORMS))
def test_level_one_takes_the_listed_form(fep, name):
    """Level 1 has the mesh's node count and takes the four-pass form exactly where the table says; no lower level does;
    tail_kernel runs where the two last levels turn out small enough for it."""
    f = sc.FORMS[name]
    c = _case(fep, name)
    sol, levels = c['sol'], c['levels']
    assert sol.amg_refresh is True and sol.amg_hierarchy is levels
    nodes = (sol.amg_levels[0][0] // 2,) + tuple(n // 3 for n, _ in sol.amg_levels[1:])
    print('\n[measured] %s nodes per level %s' % (name, nodes))
    assert nodes[0] == nodes[1] == f['n_nodes'] and len(nodes) >= 4
    assert amg_ref.node3_four_pass(sol.amg_levels) == [f['four_pass']] + [False] * (len(nodes) - 3)
    assert (nodes[1] >= 128 * 2048) is f['four_pass'] and max(nodes[2:]) < 128 * 2048
    assert 3 * nodes[-1] <= 256                                               # the refresh's dense inverse takes it
    small = nodes[-2] <= amg_ref.TAIL_NODES and 3 * nodes[-1] <= amg_ref.TAIL_COARSE
    assert amg_ref.tail_runs(sol.amg_levels, refresh=True) is small, nodes
    # the shapes the cases are in the table for
    deg = sc.row_blocks(name)
    if name == 'P1-517x508':
        assert nodes[1] % 128 == 108 and nodes[1] // 128 == 2051
    if name == 'P2-256':
        assert nodes[1] % 128 == 1 and deg.max() == 19 and np.isin([9, 19], deg).all()
    if name == 'P1-512x512':
        assert nodes[1] % 128 == 0 and deg.max() == 7


@pytest.mark.parametrize('name', list(sc.FORMS))
def test_multigrid_iterates_match_the_float64_restatement(fep, name):
    """x_1 .. x_4 and relres_1 .. relres_4 of fep_solver_amg_pcg_dev on K_elast and on the plastic tangent, three right-hand
    sides, against amg_ref.VCycle with the refresh.  Every solve refreshes, so product_kernel<1>'s operators are in every
    iterate; level 1's four smoothing passes and its residual are node3_kernel's form of the case."""
    f = sc.FORMS[name]
    c = _case(fep, name)
    errs = []
    for mat, K in c['Ks'].items():
        errs += [((mat,) + lab, ex, er) for lab, ex, er in _iterate_errors(c['sol'], K, c['qf'], c['M'][mat], amg_ref.pcg, 'amg')]
    x_tol, r_tol = sc.bound(ITER_TOL, f['sens_vcycle']), sc.bound(RELRES_TOL, f['sens_vcycle'])
    print('\n[measured] %s multigrid x_k %.2e (bound %.1e) relres_k %.2e (bound %.1e)' % ((name,) + sum(zip(_worst(errs), (x_tol, r_tol)), ())))
    _assert_errors(errs, name, x_tol, r_tol)


def test_full_solve_matches_the_restated_pcg(fep):
    """P1-517x508 to rtol = 1e-10: on K_elast with b = Q K x for a random x (45 iterations; the plastic tangent takes 300,
    a minute of the restatement on the CPU).  The device's iteration count is the restatement's, its solution the
    restatement's iterate of that count to the case's bound (30 x the sensitivity of that iterate, solver_cases.bound on
    1e-12, the bound of the other full-solve tests), a repeat is bit-identical, and x is the known solution to 1e-5
    (relres 1e-10 x a condition number of 1e5, as test_vcycle_gpu's full solves)."""
    name = sc.FORMS_FULL_SOLVE
    c = _case(fep, name)
    K, qf, sol = c['Ks']['elastic'], c['qf'], c['sol']
    known, b = sc.forms_full_solve_rhs(K, qf)
    x = sol.solve_host(K, b, rtol=1e-10)
    it, rr = sol.last['iters'], sol.last['relres']
    assert sol.last['state'] == 1 and it > K_ITERS
    assert np.array_equal(x, sol.solve_host(K, b, rtol=1e-10)) and (sol.last['state'], sol.last['iters'], sol.last['relres']) == (1, it, rr)
    assert np.all(x[~qf] == 0.0)
    ref = amg_ref.pcg(K, qf, b, c['M']['elastic'], max_iter=it + 1, rtol=1e-10, keep=True)
    tol = sc.bound(1e-12, sc.FORMS[name]['sens_full'])
    print('\n[measured] %s full solve: iterations %d (restatement %d), x against the restated iterate %.2e (bound %.1e), against '
          'the known solution %.2e' % (name, it, ref['iters'], relerr(x, ref['history'][min(it, len(ref['history'])) - 1][0]), tol,
                                       relerr(x, known)))
    assert ref['state'] == 1 and it == ref['iters'], (sol.last, ref['iters'])
    assert relerr(x, ref['history'][it - 1][0]) <= tol
    assert relerr(x, known) <= 1e-5


def test_first_transfer_products_run_one_lane_per_entry(fep, monkeypatch, capfd):
    """P1-512x512: the plans fep_solver_amg_enable_refresh reports (FEP_VERBOSE) give product_kernel<1> for both products of
    transfer 0 and the 4- or 8-lane form below.  Mean terms per entry measured on the MI355X:
      transfer          0      1      2      3      4
      A P            1.00   7.96  16.48  19.99  22.64     lanes 1 4 8 8 8
      R (A P)        0.44  20.35  44.20  51.75  34.40     lanes 1 8 8 8 8
    (0.44: the entries count the padding to whole 3x3 node blocks, the rotation's rows and columns among it)
    What product_kernel<1> computes is checked by test_multigrid_iterates_match_the_float64_restatement."""
    c = _case(fep, 'P1-512x512')
    sol = fep.KrylovSolver(c['ctx'], c['qf'])
    monkeypatch.setenv('FEP_VERBOSE', '1')
    capfd.readouterr()
    amg_ref.push_hierarchy(sol, c['levels'])
    err = capfd.readouterr().err
    monkeypatch.delenv('FEP_VERBOSE')
    sol.close()
    line = [l for l in err.splitlines() if 'multigrid refresh plans' in l]
    assert len(line) == 1, err
    plans = [tuple(int(v) for v in m) for m in _PLAN_LINE.findall(line[0])]
    assert [(p[0], p[1]) for p in plans] == [(lv['P'].shape[0], lv['P'].shape[1]) for lv in c['levels']], line[0]
    lanes = [(amg_ref.product_lanes(p[3], p[2]), amg_ref.product_lanes(p[5], p[4])) for p in plans]
    print('\n[measured] mean terms per entry (A P, R (A P)) per transfer: %s; lanes %s'
          % (', '.join('%.2f %.2f' % (p[3] / p[2], p[5] / p[4]) for p in plans), lanes))
    assert lanes[0] == (1, 1)
    assert all(l in (4, 8) for pair in lanes[1:] for l in pair), lanes
    # at most one term per entry on transfer 0: every entry of K times the single entry of a row of P_0
    assert plans[0][3] <= plans[0][2] and plans[0][5] <= plans[0][4]


def test_plans_listed_on_the_device_are_the_host_plans(fep, monkeypatch, capfd):
    """The control case with FEP_AMG_PLAN=host (a switch of the -DFEP_ABLATION build, as in test_solver_gpu.py) against the
    default builder: the same terms in the same order, so x_4 is bit for bit the same."""
    needs_ablation_build(fep)
    c = _case(fep, 'P1-511x513')
    b = _rhs(c['qf'])['random']
    out = {}
    for mode in ('device', 'host'):
        monkeypatch.setenv('FEP_AMG_PLAN', mode)
        monkeypatch.setenv('FEP_VERBOSE', '1')
        capfd.readouterr()
        sol = fep.KrylovSolver(c['ctx'], c['qf'])
        amg_ref.push_hierarchy(sol, c['levels'])
        assert 'multigrid refresh plans (%s)' % mode in capfd.readouterr().err
        out[mode] = [(sol.solve_host(K, b, rtol=1e-14, max_iter=K_ITERS), sol.last['relres']) for K in c['Ks'].values()]
        sol.close()
    for (xd, rd), (xh, rh) in zip(out['device'], out['host']):
        assert rd == rh and np.array_equal(xd, xh)

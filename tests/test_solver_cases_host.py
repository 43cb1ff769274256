"""
The cases of tests/solver_cases.py on the host: the float64 restatement alone (tests/amg_ref.py), on K_elast and the plastic
tangent of the oracle, stays inside every condition test_solver_shapes_gpu.py puts on its inputs — the hierarchy has the
recorded shape, the restated V-cycle is symmetric positive definite, the restated CG runs its four iterates without
breakdown and converges, the tangent has plastic points — and the ulp sensitivity recorded in the case table (from which
the GPU test derives its bounds) is the one measured here.  The same for the cases of test_solver_forms_gpu.py
(solver_cases.FORMS, under amg_ref.singleton_hierarchy), with the distance of the restatement without single precision.  No GPU.
"""
import numpy as np
import pytest

import amg_ref
import solver_cases as sc
from conftest import relerr
from test_vcycle_gpu import ITER_TOL, K_ITERS, RELRES_TOL, _rhs


# The GPU test's solves stop at relres <= 1e-14 and compare relres_k relatively: the restated relres_1 .. relres_4 stay far above
# that (a 4-node mesh can exhaust its Krylov space within four iterates: solver_cases.free_dofs, the small rectangles)
STILL_ITERATING = 1e-6


def _sensitivity(Ks, qf, make_M, cg):
    return max(sc.ulp_sensitivity(K, qf, make_M, cg) for K in Ks.values())


def _same_figure(measured, recorded):
    """The sensitivity is an amplitude of rounding noise: another BLAS or SciPy moves it, not by a factor of two."""
    return 0.5 * recorded <= measured <= 2.0 * recorded


def _jacobi_conditions(name, Ks, qf):
    for mat, K in Ks.items():
        M = amg_ref.block_jacobi(K, qf)
        for rhs, b in _rhs(qf).items():
            out = amg_ref.pcg_single_reduction(K, qf, b, M, max_iter=K_ITERS, keep=True)
            assert out['state'] == 0 and len(out['history']) == K_ITERS, (name, mat, rhs)
            assert min(rr for _, rr in out['history']) > STILL_ITERATING, (name, mat, rhs)
    sj = _sensitivity(Ks, qf, lambda K: amg_ref.block_jacobi(K, qf), amg_ref.pcg_single_reduction)
    assert _same_figure(sj, sc.ALL[name]['sens_jacobi']), (name, sj)


@pytest.mark.parametrize('name', list(sc.CASES))
def test_reference_alone_meets_every_condition(fep, name):
    c = sc.CASES[name]
    qf = sc.free_dofs(name)
    Ks, (n_smooth, n_apex, n_int) = sc.oracle_matrices(name)
    assert 0 < n_smooth + n_apex < n_int
    assert not qf.reshape(-1, 2)[sc.orphan_nodes(name)].any()
    levels = sc.hierarchy(name, Ks['elastic'])
    assert sc.level_nodes(levels, qf.size) == c['nodes']
    assert amg_ref.tail_runs(sc.level_sizes(Ks['elastic'], levels), refresh=c['refresh']) is c['tail']
    # the form the device falls back to: no refresh where the coarsest level is beyond dense_inverse_kernel's 256 DOFs
    assert c['refresh'] is (levels[-1]['size'][0] <= 256)
    rng = np.random.default_rng(5)
    for mat, K in Ks.items():
        M = amg_ref.VCycle(K, qf, levels, refresh=c['refresh'])
        b1, b2 = np.where(qf, rng.normal(size=(2, qf.size)), 0.0)
        z1, z2 = M(b1), M(b2)
        assert np.all(z1[~qf] == 0.0) and np.all(z2[~qf] == 0.0)
        assert abs(b1 @ z2 - b2 @ z1) <= 1e-12 * np.sqrt((b1 @ z1) * (b2 @ z2)), (name, mat)      # test_amg_ref.py's bound
        assert b1 @ z1 > 0.0 and b2 @ z2 > 0.0
        for rhs, b in _rhs(qf).items():
            out = amg_ref.pcg(K, qf, b, M, max_iter=K_ITERS, keep=True)
            assert out['state'] == 0 and len(out['history']) == K_ITERS, (name, mat, rhs)
            assert min(rr for _, rr in out['history']) > STILL_ITERATING, (name, mat, rhs)
        if mat == 'plastic':
            out = amg_ref.pcg(K, qf, _rhs(qf)['random'], M, max_iter=2000, rtol=1e-10)
            assert out['state'] == 1 and out['relres'] <= 1e-10 and out['iters'] > K_ITERS, (name, out['iters'])
    sv = _sensitivity(Ks, qf, lambda K: amg_ref.VCycle(K, qf, levels, refresh=c['refresh']), amg_ref.pcg)
    assert _same_figure(sv, c['sens_vcycle']), (name, sv)
    _jacobi_conditions(name, Ks, qf)


@pytest.mark.parametrize('name', list(sc.SMALL))
def test_small_rectangles_meet_the_block_jacobi_conditions(fep, name):
    """128, 129 and 4 nodes: block Jacobi and spmv only."""
    elem, coord, _ = sc.mesh(name)
    assert coord.shape[1] == sc.SMALL[name]['n_nodes']
    qf = sc.free_dofs(name)
    Ks, (n_smooth, n_apex, n_int) = sc.oracle_matrices(name)
    assert 0 < n_smooth + n_apex
    assert int(qf.sum()) > K_ITERS                           # four distinct iterates exist
    _jacobi_conditions(name, Ks, qf)


def test_case_table_covers_the_shapes_it_is_there_for():
    """What each case is in the table for, from the table and the meshes alone."""
    deg = {name: sc.row_blocks(name) for name in sc.CASES}
    assert deg['fan250-P1'].max() == 251 and deg['fan84-P2'].max() == 253 and deg['fan24-P4'].max() == 241
    assert (deg['tsx-P4'].min(), deg['tsx-P4'].max()) == (15, 81)
    assert (deg['orphans-P1'] == 0).sum() == sc.orphan_nodes('orphans-P1').size > 0
    nodes = {name: c['nodes'] for name, c in sc.CASES.items()}
    assert len(nodes['delaunay8-P4']) == 2 and len(nodes['delaunay72-P1']) == 4
    assert 256 < nodes['delaunay50-P1'][1] <= amg_ref.TAIL_NODES and 256 < nodes['delaunay58-P1'][1] <= amg_ref.TAIL_NODES
    assert nodes['delaunay50-P1'][1] % 8 and nodes['delaunay58-P1'][1] % 8
    assert nodes['delaunay62-P1'][1] == amg_ref.TAIL_NODES + 8 and 3 * nodes['delaunay62-P1'][2] <= amg_ref.TAIL_COARSE
    for name in ('fan250-P1', 'fan84-P2', 'fan24-P4'):
        assert 3 * nodes[name][-1] > 256 and not sc.CASES[name]['refresh']
    assert set(sc.FULL_SOLVES) <= set(sc.CASES)


def test_bound_rule():
    """The larger of the squares' bound and 30 x the sensitivity, capped at 1e-9."""
    assert abs(sc.bound(5e-12, 2.0e-13) - 6.0e-12) <= 1e-24 and sc.bound(5e-12, 1e-15) == 5e-12 and sc.bound(5e-12, 1.0) == 1e-9


def _histories(K, qf, M):
    out = {}
    for rhs, b in _rhs(qf).items():
        res = amg_ref.pcg(K, qf, b, M, max_iter=K_ITERS, keep=True)
        assert res['state'] == 0 and len(res['history']) == K_ITERS, rhs
        assert min(rr for _, rr in res['history']) > STILL_ITERATING, rhs
        out[rhs] = res['history']
    return out


@pytest.mark.parametrize('name', list(sc.FORMS))
def test_forms_reference_alone_meets_every_condition(fep, name):
    """The cases of test_solver_forms_gpu.py: the mesh has the listed node count, the tangent plastic points, the singleton
    hierarchy the listed levels (level 1 the mesh's nodes, the four-pass form there and only there where listed, a coarsest
    level the refresh takes), the restated CG runs its four iterates on both matrices, the ulp sensitivity is the recorded
    one, and the restatement WITHOUT the single-precision roundings is at least 100 x the derived bounds away in x_k and in
    relres_k (largest difference over the iterates, as the bound is applied): a device that kept double precision where
    the product rounds, or rounded elsewhere, would not pass for the product."""
    c = sc.FORMS[name]
    elem, coord, _ = sc.mesh(name)
    assert coord.shape[1] == c['n_nodes']
    qf = sc.free_dofs(name)
    Ks, (n_smooth, n_apex, n_int) = sc.oracle_matrices(name)
    assert 0 < n_smooth + n_apex < n_int
    levels = amg_ref.singleton_hierarchy(Ks['elastic'], qf, coord, coarse_nodes=sc.FORMS_COARSE_NODES)
    sizes = sc.level_sizes(Ks['elastic'], levels)
    assert sc.level_nodes(levels, qf.size) == c['nodes'] and c['nodes'][1] == c['n_nodes']
    assert amg_ref.node3_four_pass(sizes) == [c['four_pass']] + [False] * (len(levels) - 2)
    assert amg_ref.tail_runs(sizes, refresh=True) is c['tail']
    assert levels[-1]['size'][0] <= 256                                       # no FEP_ERANGE from the refresh
    assert all(np.all(np.diff(lv['D'].indptr) == 3) for lv in levels[:-1])    # nor FEP_EINVAL from build_refresh
    x_tol, r_tol = sc.bound(ITER_TOL, c['sens_vcycle']), sc.bound(RELRES_TOL, c['sens_vcycle'])
    far_x, far_r, sens = 0.0, 0.0, 0.0
    for mat, K in Ks.items():
        h = _histories(K, qf, amg_ref.VCycle(K, qf, levels))
        h64 = _histories(K, qf, amg_ref.VCycle(K, qf, levels, fp32=False, fp32_transfers=False))
        far_x = max([far_x] + [relerr(a[0], b[0]) for rhs in h for a, b in zip(h64[rhs], h[rhs])])
        far_r = max([far_r] + [abs(a[1] - b[1]) / b[1] for rhs in h for a, b in zip(h64[rhs], h[rhs])])
        sens = max(sens, sc.ulp_sensitivity(K, qf, lambda K: amg_ref.VCycle(K, qf, levels), amg_ref.pcg))
    print('\n[measured] %s nodes %s ulp sensitivity %.2e, bounds x_k %.1e relres_k %.1e, without single precision x_k %.2e relres_k %.2e'
          % (name, c['nodes'], sens, x_tol, r_tol, far_x, far_r))
    assert _same_figure(sens, c['sens_vcycle']), (name, sens)
    assert x_tol <= 1e-9 and far_x >= 100.0 * x_tol and far_r >= 100.0 * r_tol, (name, far_x, far_r)
    if name == sc.FORMS_FULL_SOLVE:
        K = Ks['elastic']
        known, b = sc.forms_full_solve_rhs(K, qf)
        Kp = sc.perturbed(K)
        out = amg_ref.pcg(K, qf, b, amg_ref.VCycle(K, qf, levels), max_iter=2000, rtol=1e-10, keep=True)
        outp = amg_ref.pcg(Kp, qf, b, amg_ref.VCycle(Kp, qf, levels), max_iter=out['iters'], rtol=0.0, keep=True)
        assert out['state'] == 1 and out['relres'] <= 1e-10 and out['iters'] > K_ITERS and relerr(out['x'], known) <= 1e-5
        sf = relerr(outp['history'][out['iters'] - 1][0], out['x'])
        print('[measured] %s full solve: %d iterations, sensitivity of the last iterate %.2e' % (name, out['iters'], sf))
        assert _same_figure(sf, c['sens_full']), sf


def test_forms_table_covers_the_shapes_it_is_there_for():
    n = amg_ref.FOUR_PASS_NODES
    nodes = {name: c['n_nodes'] for name, c in sc.FORMS.items()}
    assert nodes == {'P1-511x513': n - 1, 'P1-512x512': n, 'P1-517x508': 2051 * 128 + 108, 'P2-256': 2056 * 128 + 1}
    assert [c['four_pass'] for c in sc.FORMS.values()] == [False, True, True, True]
    # the last workgroup of P1-517x508: waves 0 .. 2 full (96 nodes), wave 3 holds 12: lane groups 0 .. 7 in pass 0, 0 .. 3 in pass 1
    assert nodes['P1-517x508'] % 128 - 3 * 32 == 12
    deg = sc.row_blocks('P2-256')
    assert deg.max() == 19 and np.isin([9, 19], deg).all() and sc.row_blocks('P1-512x512').max() == 7
    assert sc.FORMS_FULL_SOLVE in sc.FORMS

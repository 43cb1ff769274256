"""
The float64 restatement of the GPU preconditioners and CG forms (tests/amg_ref.py) checked on its own, on the host: the
V-cycle it restates is a symmetric positive definite operator, its conjugate gradients reach SuperLU's solution, and with
single precision and the refresh off it is the older, independent restatement of tools/deflation_study_lib.py.
Matrices: K_elast of the oracle's elastic set-up on the footing's square meshes, hierarchies from build_amg_hierarchy, and
from amg_ref.singleton_hierarchy (the hierarchy of test_solver_forms_gpu.py) with the two dispatch rules restated next to it.
"""
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import scipy.sparse.linalg as sspl

import amg_ref
from conftest import ROOT, dp_materials, relerr


def _elastic(fep, et, n):
    from oracle import fep_oracle as orc
    mesh = fep.square_mesh(n, et, 10)
    d1, d2, wf = fep.element_tables(et)
    n_int = mesh['elements'].shape[1] * np.size(wf)
    shear, bulk, _, _ = dp_materials(n_int)
    K = orc.elastic_setup(mesh['elements'], mesh['coordinates'], shear, bulk, d1, d2, wf)[0]
    K = ssp.csr_matrix(K)
    K.sort_indices()
    return mesh, K, mesh['Q'].flatten(order='F')


def _hierarchy(K, mesh, qf, coarse_nodes=30):
    return amg_ref.solver.build_amg_hierarchy(K, qf, mesh['coordinates'], coarse_nodes=coarse_nodes)


def _deflation_study_lib():
    spec = importlib.util.spec_from_file_location('deflation_study_lib', os.path.join(ROOT, 'tools', 'deflation_study_lib.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('et,n', [('P1', 24), ('Q2', 12)])
@pytest.mark.parametrize('refresh,fp32', [(True, True), (False, True), (False, False)])
def test_restated_vcycle_is_symmetric_positive_definite(fep, et, n, refresh, fp32):
    mesh, K, qf = _elastic(fep, et, n)
    levels = _hierarchy(K, mesh, qf)
    assert len(levels) >= 2
    M = amg_ref.VCycle(K, qf, levels, refresh=refresh, fp32=fp32, fp32_transfers=fp32)
    rng = np.random.default_rng(5)
    b1, b2 = rng.normal(size=(2, K.shape[0]))
    z1, z2 = M(b1), M(b2)
    assert np.all(z1[~qf] == 0.0) and np.all(z2[~qf] == 0.0)
    # constrained entries of b are ignored
    assert np.array_equal(M(np.where(qf, b1, 0.0)), z1)
    b1q, b2q = np.where(qf, b1, 0.0), np.where(qf, b2, 0.0)
    s12, s21 = b1q @ z2, b2q @ z1
    # symmetric up to the rounding of double arithmetic on symmetric operands: measured <= 3e-16, bound 1e-12
    assert abs(s12 - s21) <= 1e-12 * np.sqrt((b1q @ z1) * (b2q @ z2))
    assert b1q @ z1 > 0.0 and b2q @ z2 > 0.0


@pytest.mark.parametrize('et,n', [('P1', 24), ('P2', 8)])
def test_restated_pcg_reaches_the_sparse_direct_solution(fep, et, n):
    mesh, K, qf = _elastic(fep, et, n)
    levels = _hierarchy(K, mesh, qf)
    b = np.random.default_rng(2).normal(size=K.shape[0])
    ref = np.zeros(K.shape[0])
    ref[qf] = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
    for M, cg in ((amg_ref.VCycle(K, qf, levels), amg_ref.pcg), (amg_ref.block_jacobi(K, qf), amg_ref.pcg_single_reduction)):
        out = cg(K, qf, b, M, max_iter=5000, rtol=1e-12)
        assert out['state'] == 1 and out['relres'] <= 1e-12 and 0 < out['iters'] < 5000
        assert np.all(out['x'][~qf] == 0.0)
        assert relerr(out['x'], ref) <= 1e-8              # condition number ~1e5: as test_pcg_matches_sparse_direct
    # both CG forms are the same iteration: their first iterates agree to rounding
    Mj = amg_ref.block_jacobi(K, qf)
    a = amg_ref.pcg(K, qf, b, Mj, max_iter=6, keep=True)['history']
    c = amg_ref.pcg_single_reduction(K, qf, b, Mj, max_iter=6, keep=True)['history']
    for (xa, ra), (xc, rc) in zip(a, c):
        assert relerr(xc, xa) <= 1e-13 and abs(rc - ra) <= 1e-13 * ra      # measured <= 1.7e-15: rounding only


@pytest.mark.parametrize('et,n', [('P1', 24), ('Q1', 12)])
def test_restated_vcycle_is_the_deflation_study_vcycle(fep, et, n):
    """No single precision, no refresh, symmetric K: the V-cycle of tools/deflation_study_lib (an older restatement whose
    level 0 inverts the 2x2 blocks of the masked operator with solver._block_diag_inverse — the same blocks when K is
    symmetric, up to its 1e-13 diagonal shift)."""
    mesh, K, qf = _elastic(fep, et, n)
    K = ((K + K.T) * 0.5).tocsr()
    K.sort_indices()
    levels = _hierarchy(K, mesh, qf)
    ds = _deflation_study_lib()
    A0 = amg_ref.solver._masked_operator(K, qf.astype(np.float64))
    old = ds.VCycle(A0, levels)
    new = amg_ref.VCycle(K, qf, levels, refresh=False, fp32=False, fp32_transfers=False)
    rng = np.random.default_rng(11)
    for _ in range(3):
        b = np.where(qf, rng.normal(size=K.shape[0]), 0.0)
        # measured <= 3.9e-14: the 1e-13 |trace| shift of _block_diag_inverse on level 0 (the fp32 rounding alone is ~1e-7)
        assert relerr(new(b), old(b)) <= 1e-13


# ---- the hand-made hierarchy of the size-dependent kernel forms (amg_ref.singleton_hierarchy, test_solver_forms_gpu.py) ----
_SINGLETON = {}


def _singleton(fep, et, n):
    if (et, n) not in _SINGLETON:
        mesh, K, qf = _elastic(fep, et, n)
        _SINGLETON[et, n] = (mesh, K, qf, amg_ref.singleton_hierarchy(K, qf, mesh['coordinates'], coarse_nodes=30))
    return _SINGLETON[et, n]


@pytest.mark.parametrize('et,n', [('P1', 36), ('P2', 30)])
def test_singleton_hierarchy_has_the_mesh_as_level_one(fep, et, n):
    """Level 1 has one node per mesh node, P_0 is the identity on free DOFs and nothing else, A_1 is K on the free DOFs with
    every rotation row and column empty, and the lists are what fep_solver_amg_push_level and build_refresh take."""
    mesh, K, qf, levels = _singleton(fep, et, n)
    n_n = K.shape[0] // 2
    assert len(levels) >= 3 and [lv['last'] for lv in levels] == [False] * (len(levels) - 1) + [True]
    lv = levels[0]
    P, R, A, D = lv['P'], lv['R'], lv['A'], lv['D']
    assert P.shape == (2 * n_n, 3 * n_n) and lv['size'] == (3 * n_n, A.nnz) and A.shape == (3 * n_n, 3 * n_n)
    per_row = np.diff(P.indptr)
    assert per_row.max() == 1 and np.array_equal(per_row == 1, qf)             # none on constrained rows
    rows = np.flatnonzero(qf)
    assert np.array_equal(P.indices, 3 * (rows // 2) + rows % 2) and np.all(P.data == 1.0)
    assert (R != P.T).nnz == 0
    # A_1 = K on the free DOFs, the node's third DOF (the rotation) untouched
    keep = np.arange(3 * n_n) % 3 < 2
    A = ssp.csr_matrix(A)
    assert np.diff(A.indptr)[~keep].max() == 0 and np.diff(A.tocsc().indptr)[~keep].max() == 0
    Kq = ssp.diags(qf.astype(float)) @ K @ ssp.diags(qf.astype(float))
    assert abs(A[keep][:, keep] - Kq).max() == 0.0
    # D: three stored entries per row in ascending columns; a rotation's diagonal is 1 (up to _block_diag_inverse's
    # 1e-13 |trace| / 3 shift) and it is coupled to nothing
    for l in levels[:-1]:
        assert np.all(np.diff(l['D'].indptr) == 3) and l['D'].has_sorted_indices
        assert np.all(np.diff(l['D'].indices.reshape(-1, 3), axis=1) == 1)
    Db = amg_ref.solver._block_diag(ssp.csr_matrix(D), 3)
    Ab = amg_ref.solver._block_diag(A, 3)
    eps = 1e-13 * np.abs(np.where(Ab[:, 0, 0] == 0, 1.0, Ab[:, 0, 0]) + np.where(Ab[:, 1, 1] == 0, 1.0, Ab[:, 1, 1]) + 1.0) / 3.0
    assert np.all(Db[:, 2, :2] == 0.0) and np.all(Db[:, :2, 2] == 0.0)
    assert np.abs(Db[:, 2, 2] * (1.0 + eps) - 1.0).max() <= 4 * 2.0 ** -53
    assert np.abs(Db[:, 2, 2] - 1.0).max() <= 1e-13 * np.abs(K.diagonal()).max()
    # below the first transfer: ordinary smoothed aggregation (more than one entry per row, fewer nodes)
    assert levels[1]['P'].shape[0] == 3 * n_n and levels[1]['P'].shape[1] < n_n and np.diff(levels[1]['P'].indptr).max() > 1
    assert levels[-1]['size'][0] <= 3 * 30 and levels[-1]['D'] is None
    assert all(l['omega'] > 0.0 for l in levels)


@pytest.mark.parametrize('et,n', [('P1', 36), ('P2', 30)])
def test_singleton_vcycle_is_symmetric_positive_definite_and_its_cg_converges(fep, et, n):
    """The bound of test_restated_vcycle_is_symmetric_positive_definite; the restated CG with it reaches SuperLU's solution."""
    mesh, K, qf, levels = _singleton(fep, et, n)
    M = amg_ref.VCycle(K, qf, levels)
    rng = np.random.default_rng(5)
    b1, b2 = rng.normal(size=(2, K.shape[0]))
    z1, z2 = M(b1), M(b2)
    assert np.all(z1[~qf] == 0.0) and np.all(z2[~qf] == 0.0)
    b1q, b2q = np.where(qf, b1, 0.0), np.where(qf, b2, 0.0)
    assert abs(b1q @ z2 - b2q @ z1) <= 1e-12 * np.sqrt((b1q @ z1) * (b2q @ z2))
    assert b1q @ z1 > 0.0 and b2q @ z2 > 0.0
    b = np.random.default_rng(2).normal(size=K.shape[0])
    ref = np.zeros(K.shape[0])
    ref[qf] = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
    out = amg_ref.pcg(K, qf, b, M, max_iter=5000, rtol=1e-12)
    assert out['state'] == 1 and out['relres'] <= 1e-12 and 0 < out['iters'] < 5000
    assert relerr(out['x'], ref) <= 1e-8


def test_dispatch_rules_on_both_sides_of_each_threshold():
    """node3_four_pass restates vcycle_chebyshev's `big` (128 * 2048 nodes), product_lanes product_apply's choice."""
    n = 128 * 2048
    assert amg_ref.FOUR_PASS_NODES == 262144
    sizes = lambda *nodes: [(2 * nodes[0], 0)] + [(3 * m, 0) for m in nodes[1:]]
    assert amg_ref.node3_four_pass(sizes(n, n, 100, 10)) == [True, False]
    assert amg_ref.node3_four_pass(sizes(n, n - 1, 100, 10)) == [False, False]
    assert amg_ref.node3_four_pass(sizes(4 * n, n + 1, n, n - 1, 10)) == [True, True, False]
    assert amg_ref.node3_four_pass(sizes(n, 10)) == []                         # one transfer: no smoothed coarse level
    assert amg_ref.node3_four_pass([(2 * n, 0), (3 * n - 1, 0), (30, 0)]) == [False]      # whole nodes, as n_coarse / 3
    assert amg_ref.product_lanes(12 * 1000, 1000) == 8 and amg_ref.product_lanes(12 * 1000 - 1, 1000) == 4
    assert amg_ref.product_lanes(3 * 1000, 1000) == 4 and amg_ref.product_lanes(3 * 1000 - 1, 1000) == 1
    assert amg_ref.product_lanes(1, 1000) == 1 and amg_ref.product_lanes(0, 1000) == 1
    assert amg_ref.product_lanes(0, 0) == 0 and amg_ref.product_lanes(10 ** 9, 1) == 8

"""
The float64 restatement of the GPU preconditioners and CG forms (tests/amg_ref.py) checked on its own, on the host: the
V-cycle it restates is a symmetric positive definite operator, its conjugate gradients reach SuperLU's solution, and with
single precision and the refresh off it is the older, independent restatement of tools/deflation_study_lib.py.
Matrices: K_elast of the oracle's elastic set-up on the footing's square meshes, hierarchies from build_amg_hierarchy.
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

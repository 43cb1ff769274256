"""
Float64 restatement of the GPU solver's preconditioners and of both conjugate-gradient forms
(fem-elastoplasticity_amd/csrc/fep_solver.hip), for the tests that compare the device's iterates with it
(test_vcycle_gpu.py) and the tests of the restatement itself (test_amg_ref.py).  Plain NumPy / SciPy, no GPU.

What the device computes, and what this module therefore does:
  - block_jacobi_kernel: the 2x2 node blocks of the DOUBLE K, constrained DOFs replaced by identity rows and columns, the
    off-diagonal symmetrised to (b + c) / 2, the identity where det <= 0 or a <= 0 (not solver._block_diag_inverse);
  - vcycle_chebyshev: degree-2 Chebyshev smoothing (cheb_coefficients(omega of the smoothed level, 20, 1.2)) before and
    after the coarse correction; level 0 is Q K Q through the free-DOF mask (residual and smoother output 0 on
    constrained DOFs);
  - all arithmetic in double on operands rounded to single precision where the device reads single precision: K in the
    four level-0 passes (`fp32`), the prolongator's values in both transfers (`fp32_transfers`: restriction = B^T of the
    same rounded blocks), the refreshed coarse operators in node3_kernel / tail_kernel (`fp32` with `refresh`);
    the block inverses, the coarsest inverse and CG's own product stay double;
  - refresh (the default): before every solve A_{k+1} = R_k A_k P_k from the solve's K in double, 3x3 block inverses as
    block3_inverse_kernel (zero diagonal -> 1, plus 1e-13 |trace| / 3), the coarsest operator inverted after adding
    1e-10 max|A| to its diagonal (dense_inverse_kernel); without it the pushed operators of the reference matrix;
  - conjugate gradients from x = 0 with r = Q b: the standard form of the multigrid solve (mg_* kernels) and the
    single-reduction form of Chronopoulos & Gear of the block-Jacobi solve (pcg_* kernels).
"""
import importlib

import numpy as np
import scipy.sparse as ssp

solver = importlib.import_module('fem-elastoplasticity_amd.solver')

TAIL_NODES, TAIL_COARSE = 384, 128           # kTailNodes / kTailCoarse of fep_solver.hip


def f32(a):
    """Values rounded to single precision (round to nearest), back in double."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def f32_csr(M):
    M = ssp.csr_matrix(M, copy=True)
    M.data = f32(M.data)
    return M


def cheb_coefficients(omega, alpha=20.0, safety=1.2):
    """(c1, a2, cp, w2) of the degree-2 Chebyshev smoother for D^-1 A on [lmax / alpha, lmax], lmax = safety * rho."""
    rho = 4.0 / (3.0 * 1.05 * omega)
    lmax = safety * rho
    lmin = lmax / alpha
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    r0 = 1.0 / sigma
    r1 = 1.0 / (2.0 * sigma - r0)
    return 1.0 / theta, 1.0 + r1 * r0, -r1 * r0, 2.0 * r1 / delta


def block_jacobi_2x2(K, free_dof):
    """(n_n, 3) = (m00, m01, m11) of block_jacobi_kernel's symmetric 2x2 inverse per node, from the double K."""
    K = ssp.csr_matrix(K)
    a = K.diagonal(0)[0::2].copy()
    d = K.diagonal(0)[1::2].copy()
    b = K.diagonal(1)[0::2].copy()              # K[2n, 2n + 1]
    c = K.diagonal(-1)[0::2].copy()             # K[2n + 1, 2n]
    f = np.asarray(free_dof, dtype=bool).ravel()
    f0, f1 = f[0::2], f[1::2]
    a[~f0] = 1.0
    d[~f1] = 1.0
    b[~(f0 & f1)] = 0.0
    c[~(f0 & f1)] = 0.0
    sym = 0.5 * (b + c)
    det = a * d - sym * sym
    bad = ~(det > 0.0) | ~(a > 0.0)
    a[bad], d[bad], det[bad], b[bad], c[bad], sym[bad] = 1.0, 1.0, 1.0, 0.0, 0.0, 0.0
    off = np.where((b == 0.0) & (c == 0.0), 0.0, -sym / det)
    return np.stack([d / det, off, a / det], axis=1)


def apply_2x2(minv, v):
    v = v.reshape(-1, 2)
    return np.stack([minv[:, 0] * v[:, 0] + minv[:, 1] * v[:, 1], minv[:, 1] * v[:, 0] + minv[:, 2] * v[:, 1]], axis=1).ravel()


def block3_inverse(A):
    """(n, 3, 3) inverses of the 3x3 diagonal blocks as block3_inverse_kernel forms them."""
    D = solver._block_diag(ssp.csr_matrix(A), 3)
    for i in range(3):
        z = D[:, i, i] == 0.0
        D[z, i, i] = 1.0
    eps = 1e-13 * np.abs(np.einsum('nii->n', D)) / 3.0
    return np.linalg.inv(D + eps[:, None, None] * np.eye(3)[None])


def apply_3x3(Dinv, v):
    return np.einsum('nij,nj->ni', Dinv, v.reshape(-1, 3)).ravel()


def coarsest_inverse(A):
    """dense_inverse_kernel: the inverse after 1e-10 of the largest entry is added to the diagonal."""
    dense = np.asarray(ssp.csr_matrix(A).toarray(), dtype=np.float64)
    dense += 1e-10 * np.abs(dense).max() * np.eye(dense.shape[0])
    return np.linalg.inv(dense)


def tail_runs(level_sizes, refresh=True, fp32=True, tail=True, block_transfers=True, smoother='chebyshev'):
    """Whether vcycle_chebyshev runs the last smoothed level and the coarsest solve in tail_kernel: its `kt` condition
    from `level_sizes` = KrylovSolver.amg_levels [(DOFs, nnz)] (level 0 = the mesh), with the refresh on (the node-block
    operators), a single-precision operator copy, block transfers on the last transfer, the last smoothed level at most
    kTailNodes nodes and the coarsest at most kTailCoarse DOFs, whole nodes.  (The block-Jacobi smoother's vcycle has
    no tail.)"""
    nl = len(level_sizes) - 1                    # transfers
    if not (smoother == 'chebyshev' and tail and refresh and fp32 and block_transfers and nl >= 2):
        return False
    n_last_smoothed, n_coarsest = level_sizes[-2][0], level_sizes[-1][0]
    return n_last_smoothed // 3 <= TAIL_NODES and n_coarsest <= TAIL_COARSE and n_coarsest % 3 == 0


class VCycle:
    """z = M b of fep_solver_amg_pcg_dev for the solve's matrix K (csr_matrix on the solver's pattern), the hierarchy
    `levels` (build_amg_hierarchy's dicts, as pushed) and the free-DOF mask.  smoother: 'chebyshev' (the product) or
    'jacobi' (two damped block-Jacobi sweeps, vcycle(); the coarse operators then stay double)."""

    def __init__(self, K, free_dof, levels, refresh=True, fp32=True, fp32_transfers=True, smoother='chebyshev',
                 cheb_alpha=20.0, cheb_safety=1.2):
        if smoother not in ('chebyshev', 'jacobi'):
            raise ValueError(smoother)
        K = ssp.csr_matrix(K)
        self.q = np.asarray(free_dof, dtype=bool).ravel().astype(np.float64)
        self.cheb = smoother == 'chebyshev'
        self.K0 = f32_csr(K) if fp32 else K
        self.minv = block_jacobi_2x2(K, free_dof)
        self.P = [f32_csr(lv['P']) if fp32_transfers else ssp.csr_matrix(lv['P']) for lv in levels]
        self.R = [P.T.tocsr() for P in self.P] if fp32_transfers else [ssp.csr_matrix(lv['R']) for lv in levels]
        self.omega = [lv['omega'] for lv in levels]
        self.ch = [cheb_coefficients(w, cheb_alpha, cheb_safety) for w in self.omega]
        self.nl = len(levels)
        # operators of levels 1 .. nl - 1 (index k - 1) and their block inverses; the coarsest level's inverse
        self.A, self.D = [], []
        if refresh:
            Ak = K
            for lv in levels:
                Ak = (ssp.csr_matrix(lv['R']) @ (Ak @ ssp.csr_matrix(lv['P']))).tocsr()
                if lv['last']:
                    self.Ainv = coarsest_inverse(Ak)
                else:
                    self.D.append(block3_inverse(Ak))
                    self.A.append(f32_csr(Ak) if fp32 and self.cheb else Ak)
        else:
            for lv in levels:
                if lv['last']:
                    self.Ainv = ssp.csr_matrix(lv['A']).toarray()
                else:
                    self.A.append(ssp.csr_matrix(lv['A']))
                    self.D.append(solver._block_diag(ssp.csr_matrix(lv['D']), 3))

    # level 0: Q K Q, residual and output 0 on constrained DOFs
    def _res0(self, b, x):
        return self.q * (b - self.K0 @ x)

    def _m0(self, v):
        return apply_2x2(self.minv, v)

    def _coarse(self, b, j):
        """level j >= 1: operator self.A[j - 1], transfer j -> j + 1 = self.P[j]"""
        if j == self.nl:
            return self.Ainv @ b
        A, D = self.A[j - 1], self.D[j - 1]
        if self.cheb:
            c1, a2, cp, w2 = self.ch[j]
            x1 = c1 * apply_3x3(D, b)
            x2 = a2 * x1 + w2 * apply_3x3(D, b - A @ x1)
            x0 = x2 + self.P[j] @ self._coarse(self.R[j] @ (b - A @ x2), j + 1)
            x1 = x0 + c1 * apply_3x3(D, b - A @ x0)
            return a2 * x1 + cp * x0 + w2 * apply_3x3(D, b - A @ x1)
        w = self.omega[j]
        x = w * apply_3x3(D, b)
        x = x + w * apply_3x3(D, b - A @ x)
        x = x + self.P[j] @ self._coarse(self.R[j] @ (b - A @ x), j + 1)
        for _ in range(2):
            x = x + w * apply_3x3(D, b - A @ x)
        return x

    def __call__(self, b):
        q = self.q
        b = np.asarray(b, dtype=np.float64)
        if self.cheb:
            c1, a2, cp, w2 = self.ch[0]
            x1 = c1 * self._m0(q * b)
            x2 = q * (a2 * x1 + w2 * self._m0(self._res0(b, x1)))
            x0 = x2 + self.P[0] @ self._coarse(self.R[0] @ self._res0(b, x2), 1)
            x1 = q * (x0 + c1 * self._m0(self._res0(b, x0)))
            return q * (a2 * x1 + cp * x0 + w2 * self._m0(self._res0(b, x1)))
        w = self.omega[0]
        x = w * self._m0(q * b)
        x = q * (x + w * self._m0(self._res0(b, x)))
        x = x + self.P[0] @ self._coarse(self.R[0] @ self._res0(b, x), 1)
        for _ in range(2):
            x = q * (x + w * self._m0(self._res0(b, x)))
        return x


def block_jacobi(K, free_dof):
    """M b of fep_solver_pcg_dev: the 2x2 block inverses of block_jacobi_kernel."""
    minv = block_jacobi_2x2(K, free_dof)
    return lambda r: apply_2x2(minv, r)


def _result(x, it, rr, bb, state, history):
    return {'x': x, 'iters': it, 'relres': np.sqrt(rr / bb) if bb > 0.0 else 0.0, 'state': state, 'history': history}


def pcg(K, free_dof, b, M, max_iter, rtol=0.0, keep=False):
    """Standard PCG of the multigrid solve (mg_init / mg_dot / mg_update / mg_direction / mg_scalar): x = 0, r = Q b,
    q = Q K p in double.  Returns {'x', 'iters', 'relres' (recursive), 'state' (0 max_iter, 1 converged, 2 breakdown),
    'history': [(x_k, relres_k)] for k = 1, 2, ... when `keep`}."""
    K = ssp.csr_matrix(K)
    f = np.asarray(free_dof, dtype=bool).ravel().astype(np.float64)
    tol2 = rtol * rtol
    x = np.zeros(K.shape[0])
    r = f * np.asarray(b, dtype=np.float64)
    z = M(r)
    p = z.copy()
    gamma, bb = z @ r, r @ r
    rr, history = bb, []
    if bb == 0.0:
        return _result(x, 0, rr, bb, 1, history)
    if not gamma > 0.0:
        return _result(x, 0, rr, bb, 2, history)
    for it in range(1, max_iter + 1):
        q = f * (K @ p)
        pq = p @ q
        if not pq > 0.0:
            return _result(x, it - 1, rr, bb, 2, history)
        alpha = gamma / pq
        x = x + alpha * p
        r = r - alpha * q
        rr = r @ r
        z = M(r)
        g = z @ r
        if keep:
            history.append((x.copy(), np.sqrt(rr / bb)))
        if rr <= tol2 * bb:
            return _result(x, it, rr, bb, 1, history)
        if not g > 0.0:
            return _result(x, it, rr, bb, 2, history)
        p = z + (g / gamma) * p
        gamma = g
    return _result(x, max_iter, rr, bb, 0, history)


def pcg_single_reduction(K, free_dof, b, M, max_iter, rtol=0.0, keep=False):
    """The block-Jacobi solve's form (pcg_init / pcg_update / spmv with (w, u) / pcg_scalar, Chronopoulos & Gear):
    u = M r, w = Q K u, one reduction phase per iteration.  Same results as `pcg`."""
    K = ssp.csr_matrix(K)
    f = np.asarray(free_dof, dtype=bool).ravel().astype(np.float64)
    tol2 = rtol * rtol
    n = K.shape[0]
    x, p, s = np.zeros(n), np.zeros(n), np.zeros(n)
    r = f * np.asarray(b, dtype=np.float64)
    u = M(r)
    w = f * (K @ u)
    g, rr, d = r @ u, r @ r, w @ u
    bb, history = rr, []
    if rr == 0.0:
        return _result(x, 0, rr, bb, 1, history)
    if not (g > 0.0 and d > 0.0):
        return _result(x, 0, rr, bb, 2, history)
    gamma, alpha, beta = g, g / d, 0.0
    for it in range(1, max_iter + 1):
        p = u + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        u = M(r)
        w = f * (K @ u)
        g, rr, d = r @ u, r @ r, w @ u
        if keep:
            history.append((x.copy(), np.sqrt(rr / bb)))
        if rr <= tol2 * bb:
            return _result(x, it, rr, bb, 1, history)
        beta = g / gamma
        den = d - beta * g / alpha
        if not (g > 0.0 and den > 0.0 and beta == beta):
            return _result(x, it, rr, bb, 2, history)
        alpha = g / den
        gamma = g
    return _result(x, max_iter, rr, bb, 0, history)

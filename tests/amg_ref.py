"""
Float64 restatement of the GPU solver's preconditioners and of both conjugate-gradient forms
(fem-elastoplasticity_amd/csrc/fep_solver.hip), for the tests that compare the device's iterates with it
(test_vcycle_gpu.py, test_solver_shapes_gpu.py, test_solver_forms_gpu.py) and the tests of the restatement itself
(test_amg_ref.py).  Plain NumPy / SciPy, no GPU (push_hierarchy alone talks to the device).

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


FOUR_PASS_NODES = 128 * 2048                 # NODES_PER_BLOCK * 2048 of vcycle_chebyshev's `big`


def node3_four_pass(level_sizes):
    """Per smoothed coarse level (levels 1 .. of `level_sizes` = KrylovSolver.amg_levels, the coarsest left out), whether
    vcycle_chebyshev launches node3_kernel<MODE, AV, 4> there: its `big` condition, from 262 144 nodes of three DOFs."""
    return [n // 3 >= FOUR_PASS_NODES for n, _ in level_sizes[1:-1]]


def product_lanes(n_terms, n_out):
    """Lanes per output entry of product_apply: product_kernel<8> from a mean of 12 terms per entry, <4> from 3, <1> below
    (0: no launch on an empty plan)."""
    if n_out <= 0:
        return 0
    mean = float(n_terms) / float(n_out)
    return 8 if mean >= 12.0 else 4 if mean >= 3.0 else 1


def singleton_hierarchy(K, free_dof, coordinates, coarse_nodes=64, max_levels=8):
    """A hierarchy whose level 1 has one node per mesh node, in the level dicts setup_amg pushes.  Transfer 0 gives every
    mesh node an aggregate of its own and leaves the prolongator unsmoothed: the 2x3 block of a free node is (I_2 | 0)
    (the aggregate's centre is the node, so the rotation column is empty), of a constrained DOF a zero row.  Level 1's
    operator then has the mesh's own node-block pattern (rows and columns of constrained DOFs and of every rotation empty)
    and both refresh products have about one term per entry.  Transfers 1 and up are build_amg_hierarchy's for bs = 3:
    aggregation, rigid-body modes, one damped-Jacobi step on the prolongator, Galerkin products, the same `last` rule.
    Reaches the forms the device chooses by a level's size (node3_four_pass) and by a plan's mean term count
    (product_lanes) with meshes of 2.6 * 10^5 nodes instead of 2.6 * 10^6."""
    f = np.asarray(free_dof, dtype=bool).ravel().astype(np.float64)
    A = solver._masked_operator(K, f)
    xy = np.asarray(coordinates, dtype=np.float64)
    n_n = A.shape[0] // 2
    Di = solver._block_diag_inverse(A, 2)
    rho = solver._rho(A, Di)
    out = []
    for level in range(max_levels):
        if level == 0:
            na = n_n
            Pt, cxy = solver._tentative(np.arange(n_n), na, xy, 2)
            P = (ssp.diags(f) @ Pt).tocsr()
            P.eliminate_zeros()                          # -(y - cy), x - cx: stored zeros
            last = False
        else:
            agg, na = solver._aggregate(A, 3)
            Pt, cxy = solver._tentative(agg, na, xy, 3)
            P = (Pt - (4.0 / (3.0 * rho)) * (Di @ solver._spgemm(A, Pt))).tocsr()
            last = na <= coarse_nodes or level == max_levels - 1 or 3 * na > 0.7 * A.shape[0]
        R = P.T.tocsr()
        Ac = solver._spgemm(R, solver._spgemm(A, P))
        if last:
            dense = Ac.toarray()
            dense += 1e-10 * np.abs(dense).max() * np.eye(dense.shape[0])
            Aop, Dc = ssp.csr_matrix(np.linalg.inv(dense)), None
        else:
            Aop, Dc = Ac, solver._block_diag_inverse(Ac, 3)
        for M in (P, R, Aop, Dc):
            if M is not None:
                M.sort_indices()
        out.append({'P': P, 'R': R, 'A': Aop, 'D': Dc, 'omega': 4.0 / (3.0 * 1.05 * rho), 'last': last,
                    'size': (Ac.shape[0], Ac.nnz)})
        if last:
            break
        A, xy, Di = Ac, cxy, Dc
        rho = solver._rho(A, Di)
    return out


def push_hierarchy(sol, levels, refresh=True):
    """KrylovSolver.setup_amg's upload for a given list of level dicts: fep_solver_amg_clear, one fep_solver_amg_push_level
    per transfer, fep_solver_amg_enable_refresh.  Sets sol.amg_hierarchy / amg_levels / amg_refresh and returns amg_levels.
    A refresh the device declines (FEP_ERANGE) is an error here: the caller chose the hierarchy so that it cannot."""
    l, ptr, check = solver._lib.lib(), solver._lib.ptr, solver._lib.check
    check(l.fep_solver_amg_clear(sol._h), 'fep_solver_amg_clear')
    for lv in levels:
        mats = []
        for M in (lv['P'], lv['R'], lv['A'], lv['D']):
            if M is None:
                mats += [None, None, None]
            else:
                mats += [np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32),
                         np.ascontiguousarray(M.data, dtype=np.float64)]
        check(l.fep_solver_amg_push_level(sol._h, lv['P'].shape[0], lv['P'].shape[1], *[ptr(m) for m in mats],
                                          float(lv['omega']), int(lv['last'])), 'fep_solver_amg_push_level')
    sol.amg_hierarchy = levels
    sol.amg_levels = [(sol.n_dof, sol.nnz)] + [lv['size'] for lv in levels]
    sol.amg_refresh = False
    if refresh:
        rc = l.fep_solver_amg_enable_refresh(sol._h)
        assert rc != -5, 'fep_solver_amg_enable_refresh answered FEP_ERANGE'
        check(rc, 'fep_solver_amg_enable_refresh')
        sol.amg_refresh = True
    return sol.amg_levels


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

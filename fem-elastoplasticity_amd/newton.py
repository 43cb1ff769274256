"""
Callers of the hot path: the reference's load-stepping / semismooth-Newton drivers
re-stated around the GPU step.

  solve_strip_footing   Plasticity2D_DP/pythonFEM.py:986-1131  (adaptive load steps, footing pressure)
  solve_tsx_tunnel      tsx-tunnel/pythonFEM.py:1729-1832      (17 uniform steps of the initial-stress factor;
                        the accepting call leaves `apply_plastic_strain` False)

(vonmises.py's cyclic driver runs `_load_history_loop` below, a fixed history of load factors on the same ops objects.)
Both run ONE loop, `_load_step_loop`: load steps, the Newton iteration with its stopping norms, accept / halve and the
extrapolation of the next iterate, following the reference line by line.  A driver hands it what its flavour does
differently: first step and smallest step, the initial strain of a step, the accepting call and what is recorded from
it, whether the step grows, when to stop.  The loop works on an ops object (`make_ops`): host arrays and a sparse direct
solve, or device tensors and conjugate gradients; dist_newton.py derives the element-sharded ops from the device ones.
Per Newton iterate ONE call of the fused step replaces DP:1043-1058 (strain, return map, tangent, residual).
The linear solve (the reference's dense `np.linalg.solve` on a (2 n_n)^2 boolean-masked matrix) is
  linear_solver='direct'  SciPy SuperLU on the host CSR matrix (K travels to the host every iterate), or
  linear_solver='pcg'     conjugate gradients on the GPU (solver.py, block-Jacobi preconditioner); the iterate, K, F,
                          the plastic strain and the stopping norms then never leave the device, or
  linear_solver='amg'     the same with the smoothed-aggregation multigrid preconditioner built once from K_elast.
`pcg_forcing` (e.g. 1e-2) makes the Newton iteration inexact: the linear tolerance follows the previous iterate's
stopping quantity instead of being 1e-11 throughout (never looser than `pcg_forcing_cap`); `pcg_inexact_rtol` (e.g. 1e-2)
asks every linear solve for that relative residual only — Newton then converges linearly with about that factor instead
of quadratically, which on plastic tangents (hundreds of CG iterations per digit) is much the cheaper trade: BASELINE
configs[3] end to end 42 s -> 15 s with the same load history (tools/newton_bench.py --inexact 1e-2).  The converged
states are the same to the Newton tolerance either way.
`transform` (DP:760-816, nodal averaging used for the footing pressure that steers the step size) is re-stated
with `np.bincount` on the host and as `fep_transform_dev` on the device.
"""
import time
from contextlib import closing

import numpy as np
import scipy.sparse.linalg as sspl

from .hotpath import MeshContext, in_situ_strain
from .mesh import square_mesh
from .tables import (ELEMENT_SHAPE, LagrangeElementType, _coerce, element_tables, get_local_basis_volume,
                     get_quadrature_volume)


def point_sums(q_int, elements, weight, n_n=None):
    """Per node, over the adjacent integration points: sum of w*q and sum of w (the two accumulations of DP:760-816).
    `n_n` defaults to the highest node of `elements` + 1."""
    n_p, n_e = elements.shape
    w = np.asarray(weight, dtype=float).ravel()
    nodes = np.repeat(np.asarray(elements), w.size // n_e, axis=1)       # (n_p, n_int)
    if n_n is None:
        n_n = int(nodes.max()) + 1
    wq = w * np.asarray(q_int, dtype=float).ravel()
    return (np.bincount(nodes.ravel(), weights=np.tile(wq, n_p), minlength=n_n),
            np.bincount(nodes.ravel(), weights=np.tile(w, n_p), minlength=n_n))


def transform(q_int, elements, weight):
    """Integration-point values -> nodal values, weighted average over the adjacent points (DP:760-816)."""
    f1, f2 = point_sums(q_int, elements, weight)
    return f1 / f2


class _HostOps:
    """Vectors as ndarrays, K as csr_matrix, sparse direct solve."""
    pcg_iters = None

    def __init__(self, ctx, qf):
        self.ctx, self.qf = ctx, qf

    def vec(self, a):
        return np.array(a, dtype=np.float64).ravel()

    def zeros(self):
        return np.zeros(self.qf.size)

    def new_ep(self):
        return np.zeros((4, self.ctx.n_int))

    def step(self, U, Ep=None, accept=False, e0=None, want=('K', 'F'), keep_K=False, e0_field=None, e0_scale=1.0):
        kw = {} if e0 is None else {'e0': e0}
        if e0_field is not None:
            kw.update(e0_field=e0_field, e0_scale=e0_scale)
        return self.ctx.step(U, Ep, apply_plastic_strain=accept, want=want, **kw)

    def field(self, a):
        """A (4, n_int) initial-strain field as these ops' step takes it."""
        return np.ascontiguousarray(a, dtype=np.float64)

    def setup_amg(self, K, coordinates):
        pass

    def cautious(self, on):
        """The second attempt of a load step (_load_history_loop): nothing to change for the direct solve."""

    def solve(self, K, rhs, criterion=None):
        rhs = np.asarray(rhs).ravel()
        x = np.zeros(rhs.size)
        x[self.qf] = sspl.spsolve(K[self.qf][:, self.qf].tocsc(), rhs[self.qf])
        return x

    def matvec(self, K, v):
        return K @ v

    def energy(self, K, v):
        return float(np.sqrt(v @ (K @ v)))

    def host(self, v):
        return np.asarray(v)

    def csr(self, K):
        return K

    def nodal(self, q_int, elem, weight):
        return transform(self.host(q_int), elem, weight)

    def load_volume(self, uniform):
        return self.vec(self.ctx.load_volume(uniform=uniform).flatten(order='F'))

    def assembled(self, f):
        """A force vector the context assembled on the host, as a vector of these ops."""
        return self.vec(f)

    def count(self, flags):
        return int(self.host(flags).astype(bool).sum())

    def estimate(self, s, p):
        """The error indicator of the point stress `s` on the problem `p` (_tsx_setup): on the context's GPU, or — a context
        without `estimate`, a `context_factory`'s — with the NumPy twin.  {'eta2', 'total', 'max', 'n_nonfinite'}."""
        s = np.ascontiguousarray(self.host(s), dtype=np.float64)
        if hasattr(self.ctx, 'estimate'):
            r = self.ctx.estimate(s)
        else:
            from .estimate import estimate_np
            hatp = get_local_basis_volume(p['type'], get_quadrature_volume(p['type'])[0])[0]
            r = estimate_np(p['elem'], self.ctx.geometry()[2], p['materials'][0], p['materials'][1], hatp, s, p['coords'].shape[1])
        return {k: r[k] for k in ('eta2', 'total', 'max', 'n_nonfinite')}

    def close(self):
        pass


class _DeviceOps:
    """Vectors, K data, plastic strain and stresses as device tensors; `MeshContext.step_dev` writes them and
    `solver.pcg` (KrylovSolver; dist_newton.DistributedPCG in the subclass there) solves on them.  A linear solve that
    breaks down or runs out of iterations yields NaNs, which the load-step loop treats like the reference treats a NaN
    criterion (DP:1076): the load step is halved."""

    def __init__(self, ctx, solver, rtol=1e-11, max_iter=200000, forcing=None, forcing_cap=1e-4, inexact_rtol=None, amg=False):
        import torch
        self.torch, self.ctx, self.solver, self.amg = torch, ctx, solver, amg
        self.dev = torch.device('cuda', ctx.device)
        self.rtol, self.max_iter, self.forcing, self.forcing_cap = rtol, max_iter, forcing, forcing_cap
        self.inexact_rtol = inexact_rtol
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.kd = torch.empty(ctx.nnz, **f64)
        self.F = torch.empty(ctx.n_dof, **f64)
        self.s = torch.empty((4, ctx.n_int), **f64)
        self.ind = torch.empty(ctx.n_int, dtype=torch.uint8, device=self.dev)
        self.counts = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.tmp = torch.empty(ctx.n_dof, **f64)
        self.pcg_iters = []
        self.precond = None                                    # the solver's choice: multigrid when a hierarchy is loaded

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def vec(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.float64).ravel()).to(self.dev)

    def zeros(self):
        return self.torch.zeros(self.ctx.n_dof, dtype=self.torch.float64, device=self.dev)

    def new_ep(self):
        return self.torch.zeros((4, self.ctx.n_int), dtype=self.torch.float64, device=self.dev)

    def _finish_force(self):
        """F as the step kernels left it is the whole internal force (the sharded subclass sums the interface)."""

    def _global_counts(self):
        return self.counts

    def field(self, a):
        """A (4, n_int) initial-strain field as these ops' step takes it: uploaded once, resident on the device."""
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def step(self, U, Ep=None, accept=False, e0=None, want=('K', 'F'), keep_K=False, e0_field=None, e0_scale=1.0):
        t = self.torch
        kd = None
        if 'K' in want:
            kd = t.empty(self.ctx.nnz, dtype=t.float64, device=self.dev) if keep_K else self.kd
        logs = 's' in want or 'ind_p' in want                  # accepting calls: the counters are logged
        self.ctx.step_dev(self._stream(), U.data_ptr(), ep=0 if Ep is None else Ep.data_ptr(),
                          accept=accept and Ep is not None, e0=e0, s=self.s.data_ptr() if 's' in want else 0,
                          ind_p=self.ind.data_ptr() if 'ind_p' in want else 0,
                          k_data=0 if kd is None else kd.data_ptr(), f_out=self.F.data_ptr() if 'F' in want else 0,
                          counts=self.counts.data_ptr() if logs else 0,
                          **({} if e0_field is None else {'e0_field': e0_field.data_ptr(), 'e0_scale': e0_scale}))
        if 'F' in want:
            self._finish_force()
        out = {'K': kd, 'F': self.F, 's': self.s, 'ind_p': self.ind}
        out = {k: v for k, v in out.items() if k in want}
        if logs:
            c = self._global_counts().cpu()
            out['n_smooth'], out['n_apex'] = int(c[0]), int(c[1])
        return out

    def setup_amg(self, K, coordinates):
        # built once from K_elast; rebuilding it from the current tangent when the plastic zone grows was measured
        # (1 M elements, 10 load steps: 6 rebuilds) and did not lower the iteration counts
        if self.amg:
            self.solver.setup_amg(self.host(K), coordinates, k_dev=K)

    def cautious(self, on):
        """The second attempt of a load step (_load_history_loop): while `on`, the multigrid ops solve with the block-Jacobi
        preconditioner.  The multigrid's Chebyshev smoother takes its interval from K_elast; on a soft plastic tangent the
        spectrum of the block-scaled matrix can leave it, the V-cycle is then indefinite and the conjugate gradients break
        down at once (state 2), on any iterate with that tangent.  The block inverses of a positive definite K are definite."""
        self.precond = 'jacobi' if on and self.amg else None

    def solve(self, K, rhs, criterion=None):
        # inexact Newton: while the iterate is far from converged the correction need not be solved to 11 digits.
        # `criterion` is the stopping quantity of the previous Newton iterate (DP:1075); the linear residual is asked
        # to be `forcing` times smaller than it, never looser than `forcing_cap` (1e-4) nor tighter than `rtol`.
        rtol = self.rtol
        if self.inexact_rtol and criterion is not None:        # (the elastic solves before the loop pass no criterion)
            rtol = max(self.rtol, self.inexact_rtol)
        elif self.forcing and criterion is not None and np.isfinite(criterion):
            rtol = min(self.forcing_cap, max(self.rtol, self.forcing * criterion))
        kw = {} if self.precond is None else {'precond': self.precond}
        x = self.solver.pcg(K, rhs, rtol=rtol, max_iter=self.max_iter, **kw)
        self.pcg_iters.append(self.solver.last['iters'])
        if self.solver.last['state'] != 1:
            x.fill_(float('nan'))
        return x

    def matvec(self, K, v):
        return self.solver.spmv(K, v)

    def energy(self, K, v):
        self.solver.spmv(K, v, out=self.tmp)
        return float(self.torch.sqrt(self.torch.dot(v, self.tmp)))

    def host(self, v):
        return v.cpu().numpy()

    def csr(self, K):
        return self.ctx.csr(self.host(K))

    def nodal(self, q_int, elem, weight):
        t = self.torch
        q = q_int.contiguous()
        out = t.empty(self.ctx.n_n, dtype=t.float64, device=self.dev)
        self.ctx.transform_dev(self._stream(), q.data_ptr(), out.data_ptr())
        return out.cpu().numpy()

    def assembled(self, f):
        """A force vector the context assembled on the host, as a vector of these ops (the sharded subclass sums the interface)."""
        return self.vec(f)

    def count(self, flags):
        """Number of set flags of a point array (the sharded subclass sums over the ranks)."""
        return int(self.host(flags).astype(bool).sum())

    def load_volume(self, uniform):
        f = self.zeros()
        self.ctx.load_volume_dev(self._stream(), f.data_ptr(), uniform=uniform)
        return f

    def estimate(self, s, p):
        """The error indicator of the device-resident point stress `s`: recovery, indicator and statistics on the device, read
        back once.  {'eta2', 'total', 'max', 'n_nonfinite'}."""
        eta2, st, _ = self.ctx.estimate_dev(s.contiguous())
        st = st.cpu()
        return {'eta2': eta2.cpu().numpy(), 'total': float(st[0]), 'max': float(st[1]), 'n_nonfinite': int(st[2])}

    def close(self):
        self.solver.close()


def make_ops(ctx, qf, linear_solver, pcg_rtol, pcg_forcing=None, pcg_forcing_cap=1e-4, pcg_inexact_rtol=None):
    """The vector / step / solve operations of a driver for `linear_solver` and its options (module docstring)."""
    if linear_solver == 'direct':
        return _HostOps(ctx, qf)
    if linear_solver in ('pcg', 'amg'):
        if not isinstance(ctx, MeshContext):
            raise ValueError(f"linear_solver='{linear_solver}' needs the GPU MeshContext")
        from .solver import KrylovSolver
        return _DeviceOps(ctx, KrylovSolver(ctx, qf), rtol=pcg_rtol, forcing=pcg_forcing, forcing_cap=pcg_forcing_cap,
                          inexact_rtol=pcg_inexact_rtol, amg=linear_solver == 'amg')
    raise ValueError("linear_solver must be 'direct', 'pcg' or 'amg'")


def _e0_keywords(e0):
    """The keywords of ops.step for the initial strain of a load step: `e0` itself (four values or None), or, when a driver
    hands a dict, the dict ({'e0_field': ..., 'e0_scale': ...}: a field per point and the step's factor)."""
    return e0 if isinstance(e0, dict) else {'e0': e0}


def _newton_iteration(ops, K_elast, U_it, Ep, e0, rhs_of, hist, criterion, zero_dU_converged=False, q_load=None):
    """The semismooth-Newton iteration of one load step, for every driver: at most 25 iterates from `U_it` at the plastic
    strain `Ep` and initial strain `e0`, each solving for the right-hand side `rhs_of(F)`, stopped on the K_elast norms.
    `criterion`: the previous step's (it steers the first inexact solve but one).  `zero_dU_converged`: an exactly zero
    correction counts as criterion 0 instead of the quotient as it stands.  `q_load`: the K_elast norm of the elastic response
    to the step's external load, added to the quotient's denominator (a state that the load holds at rest has iterates of
    rounding size, which the quotient alone compares with each other).  Returns (iterate, iterations, criterion)."""
    its = 0
    e0_kw = _e0_keywords(e0)
    for _ in range(25):                                                                   # DP:1040
        r = ops.step(U_it, Ep, want=('K', 'F'), **e0_kw)                                  # DP:1043-1058, TSX:1771-1778
        hist['n_calls'] += 1
        its += 1
        dU = ops.solve(r['K'], rhs_of(r['F']), criterion if its > 1 else 1.0)             # DP:1062-1066, TSX:1781
        U_new = U_it + dU
        q1, q2, q3 = ops.energy(K_elast, dU), ops.energy(K_elast, U_it), ops.energy(K_elast, U_new)   # DP:1072-1074
        den = q2 + q3 if q_load is None else q2 + q3 + q_load
        criterion = 0.0 if zero_dU_converged and q1 == 0 else q1 / den                    # TSX:1788-1792
        if np.isnan(criterion):                                                           # DP:1076
            break
        U_it = U_new
        if criterion < 1e-12:                                                             # DP:1086
            break
    return U_it, its, criterion


def _load_step_loop(ops, K_elast, U_it, d_zeta, d_zeta_min, hist, *, e0_of, accept_kw, accepted, finished, external=None):
    """The load-step loop around _newton_iteration, for both flavours (DP:1031-1127, TSX:1765-1826).
    `U_it`: the starting iterate.  Per flavour: `e0_of(zeta)` the initial strain of a step (or None), `accept_kw` the
    arguments of the accepting call of the step, `accepted(r, zeta, U, Ep_old, its, criterion)` records the step from
    that call's result `r` and returns (the plastic strain to go on with, whether the step may grow),
    `finished(zeta_old)` the flavour's stop besides `d_zeta_min`, `external` = (f_ext, q_ext) an external load that follows
    zeta: the Newton iterates of a step then solve for zeta * f_ext - F instead of -F, and zeta * q_ext (q_ext the K_elast
    norm of the elastic response to f_ext) joins the stopping quotient's denominator.  Returns the last accepted U and
    plastic strain."""
    def rhs_at(zeta):
        if external is None:
            return lambda F: -F
        return lambda F: zeta * external[0] - F
    d_zeta_old = d_zeta
    zeta_old = 0.0
    U = ops.zeros()
    U_old = -U_it
    Ep_old = ops.new_ep()
    criterion = None
    while True:
        zeta = zeta_old + d_zeta                                                          # DP:1031
        e0 = e0_of(zeta)                                                                  # TSX:1765
        U_it, its, criterion = _newton_iteration(ops, K_elast, U_it, Ep_old, e0, rhs_at(zeta), hist, criterion,
                                                 q_load=None if external is None else zeta * external[1])
        if criterion < 1e-10:                                                             # DP:1091, TSX:1804
            U_old = U
            U = U_it
            r = ops.step(U, Ep_old, **_e0_keywords(e0), **accept_kw)                      # DP:1095-1098, TSX:1809
            hist['n_calls'] += 1
            zeta_old = zeta
            d_zeta_old = d_zeta
            hist['zeta'].append(zeta)
            Ep_old, grow = accepted(r, zeta, U, Ep_old, its, criterion)
            if grow:
                d_zeta *= 2                                                               # DP:1109
        else:
            d_zeta /= 2                                                                   # DP:1117, TSX:1818
        U_it = d_zeta * (U - U_old) / d_zeta_old + U                                      # DP:1120, TSX:1821
        if finished(zeta_old) or d_zeta < d_zeta_min:                                     # DP:1123-1127, TSX:1824
            return U, Ep_old


def _load_history_loop(ops, K_elast, f_ext, zetas, hist, *, accepted, U=None, Ep=None, accept_want=('ind_p',)):
    """A prescribed history of load factors on an external load (no counterpart in the reference, whose plastic drivers
    load through prescribed displacements or an initial stress): for every `zeta` of `zetas` _newton_iteration on the residual
    zeta * f_ext - F(U), started from the last accepted U, then the accepting call, which updates the plastic strain in
    place: the state a load cycle carries.  The stopping quantity is 0 when the correction is exactly 0 (an elastic cycle
    returns to exactly U = 0 at zeta = 0, where the quotient is 0/0).  There is no sub-stepping.  A step that does not
    converge (25 iterates without a small stopping quantity, or a NaN one: a linear solve that broke down) is retried ONCE
    from the last accepted state, the first correction solved on K_elast instead of the tangent, then the iteration as
    before, with the ops `cautious` (the multigrid ops then precondition with the block inverses, which no tangent makes
    indefinite); its index goes to hist['retries'], and `accepted` is told the iterations of both attempts and the elastic
    correction.  (After a plastic step every point sits on its yield surface to rounding, so rounding decides which points
    the first tangent of the next step takes for plastic.  If most are and the load goes back, the soft tangent carries the
    iterate through the whole elastic range into reverse yielding, where the tangent is soft again, and the iteration
    alternates between the two for good; the elastic correction is the exact answer to an elastic step.  DESIGN.md
    section 7.)  A step that does not converge then either ends the history and its index goes to hist['failed_at'].
    The retry is reached only after a failure: a history that converged without it has the same iterates and calls as
    before.
    `accepted(r, zeta, U, its)` records a step from
    the accepting call's result.  `U`, `Ep`: the state the history goes on from (vectors of `ops`; `Ep` is updated in place),
    instead of zero: a history that was refined on the way (vonmises.solve_cutout_cyclic, adapt_at); `accept_want`: what the
    accepting calls return.  Returns the last accepted U and the plastic strain."""
    U = ops.zeros() if U is None else U
    Ep = ops.new_ep() if Ep is None else Ep
    criterion = None
    hist['failed_at'] = None
    hist.setdefault('retries', [])
    for k, zeta in enumerate(zetas):
        zeta = float(zeta)
        rhs_of = lambda F: zeta * f_ext - F                                                # noqa: E731
        U_it, its, criterion = _newton_iteration(ops, K_elast, U, Ep, None, rhs_of, hist, criterion, zero_dU_converged=True)
        if not criterion < 1e-10:
            hist['retries'].append(k)
            r = ops.step(U, Ep, want=('K', 'F'))
            hist['n_calls'] += 1
            U_el = U + ops.solve(K_elast, rhs_of(r['F']))
            ops.cautious(True)
            try:
                U_it, again, criterion = _newton_iteration(ops, K_elast, U_el, Ep, None, rhs_of, hist, None, zero_dU_converged=True)
            finally:
                ops.cautious(False)
            its += 1 + again
        if not criterion < 1e-10:
            hist['failed_at'] = k
            break
        U = U_it
        r = ops.step(U, Ep, accept=True, want=accept_want)
        hist['n_calls'] += 1
        hist['zeta'].append(float(zeta))
        accepted(r, zeta, U, its)
    return U, Ep


def _context_maker(context_factory, device):
    return context_factory or (lambda *a: MeshContext(*a, device=device))


def prandtl_nc(phi):
    """Prandtl's bearing-capacity factor of a strip footing on a weightless Mohr-Coulomb half plane: the limit pressure
    over the cohesion, N_c = (tan^2(45 deg + phi/2) e^(pi tan phi) - 1) / tan phi."""
    return (np.tan(np.pi / 4 + phi / 2) ** 2 * np.exp(np.pi * np.tan(phi)) - 1) / np.tan(phi)


def _footing_setup(element_type, level, n_cells, size_xy, make_context, model='dp', friction_angle=None, cohesion=None):
    """Mesh and context (materials set) of the strip-footing benchmark (DP:910-945), `c0`, and the times for the log.
    `model='mc'`: a Mohr-Coulomb context on (shear0, bulk0, sin(phi), c0) instead of the matched Drucker-Prager cone."""
    if model not in ('dp', 'mc'):
        raise ValueError("model must be 'dp' or 'mc'")
    t = _coerce(element_type)
    young, poisson, c0, phi = 1e7, 0.48, 450, np.pi / 9                                   # DP:910-933
    phi = phi if friction_angle is None else float(friction_angle)
    c0 = c0 if cohesion is None else cohesion
    shear0 = young / (2 * (1 + poisson))
    bulk0 = young / (3 * (1 - 2 * poisson))
    eta0 = 3 * np.tan(phi) / np.sqrt(9 + 12 * (np.tan(phi)) ** 2)
    c_0 = 3 * c0 / np.sqrt(9 + 12 * (np.tan(phi)) ** 2)
    t_setup = [time.perf_counter()]
    mesh = square_mesh(size_xy * 2 ** level if n_cells is None else n_cells, t, size_xy)  # DP:945
    t_setup.append(time.perf_counter())
    ctx = make_context(mesh['elements'], mesh['coordinates'], *element_tables(t))
    if model == 'mc':
        ctx.set_model('mc')
        ctx.set_materials(shear0, bulk0, np.sin(phi), c0)
    else:
        ctx.set_materials(shear0, bulk0, eta0, c_0)
    t_setup.append(time.perf_counter())
    return mesh, ctx, c0, t_setup


def solve_strip_footing(element_type='P1', level=1, n_cells=None, size_xy=10, max_steps=None, zeta_max=1.0,
                        device=None, log=None, context_factory=None, linear_solver='direct', pcg_rtol=1e-11,
                        keep_U=True, pcg_forcing=None, pcg_forcing_cap=1e-4, pcg_inexact_rtol=None, model='dp',
                        friction_angle=None, cohesion=None):
    """Strip-footing benchmark of Plasticity2D_DP (DP:901-1131).  `level` as in the reference
    (N = size_xy * 2**level cells per side) or `n_cells` directly.  Returns a dict with the load history
    ('zeta', 'pressure'), the accepted displacements 'U' (list of (2,n_n)), final 'Ep', counters.
    `context_factory(elements, coordinates, dhatp1, dhatp2, wf)` may supply another object with MeshContext's
    `set_materials / step / geometry / close` (the tests drive the same loop with their CPU checker that way).

    `model='dp'` (the default) is the reference's run: the Drucker-Prager cone matched in plane strain to the friction
    angle (20 degrees) and cohesion (450) of the benchmark.  `model='mc'` runs the same displacement-controlled loop on a
    Mohr-Coulomb context (MeshContext.set_model, also asked of a `context_factory`'s object) with the materials
    (shear0, bulk0, sin(phi), c0) from the same Young's modulus, Poisson's ratio, `friction_angle` (radians) and
    `cohesion`; the two arguments override the benchmark's values for either model.  'pressure' stays normalised by the
    cohesion, so for Mohr-Coulomb it tends to Prandtl's limit N_c = (tan^2(45 deg + phi/2) e^(pi tan phi) - 1) / tan phi
    from above as the mesh is refined (14.83 at 20 degrees; coarse meshes overshoot it).  The result's 'prandtl_nc' holds
    that number, and the log shows it beside the last pressure."""
    mesh, ctx, c0, t_setup = _footing_setup(element_type, level, n_cells, size_xy, _context_maker(context_factory, device),
                                            model, friction_angle, cohesion)
    nc = prandtl_nc(np.pi / 9 if friction_angle is None else float(friction_angle)) if model == 'mc' else None
    with closing(ctx), closing(make_ops(ctx, mesh['Q'].flatten(order='F'), linear_solver, pcg_rtol, pcg_forcing,
                                        pcg_forcing_cap, pcg_inexact_rtol)) as ops:
        hist = _strip_footing(mesh=mesh, ctx=ctx, ops=ops, c0=c0, t_setup=t_setup, max_steps=max_steps,
                              zeta_max=zeta_max, keep_U=keep_U, log=log)
    if nc is not None:
        hist['prandtl_nc'] = float(nc)
        if log and hist['pressure']:
            log(f'last pressure / c0 = {hist["pressure"][-1]:.6g}; Prandtl N_c = {nc:.6g}')
    return hist


def _strip_footing(*, mesh, ctx, ops, c0, t_setup, max_steps, zeta_max, keep_U, log):
    """solve_strip_footing once mesh, context and ops exist (dist_newton.py enters here with its sharded ones)."""
    elem, coord = mesh['elements'], mesh['coordinates']
    q_nd = mesh['dirichlet_nodes'][1, :] > 0
    K_elast = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']                        # DP:977
    t_setup.append(time.perf_counter())
    ops.setup_amg(K_elast, coord)                                                         # linear_solver='amg' only
    _, _, weight, _ = ctx.geometry()
    t_setup.append(time.perf_counter())
    if log:
        log('setup: mesh %.2f s, context %.2f s, solver + K_elast %.2f s, multigrid hierarchy %.2f s'
            % tuple(b - a for a, b in zip(t_setup[:-1], t_setup[1:])))

    d_zeta = 1 / 1000                                                                     # DP:989-994
    Ud = ops.vec((-d_zeta * mesh['dirichlet_nodes']).flatten(order='F'))                  # DP:997-1004
    U_it = Ud + ops.solve(K_elast, -ops.matvec(K_elast, Ud))
    hist = {'zeta': [], 'pressure': [], 'U': [], 'counts': [], 'n_calls': 0, 'newton_its': []}

    def accepted(r, zeta, U, Ep_old, its, criterion):                                     # Ep_old was updated in place
        pressure_old = hist['pressure'][-1] if hist['pressure'] else 0.0
        pressure_arr = ops.nodal(r['s'][1, :], elem, weight)                              # DP:1105
        pressure = -np.mean(pressure_arr[q_nd]) / c0
        hist['pressure'].append(pressure)
        if keep_U:
            hist['U'].append(ops.host(U).reshape((2, -1), order='F').copy())
        hist['counts'].append((r['n_smooth'], r['n_apex']))
        hist['newton_its'].append(its)
        if log:
            log(f'zeta={zeta:.6g} pressure={pressure:.10g} its={its} smooth/apex={r["n_smooth"]}/{r["n_apex"]}')
        return Ep_old, pressure - pressure_old < 0.1 and criterion < 1e-12                # DP:1109

    def finished(zeta_old):                                                               # DP:1123
        return zeta_old >= zeta_max or (max_steps is not None and len(hist['zeta']) >= max_steps)

    U, Ep_old = _load_step_loop(ops, K_elast, U_it, d_zeta, d_zeta / 1300, hist, e0_of=lambda zeta: None,
                                accept_kw=dict(accept=True, want=('s',)), accepted=accepted, finished=finished)
    hist['Ep'] = ops.host(Ep_old)
    hist['U_last'] = ops.host(U).reshape((2, -1), order='F').copy()
    hist['mesh'] = mesh
    hist['pcg_iters'] = ops.pcg_iters
    return hist


def solve_tsx_tunnel(coords=None, elem=None, element_type='P1', n_load_steps=17, monitor=(0, 40), device=None, log=None,
                     linear_solver='direct', pcg_rtol=1e-11, pcg_forcing=None, mesh_dir=None, pcg_inexact_rtol=None,
                     pcg_forcing_cap=1e-4, context_factory=None, refine=0, renumber=False, curves=None, in_situ=None,
                     body_force=None, materials=None, adapt=0, mark=None, theta=0.5, transfer_materials=False):
    """TSX tunnel excavation (TSX:1637-1832) on a given mesh (`coords` (2,n_n), `elem` (n_p,n_e) 0-based), or — as the
    reference does at TSX:1687-1690 — on the mesh read from `mesh_dir`/coord.csv, elem.csv with the midpoints of
    `element_type` added.  Returns the history of the monitored displacement, plastic-point counts and accepted
    displacements.  `context_factory` as in solve_strip_footing (the object also needs `assemble` and `n_int`).
    `refine` > 0 or `renumber` (no counterpart in the reference): the P1 mesh — `mesh_dir`'s, or `coords` / `elem` with
    3 vertex rows — is refined uniformly `refine` times (refine_uniform; the hole's boundary stays a polygon unless `curves`
    names it), then, with `renumber`, numbered along a Morton curve (refinement appends every level's nodes at the end), then raised to
    `element_type`; on the GPU when the context is the GPU one, on the host with a `context_factory`.  `monitor` keeps
    naming a node of the INPUT mesh; 'U' is in the numbering of the mesh solved on, returned as 'coords' / 'elem', and
    'node_of_input' maps input node ids to it (None unless renumbered).
    `curves` (a sequence of Ellipse; tsx_tunnel.TSX_HOLE is the tunnel wall): refinement and enrichment put their new
    boundary nodes on these curves (prepare_tsx_mesh; with `mesh_dir` alone the midpoints of load_tsx_mesh), and a mesh with
    a non-positive Jacobian determinant at any integration point (a P2 / P4 element folded by its curved side) is refused.
    `in_situ` (no counterpart in the reference, whose s0 is one stress for the whole mesh): a callable (x, y) -> (4, n)
    stress, rows 11, 22, 12, 33 (linear_in_situ builds the usual one), evaluated at the context's integration points
    (`point_coords`).  Its strain in_situ_strain(s0, shear, bulk) replaces the uniform initial strain as a field per point,
    handed to the ops once (on the device it stays resident); every step runs with e0_scale = zeta and the array is never
    rescaled.  `body_force` = (fx, fy), uniform (self-weight), goes with it: F0 = B^T w s0 - f_V and every Newton residual
    is F(U) - zeta f_V, so that a stress field in equilibrium with the body force (d s22 / dy = -fy) leaves the unexcavated
    ground at rest; the stopping quantity of the Newton iterates is then taken relative to the elastic response to the body force as well
    (_newton_iteration, q_load), since such a state has no displacement of its own to be relative to.  `materials` = (shear, bulk, eta, c), scalars or (n_int) arrays (layered ground), instead of the
    reference's constants.  With all three None the run is the reference's, bit for bit.  The result carries 's0_field'
    and the accepting calls' stress 's' ((4, n_int), list per step) when `in_situ` is given.
    `adapt` = k > 0 (no counterpart in the reference): the whole excavation runs k + 1 times; after each run but the last the
    P1 vertex mesh is refined where `mark` says (midpoints.refine_marked: conforming longest-edge bisection, new wall nodes on
    `curves`), renumbered again with `renumber`, raised to `element_type`, and the next run starts from zero on it (this
    driver carries no plastic strain from step to step, so there is no state to transfer).  `mark`: None — mark_plastic of
    the last accepted step's flags with one ring of neighbours — or a callable (hist, coords, elem_p1) -> bool (n_e) on the
    P1 vertex mesh the run was solved on — or 'zz': the recovered-stress error indicator of the last accepted step's stress
    (MeshContext.estimate on the context's GPU, estimate.estimate_np under a `context_factory`) with bulk marking of the
    fraction `theta` of its total (estimate.mark_bulk; the element ids of a P2 / P4 mesh are those of its P1 vertex mesh, so
    the indicator marks that directly).  Every row of 'adapt' then also holds 'eta' (the square root of the indicator's total),
    'n_nonfinite', 'theta' and 'eta2' (the indicator per element), and a non-finite indicator raises ValueError.
    `refine` is applied first, once; `in_situ` is evaluated again on every mesh;
    `materials` given as arrays raise ValueError unless `transfer_materials` is set: then every array (n_int) goes from each
    round's mesh to the next by the nearest-point rule of transfer.transfer_points (a copied modulus is one the caller gave;
    layer interfaces along element edges stay exact), with the element permutation of `renumber` applied to the parents and
    corner codes first, and every row of 'adapt' holds the round's 'materials' and the refinement's 'corners'.  The result is the last
    run's history — 'coords', 'elem', 'node_of_input' included — plus 'adapt': per run {'n_e', 'n_n', 'n_marked', 'n_child',
    'displ' (the last monitored value), 'n_steps' (accepted load steps), 'n_plast' (at the end), 'plastic' (elements with a plastic point at the end), 'marked', 'parent' (of the
    refinement that followed; None after the last run), 'ind_p' (the last accepted step's flags per integration point), 'coords',
    'elem' (the mesh of that run)}.  `monitor` keeps naming a node of the input mesh."""
    if body_force is not None and in_situ is None:
        raise ValueError('body_force goes with in_situ (the stress field it is in equilibrium with)')
    if adapt:
        return _tsx_adaptive(coords, elem, element_type, mesh_dir, refine, renumber, monitor, device, context_factory, log, curves,
                             int(adapt), mark, theta, materials, bool(transfer_materials),
                             dict(n_load_steps=n_load_steps, linear_solver=linear_solver, pcg_rtol=pcg_rtol, pcg_forcing=pcg_forcing,
                                  pcg_forcing_cap=pcg_forcing_cap, pcg_inexact_rtol=pcg_inexact_rtol, in_situ=in_situ,
                                  body_force=body_force))
    p = _tsx_setup(coords, elem, element_type, mesh_dir, refine, renumber, monitor, device, context_factory, log, curves)
    return _tsx_run(p, device, context_factory, log, materials, n_load_steps, linear_solver, pcg_rtol, pcg_forcing, pcg_forcing_cap,
                    pcg_inexact_rtol, in_situ, body_force)


def _tsx_run(p, device, context_factory, log, materials, n_load_steps, linear_solver, pcg_rtol, pcg_forcing, pcg_forcing_cap,
             pcg_inexact_rtol, in_situ, body_force):
    """solve_tsx_tunnel once the problem `p` (_tsx_setup) exists: context, ops, the load steps."""
    clock = [time.perf_counter()]
    ctx = _context_maker(context_factory, device)(p['elem'], p['coords'], *element_tables(p['type']))
    assert ctx.n_int == p['elem'].shape[1] * ELEMENT_SHAPE[p['type']][1]
    if materials is not None:
        p['materials'] = tuple(materials)
    ctx.set_materials(*p['materials'])
    clock.append(time.perf_counter())
    with closing(ctx), closing(make_ops(ctx, p['Q'].flatten(order='F'), linear_solver, pcg_rtol, pcg_forcing, pcg_forcing_cap,
                                        pcg_inexact_rtol)) as ops:
        _refuse_folded(p, ctx)
        return _tsx_tunnel(p, ctx, ops, clock, n_load_steps, log, in_situ, body_force)


def _tsx_adaptive(coords, elem, element_type, mesh_dir, refine, renumber, monitor, device, context_factory, log, curves, adapt,
                  mark, theta, materials, transfer_materials, run_kw):
    """solve_tsx_tunnel(adapt > 0): solve, mark, refine the marked elements, again."""
    from .hotpath import default_device
    from .mesh import renumber_for_locality
    from .meshio import load_tsx_mesh
    from .estimate import _check_theta, mark_bulk
    from .midpoints import DeviceMesh, child_corners, create_midpoints, mark_plastic, refine_marked, refine_uniform
    if adapt < 0:
        raise ValueError('adapt must be >= 0')
    zz = isinstance(mark, str)
    if zz and mark != 'zz':
        raise ValueError(f"mark: None, a callable or 'zz', got {mark!r}")
    if zz:
        theta = _check_theta(theta)
    if materials is not None and any(np.ndim(m) > 0 for m in materials) and not transfer_materials:
        raise ValueError('adapt: materials per integration point have no parent-to-child rule yet; pass scalars')
    carry = None                                               # (parent, corners) of the refinement before the round
    t = _coerce(element_type)
    if mesh_dir is not None:
        coords, elem = load_tsx_mesh(mesh_dir, 'P1')
    if coords is None or elem is None:
        raise ValueError('pass the mesh (coords, elem) or mesh_dir')
    c1, e1 = np.asarray(coords, dtype=np.float64), np.asarray(elem, dtype=np.int64)
    if e1.shape[0] != 3:
        raise ValueError(f'adapt starts from the P1 mesh: (3, n_e) vertex ids, got {e1.shape}')
    mesh_device = None if context_factory is not None else (default_device() if device is None else device)
    input_ids = np.arange(c1.shape[1])                         # where the input's nodes are in the current mesh
    if refine:
        c1, e1 = refine_uniform(c1, e1, levels=refine, device=mesh_device, curves=curves)
    n_q = ELEMENT_SHAPE[t][1]
    rounds = []
    for k in range(adapt + 1):
        if renumber:
            e1, c1, node_perm, elem_perm = renumber_for_locality(e1, c1)
            inv = np.empty_like(node_perm)
            inv[node_perm] = np.arange(node_perm.size)
            input_ids = inv[input_ids]
            if carry is not None:                              # new element j is old element elem_perm[j]
                carry = (carry[0][elem_perm], np.ascontiguousarray(carry[1][:, elem_perm]))
        if carry is not None:
            from .transfer import transfer_points
            materials = tuple(m if np.ndim(m) == 0 else transfer_points(t, carry[0], carry[1], np.asarray(m, dtype=np.float64).ravel(),
                                                                        device=mesh_device) for m in materials)
        ck, ek = c1, e1
        if t is not LagrangeElementType.P1:
            ext = create_midpoints(t, c1, e1, device=mesh_device, curves=curves)
            ck, ek = np.asarray(ext['coord_ext'], dtype=np.float64), np.asarray(ext['elem_ext'], dtype=np.int64)
        p = _tsx_setup(ck, ek, t, None, 0, False, (monitor[0], int(input_ids[monitor[1]])), device, context_factory, log, curves)
        p['prepared'], p['node_of_input'], p['keep_flags'] = True, (input_ids.copy() if renumber else None), True
        p['estimate'] = zz
        hist = _tsx_run(p, device, context_factory, log, materials, **run_kw)
        flags = hist.pop('ind_p')
        est = hist.pop('estimate', None)
        row = {'n_e': int(ek.shape[1]), 'n_n': int(ck.shape[1]), 'n_marked': None, 'n_child': None, 'displ': hist['displ'][-1],
               'n_steps': len(hist['zeta']), 'n_plast': hist['n_plast'][-1],
               'plastic': mark_plastic(flags, e1, n_q, rings=0), 'marked': None, 'parent': None,
               'ind_p': flags, 'coords': ck, 'elem': ek}
        if zz:
            row.update(eta=float(np.sqrt(est['total'])), n_nonfinite=est['n_nonfinite'], theta=theta, eta2=est['eta2'])
        if transfer_materials and materials is not None:
            row['materials'] = materials
        rounds.append(row)
        if log:
            log(f'adapt {k}: {row["n_e"]} elements, {row["n_n"]} nodes, U{monitor}={row["displ"]:.16g}')
        if k == adapt:
            break
        if zz:
            if est['n_nonfinite']:
                raise ValueError(f"adapt {k}: {est['n_nonfinite']} of {e1.shape[1]} error indicators are not finite")
            marked = np.asarray(mark_bulk(est['eta2'], theta, device=mesh_device)[0], dtype=bool)
        else:
            marked = mark_plastic(flags, e1, n_q, rings=1) if mark is None else np.asarray(mark(hist, c1, e1)) != 0
        if marked.shape != (e1.shape[1],):
            raise ValueError(f'mark: one entry per element ({e1.shape[1]},), got {marked.shape}')
        if transfer_materials and materials is not None:
            if mesh_device is None:
                corners = child_corners(c1, e1, marked)
            else:
                with DeviceMesh(c1, e1, mesh_device) as m:
                    m.mark(marked)
                    corners = m.child_corners()
            row['corners'] = corners
        c1, e1, parent = refine_marked(c1, e1, marked, device=mesh_device, curves=curves)
        row.update(n_marked=int(marked.sum()), n_child=int(e1.shape[1]), marked=marked, parent=parent)
        if 'corners' in row:
            carry = (parent, row['corners'])
    hist['adapt'] = rounds
    return hist


def _refuse_folded(p, ctx):
    """With curves, a mesh is refused unless the determinant of every integration point of `ctx` is positive."""
    if not p['curved']:
        return
    det = np.asarray(ctx.geometry()[3])
    if not (det > 0).all():
        raise ValueError(f'curved mesh: {int(np.count_nonzero(~(det > 0)))} of {det.size} integration points have a '
                         f'non-positive Jacobian determinant (smallest {det.min():.3e})')


def _tsx_setup(coords, elem, element_type, mesh_dir, refine, renumber, monitor, device, context_factory, log, curves=None):
    """Mesh, materials, initial stress and constraints of the TSX problem (TSX:1637-1699), before any context exists."""
    t = _coerce(element_type)
    node_of_input, t_mesh = None, {}
    curved = curves is not None and len(curves) > 0
    if refine or renumber:
        from .hotpath import default_device
        from .meshio import load_tsx_mesh, prepare_tsx_mesh
        if mesh_dir is not None:
            coords, elem = load_tsx_mesh(mesh_dir, 'P1')
        if coords is None or elem is None:
            raise ValueError('pass the mesh (coords, elem) or mesh_dir')
        mesh_device = None if context_factory is not None else (default_device() if device is None else device)
        coords, elem, node_of_input, t_mesh = prepare_tsx_mesh(coords, elem, t, refine=refine, renumber=renumber,
                                                               device=mesh_device, curves=curves)
        if node_of_input is not None:
            monitor = (monitor[0], int(node_of_input[monitor[1]]))
        if log:
            log('mesh: refine %.3f s, renumber %.3f s, enrich %.3f s; %d elements, %d nodes'
                % (t_mesh['refine'], t_mesh['renumber'], t_mesh['enrich'], elem.shape[1], coords.shape[1]))
    elif mesh_dir is not None:
        from .meshio import load_tsx_mesh
        coords, elem = load_tsx_mesh(mesh_dir, t, curves=curves)
    if coords is None or elem is None:
        raise ValueError('pass the mesh (coords, elem) or mesh_dir')
    young, nu = 60000, 0.2                                                                # TSX:1663-1672
    shear0 = young / (2 * (1 + nu))
    bulk0 = young / (3 * (1 - 2 * nu))
    fr = 49 * np.pi / 180
    eta0 = 3 * np.tan(fr) / np.sqrt(9 + 12 * (np.tan(fr)) ** 2)
    c_0 = 3 * 18.7 / np.sqrt(9 + 12 * (np.tan(fr)) ** 2)
    s0 = np.array([-45.0, -11.0, 0.0, -60.0]).reshape((-1, 1))                             # TSX:1675-1681
    tr0 = s0[0] + s0[1] + s0[3]
    init_strain = np.array([-nu * tr0 + (1 + nu) * s0[0], -nu * tr0 + (1 + nu) * s0[1], [0.0],
                            -nu * tr0 + (1 + nu) * s0[3]], dtype=float).reshape((-1, 1)) / young
    Q = np.ones(coords.shape, dtype=bool)                                                 # TSX:1695-1699
    Q[0, coords[0, :] < -49.99] = 0
    Q[0, coords[0, :] > 49.99] = 0
    Q[1, coords[1, :] < -49.99] = 0
    Q[1, coords[1, :] > 49.99] = 0
    return {'type': t, 'coords': coords, 'elem': elem, 'monitor': monitor, 'node_of_input': node_of_input, 't_mesh': t_mesh,
            'materials': (shear0, bulk0, eta0, c_0), 's0': s0, 'init_strain': init_strain, 'Q': Q,
            'prepared': bool(refine or renumber), 'curved': curved}


def _tsx_tunnel(p, ctx, ops, clock, n_load_steps, log, in_situ=None, body_force=None):
    """solve_tsx_tunnel once the problem `p` (_tsx_setup), context (materials set) and ops exist (dist_newton.py enters here
    with its sharded ones).  `clock`: the times before and after the context was made."""
    coords, monitor, s0, init_strain = p['coords'], p['monitor'], p['s0'], p['init_strain']
    K = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']                              # TSX:1722
    clock.append(time.perf_counter())
    ops.setup_amg(K, coords)                                                              # linear_solver='amg' only
    clock.append(time.perf_counter())
    t_setup = dict(p['t_mesh'], **dict(zip(('context', 'solver + K_elast', 'hierarchy'),
                                           (b - a for a, b in zip(clock[:-1], clock[1:])))))
    if log:
        log('setup: context %.2f s, solver + K_elast %.2f s, multigrid hierarchy %.2f s'
            % (t_setup['context'], t_setup['solver + K_elast'], t_setup['hierarchy']))
    field, external, s0_field = None, None, None
    if in_situ is None:
        F0 = ops.assembled(ctx.assemble(None, s0 * np.ones((1, ctx.n_int)))[1])           # TSX:1737
    else:
        xq = np.asarray(ctx.point_coords())
        s0_field = np.ascontiguousarray(np.broadcast_to(np.asarray(in_situ(xq[0], xq[1]), dtype=np.float64), (4, ctx.n_int)))
        field = ops.field(in_situ_strain(s0_field, p['materials'][0], p['materials'][1]))
        F0 = ops.assembled(ctx.assemble(None, s0_field)[1])
        if body_force is not None:
            f_V = ops.load_volume((float(body_force[0]), float(body_force[1])))
            F0 = F0 - f_V
            external = (f_V, ops.energy(K, ops.solve(K, f_V)))

    d_zeta = 1 / n_load_steps                                                             # TSX:1730-1735
    U_elast = ops.solve(K, -F0)                                                           # TSX:1748
    hist = {'zeta': [], 'displ': [], 'n_plast': [], 'U': [], 'n_calls': 0}
    kept = {}

    def accepted(r, zeta, U, Ep_old, its, criterion):
        Um = ops.host(U).reshape((2, -1), order='F')
        hist['displ'].append(Um[monitor])
        hist['n_plast'].append(ops.count(r['ind_p']))
        if p.get('keep_flags'):                                      # the adaptive driver marks from the last accepted step
            hist['ind_p'] = np.asarray(ops.host(r['ind_p'])).astype(bool).ravel()
        if p.get('estimate'):                                        # ... or from its stress (the ops' own array: not copied)
            kept['s'] = r['s']
        hist['U'].append(Um.copy())
        if field is not None:
            hist['s'].append(np.array(ops.host(r['s'])))
        if log:
            log(f'zeta={zeta:.6g} U{monitor}={Um[monitor]:.16g} n_plast={hist["n_plast"][-1]}')
        return ops.new_ep(), False                                   # 'ep' of a non-accepting call, TSX:1809

    # the accepting call leaves apply_plastic_strain False (C7)
    if field is None:
        _load_step_loop(ops, K, d_zeta * U_elast, d_zeta, d_zeta / 10, hist, e0_of=lambda zeta: zeta * init_strain,
                        accept_kw=dict(want=('s', 'ind_p') if p.get('estimate') else ('ind_p',)), accepted=accepted,
                        finished=lambda zeta_old: zeta_old >= 1)                                                     # TSX:1824
    else:
        hist['s'], hist['s0_field'] = [], s0_field
        _load_step_loop(ops, K, d_zeta * U_elast, d_zeta, d_zeta / 10, hist,
                        e0_of=lambda zeta: {'e0_field': field, 'e0_scale': zeta},
                        accept_kw=dict(want=('s', 'ind_p')), accepted=accepted, finished=lambda zeta_old: zeta_old >= 1,
                        external=external)
    hist['F0'] = np.asarray(ops.host(F0)).reshape((2, -1), order='F')
    hist['Q'] = p['Q']
    hist['pcg_iters'] = ops.pcg_iters
    hist['t_setup'] = t_setup
    if p.get('estimate'):
        hist['estimate'] = ops.estimate(kept['s'], p)
    if p['prepared']:
        hist['coords'], hist['elem'], hist['node_of_input'] = coords, p['elem'], p['node_of_input']
    return hist

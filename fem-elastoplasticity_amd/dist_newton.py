"""
The Newton / load-step driver on an element-sharded mesh (SURVEY 8e + 8f row 1): one process per GPU, every rank keeps
its part of the iterate, of K and of F on its device.

    K = sum_r P_r^T K_r P_r      sub-assembled: rank r holds K_r on its local nodes (sharding.ShardedContext), rows of
                                 interface nodes are partial sums
    vectors                      CONSISTENT: every rank holds the full value on all its local DOFs (interface DOFs are
                                 duplicated); a product K_r x_r is partial on the interface and becomes consistent by the
                                 interface exchange (the all-reduce of sharding.Partition.exchange_force_)
    inner products               sum over ranks of  sum_i w_i a_i b_i,  w_i = 1 / (number of ranks that hold DOF i)

DistributedPCG: conjugate gradients on K[Q][:,Q] x[Q] = b[Q] (the reference's np.linalg.solve, DP:1062-1066) with the
2x2 node-block Jacobi preconditioner of the single-GPU solver (the diagonal blocks of interface nodes are summed over the
ranks once per solve).  Per iteration: one local block SpMV (fep_solver_spmv_dev on K_r where the assembly kernels left
it), one interface exchange, two small all-reduces (p.Kp; r.z and r.r together).  The loop is driven from the host with
torch tensors as device vectors; convergence is looked at every `check_every` iterations.

GatheredSolver: the single-GPU multigrid conjugate gradients (solver.KrylovSolver) on K gathered to one rank every
Newton iterate — K_r and right-hand sides sent to the solve rank, merged by fep_csr_merge_f64 through the tables of
sharding.GatherPlan, solved there, x broadcast.  Block-Jacobi needs hundreds of times the iterations of the multigrid;
the solve is not on the sharded hot path, so the cheapest sound form keeps the solver whole.

solve_strip_footing_sharded: Plasticity2D_DP's load-step loop (DP:986-1131) on the ranks of the default process group.
It is newton.py's loop itself, entered with a ShardedContext and _ShardOps: newton's device ops with the local slice
in `vec`, the interface exchange of F, all-reduced branch counters, DistributedPCG or GatheredSolver as the solver,
energy norms through the weighted inner product and global gathers in `host` / `nodal`.
solve_tsx_tunnel_sharded: the same for the TSX tunnel (TSX:1729-1832).

The reference has no parallelism of any kind; this module is new.
"""
import time
from contextlib import closing

import numpy as np

from .newton import _DeviceOps, _footing_setup, _refuse_folded, _strip_footing, _tsx_setup, _tsx_tunnel, point_sums
from .sharding import ShardedContext
from .tables import element_tables


def _allreduce_(t, group=None, device=None):
    """In-place sum over the ranks.  The tensor goes where the backend can reduce it: device tensors through the host when
    the backend is gloo (rehearsal on one GPU), HOST tensors through the rank's device (`device`, default: torch's current
    one) when it is not — an RCCL process group rejects CPU tensors."""
    import torch
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return t
    gloo = dist.get_backend(group) == 'gloo'
    if t.is_cuda and gloo:
        tmp = t.cpu()
        dist.all_reduce(tmp, group=group)
        t.copy_(tmp)
    elif not t.is_cuda and not gloo:
        tmp = t.to(device if device is not None else torch.device('cuda', torch.cuda.current_device()))
        dist.all_reduce(tmp, group=group)
        t.copy_(tmp)
    else:
        dist.all_reduce(t, group=group)
    return t


class _DistAlgebra:
    """What every distributed solver here offers besides `pcg`: the local DOF numbering, the multiplicity weights, products
    with the sub-assembled K (local block SpMV + interface exchange) and global inner products of consistent vectors."""

    def __init__(self, sc, free_dof_global, group=None):
        import torch
        from .solver import KrylovSolver
        self.torch, self.sc, self.group = torch, sc, group
        ctx = sc.ctx
        self.dev = torch.device('cuda', ctx.device)
        dofs = (2 * sc.nodes[:, None] + np.arange(2)[None, :]).ravel()
        self.dofs_global = dofs
        free = np.asarray(free_dof_global).ravel()[dofs] != 0
        self.solver = KrylovSolver(ctx, free)
        self.free = torch.from_numpy(free.astype(np.float64)).to(self.dev)
        self.w = torch.from_numpy(np.repeat(1.0 / sc.mult, 2)).to(self.dev)          # 1 / multiplicity per local DOF
        self.n_dof = ctx.n_dof
        self.last = None

    def close(self):
        self.solver.close()

    def exchange_(self, v):
        return self.sc.exchange_force_(v, group=self.group)

    def dot(self, a, b):
        return _allreduce_((self.w * a * b).sum().reshape(1), self.group)[0]

    def spmv(self, k_data, x, masked=False):
        y = self.solver.spmv(k_data, x, masked=masked)
        return self.exchange_(y)


class DistributedPCG(_DistAlgebra):
    """Block-Jacobi conjugate gradients on the sub-assembled K of a ShardedContext."""

    def __init__(self, sc, free_dof_global, group=None):
        super().__init__(sc, free_dof_global, group)
        torch, ctx = self.torch, sc.ctx
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.wfree = self.w * self.free
        # positions of every node's diagonal 2x2 block in the CSR data of the local pattern
        ip, ix = ctx.pattern()
        n_n = ctx.n_n
        rows0 = ip[0:2 * n_n:2].astype(np.int64)
        rows1 = ip[1:2 * n_n:2].astype(np.int64)
        row_of = np.repeat(np.arange(2 * n_n, dtype=np.int64), np.diff(ip.astype(np.int64)))
        hit = np.flatnonzero((row_of % 2 == 0) & (ix == row_of))         # entry (2n, 2n) of every node that has a block
        has = np.zeros(n_n, dtype=bool)
        p = np.zeros(n_n, dtype=np.int64)
        has[row_of[hit] // 2] = True
        p[row_of[hit] // 2] = hit - rows0[row_of[hit] // 2]
        self._d_idx = [torch.from_numpy(a).to(self.dev) for a in (rows0 + p, rows0 + p + 1, rows1 + p, rows1 + p + 1)]
        self._has = torch.from_numpy(has.astype(np.float64)).to(self.dev)
        self.tmp = [torch.empty(self.n_dof, **f64) for _ in range(2)]

    def _block_jacobi(self, k_data):
        """Inverse of the assembled 2x2 diagonal blocks restricted to the free DOFs, as four per-node vectors."""
        t = self.torch
        d = [k_data[i] * self._has for i in self._d_idx]                 # d00, d01, d10, d11 of K_r
        a = t.stack([d[0], d[3]], dim=1).reshape(-1).contiguous()         # (d00, d11) and (d01, d10) as DOF vectors:
        b = t.stack([d[1], d[2]], dim=1).reshape(-1).contiguous()         # summed over the ranks by the interface exchange
        self.exchange_(a)
        self.exchange_(b)
        f0, f1 = self.free[0::2], self.free[1::2]
        d00 = t.where(f0 > 0, a[0::2], t.ones_like(f0))
        d11 = t.where(f1 > 0, a[1::2], t.ones_like(f1))
        both = f0 * f1
        d01, d10 = b[0::2] * both, b[1::2] * both
        d00 = t.where(d00 == 0, t.ones_like(d00), d00)                   # nodes of no element
        d11 = t.where(d11 == 0, t.ones_like(d11), d11)
        det = d00 * d11 - d01 * d10
        return d11 / det, -d01 / det, -d10 / det, d00 / det

    def _apply_m(self, Mi, r):
        t = self.torch
        r0, r1 = r[0::2], r[1::2]
        z = t.stack([Mi[0] * r0 + Mi[1] * r1, Mi[2] * r0 + Mi[3] * r1], dim=1).reshape(-1)
        return z * self.free

    def pcg(self, k_data, b, rtol=1e-11, max_iter=100000, check_every=10):
        """x (consistent, 0 on constrained DOFs) with |r| <= rtol |b[Q]| (weighted norms = the global Euclidean ones)."""
        t = self.torch
        Mi = self._block_jacobi(k_data)
        r = (b * self.free).clone()
        x = t.zeros_like(r)
        z = self._apply_m(Mi, r)
        p = z.clone()
        s = _allreduce_(t.stack([(self.w * r * z).sum(), (self.w * r * r).sum()]), self.group)
        rz, bb = s[0], float(s[1])
        if bb == 0.0:
            self.last = {'iters': 0, 'relres': 0.0, 'state': 1}
            return x
        state, it, rr = 0, 0, bb
        while it < max_iter:
            q = self.spmv(k_data, p, masked=True)
            pq = self.dot(p, q)
            alpha = rz / pq
            x.add_(alpha * p)
            r.sub_(alpha * q)
            z = self._apply_m(Mi, r)
            s = _allreduce_(t.stack([(self.w * r * z).sum(), (self.w * r * r).sum()]), self.group)
            beta = s[0] / rz
            rz = s[0]
            p = z + beta * p
            it += 1
            if it % check_every == 0 or it == max_iter:
                rr = float(s[1])
                pqh = float(pq)
                if not np.isfinite(rr) or not pqh > 0.0:
                    state = 2
                    break
                if rr <= (rtol ** 2) * bb:
                    state = 1
                    break
        self.last = {'iters': it, 'relres': float(np.sqrt(rr / bb)), 'state': state}
        return x


class GatheredSolver(_DistAlgebra):
    """The single-GPU multigrid conjugate gradients (solver.KrylovSolver, precond='amg') on K gathered to one rank.

    Every solve, each rank sends its K_r values and its right-hand side to the solve rank (one message per rank, persistent
    buffers, one `batch_isend_irecv`); there fep_csr_merge_f64 sums them onto the global pattern (sharding.GatherPlan),
    fep_gather_f64 picks the global right-hand side, the unchanged KrylovSolver solves, and x travels back in one
    broadcast together with `iters`, `relres` and `state` — so `last` is the same on every rank and the load-step loop
    branches the same way everywhere.  Products and inner products (energy norms) stay distributed (_DistAlgebra).
    With one rank everything is a device copy and no process group is needed.  Under nccl only device tensors move and the
    host is not synchronised before the solver itself reports its iteration count; under gloo (the rehearsal backend) the
    messages are staged through pinned host buffers.  Ranks without elements (`min_elements_per_rank`) are not supported.

    `seconds` accumulates, when `timed` is set (it synchronises the device around every phase), the wall time of
    'send', 'merge', 'solve', 'broadcast' over `n_solves` solves (tools/newton_bench.py)."""

    def __init__(self, sc, free_dof_global, elements_global, group=None, solve_rank=0):
        import torch.distributed as dist
        from .sharding import GatherPlan
        if sc.gated:
            raise ValueError('the gathered solve does not support ranks without elements (min_elements_per_rank)')
        super().__init__(sc, free_dof_global, group)
        torch = self.torch
        self.world = sc.world
        if self.world > 1 and not dist.is_initialized():
            raise ValueError('more than one rank needs an initialised process group')
        self.gloo = self.world > 1 and dist.get_backend(group) == 'gloo'         # resolved once
        self._root = solve_rank if (group is None or self.world == 1) else dist.get_global_rank(group, solve_rank)
        free_g = np.asarray(free_dof_global).ravel() != 0
        n_n = free_g.size // 2
        plan = self.plan = GatherPlan(sc, elements_global, n_n, solve_rank)
        self.is_solve_rank = plan.is_solve_rank
        if plan.block_map.size != sc.ctx.nnz // 4:
            raise AssertionError('the local pattern is not the node graph of the local elements')
        if self.world == 1:
            maps = [plan.own_map()]
        else:
            maps = [None] * self.world if self.is_solve_rank else None
            dist.gather_object(plan.own_map(), maps, dst=self._root, group=group)
        f64 = dict(dtype=torch.float64, device=self.dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)
        self.n_dof_g = 2 * n_n
        self.nnz_l = sc.ctx.nnz
        self._xbuf = torch.empty(self.n_dof_g + 3, **f64)                        # x, iters, relres, state: one broadcast
        self._xbuf_h = torch.empty(self.n_dof_g + 3, dtype=torch.float64).pin_memory() if self.gloo else None
        self._slice = i32(self.dofs_global)
        self.global_solver = None
        if self.is_solve_rank:
            from .solver import KrylovSolver
            plan.build_merge(maps)
            self._tab = [i32(a) for a in (plan.first, plan.multi_ptr, plan.multi_src, plan.rhs_index)]
            self._recv = torch.empty(plan.n_recv, **f64)
            self._recv_h = torch.empty(plan.n_recv, dtype=torch.float64).pin_memory() if self.gloo else None
            self._kg = torch.empty(plan.nnz, **f64)
            self._bg = torch.empty(self.n_dof_g, **f64)
            self._tail_h = torch.empty(3, dtype=torch.float64).pin_memory()
            self.global_solver = KrylovSolver(plan.pattern, free_g, device=sc.ctx.device)
        else:
            self._send = torch.empty(plan.n_send, **f64)
            self._send_h = torch.empty(plan.n_send, dtype=torch.float64).pin_memory() if self.gloo else None
            plan.nptr = plan.ncol = plan._pattern = None                         # the global pattern was only needed for the map
        self.timed = False
        self.seconds = {'send': 0.0, 'merge': 0.0, 'solve': 0.0, 'broadcast': 0.0}
        self.n_solves = 0

    def close(self):
        super().close()
        if self.global_solver is not None:
            self.global_solver.close()

    def _tick(self, key, t0):
        if not self.timed:
            return t0
        import time
        self.torch.cuda.synchronize(self.dev)
        t1 = time.perf_counter()
        if key is not None:
            self.seconds[key] += t1 - t0
        return t1

    def _gather(self, k_data, b):
        """K_r and b_r of every rank into the receive buffer of the solve rank."""
        import torch.distributed as dist
        n = self.nnz_l
        if self.is_solve_rank:
            a = self.plan.offsets
            own = self._recv[a[self.sc.rank]:a[self.sc.rank + 1]]
            own[:n].copy_(k_data)
            own[n:].copy_(b)
            if self.world > 1:
                buf = self._recv_h if self.gloo else self._recv
                ops = [dist.P2POp(dist.irecv, buf[a[r]:a[r + 1]], self._peer(r), self.group)
                       for r in range(self.world) if r != self.sc.rank]
                for w in dist.batch_isend_irecv(ops):
                    w.wait()                                                     # nccl: orders the stream, no host wait
                if self.gloo:
                    for r in range(self.world):
                        if r != self.sc.rank:
                            self._recv[a[r]:a[r + 1]].copy_(buf[a[r]:a[r + 1]], non_blocking=True)
        else:
            buf = self._send_h if self.gloo else self._send                      # (gloo: the copies synchronise; rehearsal only)
            buf[:n].copy_(k_data)
            buf[n:].copy_(b)
            for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, buf, self._root, self.group)]):
                w.wait()

    def _peer(self, r):
        import torch.distributed as dist
        return dist.get_global_rank(self.group, r) if self.group is not None else r

    def _merge(self):
        """K on the global pattern and the global right-hand side from the receive buffer (solve rank)."""
        from . import _lib
        first, mptr, msrc, rhs = self._tab
        st = self.torch.cuda.current_stream(self.dev).cuda_stream
        l = _lib.lib()
        _lib.check(l.fep_csr_merge_f64(self.dev.index, st, self.plan.n_blocks, first.data_ptr(), mptr.data_ptr(), msrc.data_ptr(),
                                       self._recv.data_ptr(), self._kg.data_ptr()), 'fep_csr_merge_f64')
        _lib.check(l.fep_gather_f64(self.dev.index, st, self.n_dof_g, self._recv.data_ptr(), rhs.data_ptr(), self._bg.data_ptr()),
                   'fep_gather_f64')

    def setup(self, K_elast, coordinates):
        """The multigrid hierarchy of the solve rank from the gathered K_elast (local values in, global coordinates)."""
        self._gather(K_elast, self.torch.zeros(self.n_dof, dtype=self.torch.float64, device=self.dev))
        if self.is_solve_rank:
            self._merge()
            self.global_solver.setup_amg(self._kg.cpu().numpy(), coordinates, k_dev=self._kg)

    def pcg(self, k_data, b, rtol=1e-11, max_iter=100000):
        """x (consistent, 0 on constrained DOFs) with |r| <= rtol |b[Q]|, by the multigrid solver of the solve rank."""
        from . import _lib
        import torch.distributed as dist
        torch = self.torch
        if self.is_solve_rank and not self.global_solver.amg_levels:
            raise RuntimeError('GatheredSolver.setup has not run')
        t = self._tick(None, 0.0)
        self._gather(k_data, b)
        t = self._tick('send', t)
        if self.is_solve_rank:
            self._merge()
            t = self._tick('merge', t)
            gs = self.global_solver
            gs.pcg(self._kg, self._bg, out=self._xbuf[:self.n_dof_g], rtol=rtol, max_iter=max_iter, precond='amg')
            self._tail_h[0], self._tail_h[1], self._tail_h[2] = gs.last['iters'], gs.last['relres'], gs.last['state']
            self._xbuf[self.n_dof_g:].copy_(self._tail_h, non_blocking=True)
            t = self._tick('solve', t)
        if self.world > 1:
            if self.gloo:
                if self.is_solve_rank:
                    self._xbuf_h.copy_(self._xbuf)
                dist.broadcast(self._xbuf_h, self._root, group=self.group)
                if not self.is_solve_rank:
                    self._xbuf.copy_(self._xbuf_h, non_blocking=True)
                tail = self._xbuf_h[self.n_dof_g:]
            else:
                dist.broadcast(self._xbuf, self._root, group=self.group)
                tail = self._xbuf[self.n_dof_g:].cpu()
        else:
            tail = self._tail_h
            torch.cuda.current_stream(self.dev).synchronize()
        x = torch.empty(self.n_dof, dtype=torch.float64, device=self.dev)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        _lib.check(_lib.lib().fep_gather_f64(self.dev.index, st, self.n_dof, self._xbuf.data_ptr(), self._slice.data_ptr(),
                                             x.data_ptr()), 'fep_gather_f64')
        self.last = {'iters': int(tail[0]), 'relres': float(tail[1]), 'state': int(tail[2]), 'precond': 'amg'}
        self._tick('broadcast', t)
        self.n_solves += 1
        return x


class _ShardOps(_DeviceOps):
    """newton._DeviceOps on a ShardedContext: local vectors (consistent on the interface), sub-assembled K, DistributedPCG
    (`linear_solver='pcg'`) or GatheredSolver ('amg', which needs the global element table) as the solver.  Only what the
    sharding changes is stated here."""

    def __init__(self, sc, qf_global, rtol=1e-11, max_iter=200000, inexact_rtol=None, group=None, linear_solver='pcg',
                 solve_rank=0, elements_global=None):
        if linear_solver not in ('pcg', 'amg'):
            raise ValueError("linear_solver must be 'pcg' or 'amg'")
        solver = (DistributedPCG(sc, qf_global, group) if linear_solver == 'pcg' else
                  GatheredSolver(sc, qf_global, elements_global, group, solve_rank))
        super().__init__(sc.ctx, solver, rtol=rtol, max_iter=max_iter, inexact_rtol=inexact_rtol, amg=linear_solver == 'amg')
        self.sc, self.group = sc, group
        self.n_dof_global = int(np.asarray(qf_global).size)

    def setup_amg(self, K, coordinates):
        if self.amg:
            self.solver.setup(K, coordinates)

    def assembled(self, f_local):
        """A force vector assembled by the rank's context (partial on the interface), made consistent."""
        return self.solver.exchange_(self.torch.from_numpy(np.array(f_local, dtype=np.float64).ravel()).to(self.dev))

    def count(self, flags):
        n = self.torch.count_nonzero(flags).reshape(1).to(self.torch.int64)
        return int(_allreduce_(n, self.group))

    def vec(self, a_global):
        a = np.asarray(a_global, dtype=np.float64).ravel()[self.solver.dofs_global]
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _finish_force(self):
        self.sc.exchange_force_(self.F, group=self.group)                # the one exchange of the hot path: interface forces

    def _global_counts(self):
        return _allreduce_(self.counts.clone(), self.group)

    def energy(self, K, v):
        return float(self.torch.sqrt(self.solver.dot(v, self.solver.spmv(K, v))))

    def host(self, v):
        """The GLOBAL vector on every rank (every DOF from the ranks that hold it, weighted: they agree)."""
        t = self.torch
        if v.dim() == 2:                                                 # point data (rows, n_int): this rank's slice only
            return v.cpu().numpy()
        g = t.zeros(self.n_dof_global, dtype=t.float64)
        g[t.from_numpy(self.solver.dofs_global)] = (v * self.solver.w).cpu()
        return _allreduce_(g, self.group, self.dev).numpy()

    def nodal(self, q_int, elem_global, weight_local):
        """transform (DP:760-816) of a point field: numerators and denominators summed over the ranks, global nodal array."""
        f = self.torch.from_numpy(np.stack(point_sums(q_int.cpu().numpy(), self.sc.nodes[self.sc.local_elements], weight_local,
                                                      self.n_dof_global // 2)))
        _allreduce_(f, self.group, self.dev)
        return (f[0] / f[1]).numpy()


def _ranks(group):
    import torch.distributed as dist
    if not dist.is_initialized():
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def solve_strip_footing_sharded(element_type='P1', level=1, n_cells=None, size_xy=10, max_steps=None, zeta_max=1.0,
                                device=None, log=None, pcg_rtol=1e-11, pcg_inexact_rtol=None, keep_U=True, group=None,
                                linear_solver='pcg', solve_rank=0, timed=False):
    """newton.solve_strip_footing on the ranks of the process group (torch.distributed initialised by the caller; a
    single process works too): the mesh is split by contiguous element ranges, every rank runs the hot path on its
    shard, and the Newton corrections are solved by the distributed block-Jacobi conjugate gradients above
    (`linear_solver='pcg'`) or by the multigrid solver on K gathered to rank `solve_rank` ('amg', GatheredSolver).  Every
    rank takes elements: idle ranks (`min_elements_per_rank`) are not offered here.  Returns the same history on every
    rank ('U' holds GLOBAL displacement fields; 'Ep' is the rank's own slice).  `timed` ('amg' only): the gathered solve
    synchronises around its phases and the history gets 'gathered_solve' = seconds per phase and the number of solves."""
    rank, world = _ranks(group)
    mesh, sc, c0, t_setup = _footing_setup(element_type, level, n_cells, size_xy,
                                           lambda elem, coord, *tab: ShardedContext(elem, coord, rank, world, *tab, device=device))
    with closing(sc), closing(_ShardOps(sc, mesh['Q'].flatten(order='F'), rtol=pcg_rtol, inexact_rtol=pcg_inexact_rtol,
                                        group=group, linear_solver=linear_solver, solve_rank=solve_rank,
                                        elements_global=mesh['elements'])) as ops:
        if linear_solver == 'amg':
            ops.solver.timed = bool(timed)
        hist = _strip_footing(mesh=mesh, ctx=sc.ctx, ops=ops, c0=c0, t_setup=t_setup, max_steps=max_steps,
                              zeta_max=zeta_max, keep_U=keep_U, log=log)
        if linear_solver == 'amg' and timed:
            hist['gathered_solve'] = dict(ops.solver.seconds, n_solves=ops.solver.n_solves)
        return hist


def solve_tsx_tunnel_sharded(coords=None, elem=None, element_type='P1', n_load_steps=17, monitor=(0, 40), device=None, log=None,
                             linear_solver='amg', pcg_rtol=1e-11, mesh_dir=None, pcg_inexact_rtol=None, refine=0,
                             renumber=False, group=None, solve_rank=0, curves=None, in_situ=None, body_force=None):
    """newton.solve_tsx_tunnel on the ranks of the process group (a single process works too), arguments as there
    (`linear_solver` 'pcg' or 'amg' as in solve_strip_footing_sharded; no `context_factory`, no forcing).  Every rank
    prepares the same mesh (`refine` / `renumber` run on each rank's device; the device refinement is bit-equal to the host
    one, so all ranks see one mesh), takes a contiguous range of its elements and enters newton's loop with its
    ShardedContext: the initial-stress force is made consistent by the interface exchange, the plastic-point counts are
    summed over the ranks.  `curves` as in solve_tsx_tunnel (each rank checks the determinants of its own elements).  Idle
    ranks (`min_elements_per_rank`) are not offered here.  Returns the same history on every rank.
    `in_situ` / `body_force` (solve_tsx_tunnel's initial-strain field per point) are refused with ValueError: the field is
    not sharded yet."""
    if in_situ is not None or body_force is not None:
        raise ValueError('in_situ / body_force: the sharded drivers do not shard an initial-strain field; '
                         'use solve_tsx_tunnel on one device')
    rank, world = _ranks(group)
    p = _tsx_setup(coords, elem, element_type, mesh_dir, refine, renumber, monitor, device, None, log, curves)
    clock = [time.perf_counter()]
    sc = ShardedContext(p['elem'], p['coords'], rank, world, *element_tables(p['type']), device=device)
    sc.set_materials(*p['materials'])
    clock.append(time.perf_counter())
    with closing(sc), closing(_ShardOps(sc, p['Q'].flatten(order='F'), rtol=pcg_rtol, inexact_rtol=pcg_inexact_rtol, group=group,
                                        linear_solver=linear_solver, solve_rank=solve_rank, elements_global=p['elem'])) as ops:
        _refuse_folded(p, sc.ctx)                                                         # each rank: its own elements
        return _tsx_tunnel(p, sc.ctx, ops, clock, n_load_steps, log)

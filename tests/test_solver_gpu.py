"""
GPU Krylov solver and nodal averaging against SciPy on the same matrices.

Tolerances: PCG runs to a relative residual of 1e-12, the solution is compared with SuperLU's to 1e-8
relative (condition number of the footing problem ~1e5..1e6); SpMV and `transform` to 1e-13.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as sspl

from conftest import needs_ablation_build, dp_materials, relerr

pytestmark = pytest.mark.gpu


def _problem(fep, et, n, plastic):
    mesh = fep.square_mesh(n, et, 10)
    ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'], element_type=et)
    ctx.set_materials(*dp_materials(ctx.n_int))
    rng = np.random.default_rng(3)
    U, Ep = np.zeros(ctx.n_dof), np.zeros((4, ctx.n_int))
    if plastic:                       # tangent at a converged iterate a few load steps into the plastic regime
        h = fep.solve_strip_footing(et, n_cells=n, max_steps=4)
        U, Ep = h['U'][-1], h['Ep']
    r = ctx.step(U, Ep, want=('K', 'F'))
    qf = mesh['Q'].flatten(order='F')
    return mesh, ctx, r, qf, rng


@pytest.mark.parametrize('et,n,plastic', [('P1', 12, False), ('P1', 40, True), ('P2', 8, True), ('Q1', 16, True),
                                          ('Q2', 6, False)])
def test_pcg_matches_sparse_direct(fep, et, n, plastic):
    mesh, ctx, r, qf, rng = _problem(fep, et, n, plastic)
    if plastic:
        assert r['n_smooth'] + r['n_apex'] > 0
    K = r['K']
    b = rng.normal(size=ctx.n_dof)
    sol = fep.KrylovSolver(ctx, qf)
    assert (sol.n_n, sol.n_dof, sol.nnz, sol.n_free) == (ctx.n_n, ctx.n_dof, ctx.nnz, int(qf.sum()))
    x = sol.solve_host(K, b, rtol=1e-12)
    assert sol.last['state'] == 1 and 0 < sol.last['iters'] < 20000 and sol.last['relres'] <= 1e-12
    ref = np.zeros(ctx.n_dof)
    ref[qf] = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
    assert np.all(x[~qf] == 0.0)
    assert relerr(x, ref) <= 1e-8
    res = (K @ x - b)[qf]
    assert np.linalg.norm(res) <= 1e-10 * np.linalg.norm(b[qf])       # true residual, not the recursive one
    # reproducible bit for bit
    assert np.array_equal(x, sol.solve_host(K, b, rtol=1e-12))
    sol.close()
    ctx.close()


def test_spmv_matches_scipy(fep):
    import torch
    mesh, ctx, r, qf, rng = _problem(fep, 'P2', 7, True)
    K = r['K']
    sol = fep.KrylovSolver(ctx, qf)
    x = rng.normal(size=ctx.n_dof)
    y = sol.spmv(K.data, x).cpu().numpy()
    assert relerr(y, K @ x) <= 1e-13
    xm = np.where(qf, x, 0.0)
    ym = sol.spmv(K.data, xm, masked=True).cpu().numpy()
    assert relerr(ym, np.where(qf, K @ xm, 0.0)) <= 1e-13 and np.all(ym[~qf] == 0.0)
    assert torch.cuda.is_available()
    sol.close()
    ctx.close()


def test_pcg_edge_cases(fep):
    mesh, ctx, r, qf, rng = _problem(fep, 'P1', 10, False)
    K = r['K']
    sol = fep.KrylovSolver(ctx, qf)
    # zero right-hand side on the free DOFs: x = 0 without iterating
    b0 = np.where(qf, 0.0, 7.0)
    x = sol.solve_host(K, b0)
    assert (sol.last['iters'], sol.last['relres'], sol.last['state']) == (0, 0.0, 1) and np.all(x == 0.0)
    # a negative definite matrix is reported as breakdown, not iterated on
    x = sol.solve_host(-K.data, rng.normal(size=ctx.n_dof))
    assert sol.last['state'] == 2
    # iteration cap
    x = sol.solve_host(K, rng.normal(size=ctx.n_dof), rtol=1e-14, max_iter=3, check_every=2)
    assert sol.last['state'] == 0 and sol.last['iters'] == 3 and np.isfinite(x).all()
    # everything constrained
    s2 = fep.KrylovSolver(ctx, np.zeros(ctx.n_dof, dtype=bool))
    assert np.all(s2.solve_host(K, rng.normal(size=ctx.n_dof)) == 0.0) and s2.last['state'] == 1
    s2.close()
    sol.close()
    ctx.close()


@pytest.mark.parametrize('et,n', [('P1', 48), ('P2', 12), ('Q1', 24)])
def test_multigrid_pcg_matches_sparse_direct(fep, et, n):
    """Hierarchy from K_elast, solve with the tangent of a plastic state (coarse operators lag behind on purpose)."""
    mesh, ctx, r, qf, rng = _problem(fep, et, n, True)
    assert r['n_smooth'] + r['n_apex'] > 0
    K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    sol = fep.KrylovSolver(ctx, qf)
    with pytest.raises(fep.FepError, match='call order'):
        sol.solve_host(r['K'], np.ones(ctx.n_dof), precond='amg')
    levels = sol.setup_amg(K_el, mesh['coordinates'], coarse_nodes=30)
    assert len(levels) >= 3 and levels[0][0] == ctx.n_dof and levels[-1][0] <= 3 * 200
    b = rng.normal(size=ctx.n_dof)
    for K in (K_el, r['K']):
        x = sol.solve_host(K, b, rtol=1e-12)
        it_amg = sol.last['iters']
        assert sol.last['state'] == 1 and sol.last['precond'] == 'amg' and 0 < it_amg < 200
        ref = np.zeros(ctx.n_dof)
        ref[qf] = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
        assert np.all(x[~qf] == 0.0) and relerr(x, ref) <= 1e-8
        assert np.linalg.norm((K @ x - b)[qf]) <= 1e-10 * np.linalg.norm(b[qf])
        assert np.array_equal(x, sol.solve_host(K, b, rtol=1e-12))                      # reproducible
        sol.solve_host(K, b, rtol=1e-12, precond='jacobi')
        assert sol.last['state'] == 1 and sol.last['iters'] > 2 * it_amg
    # zero right-hand side, breakdown on a negative definite matrix
    assert np.all(sol.solve_host(K_el, np.where(qf, 0.0, 1.0)) == 0.0) and sol.last['iters'] == 0
    sol.solve_host(-K_el.data, b)
    assert sol.last['state'] == 2
    sol.close()
    ctx.close()


def test_hierarchy_replaced_on_a_live_solver(fep):
    """`setup_amg` again on the same solver drops the levels and pushes new ones, here of other sizes (coarse_nodes 30 ->
    60 -> 30, refresh on: every level's operator is replaced by the one on the product's pattern as well).  The solver then
    solves as one that never held another hierarchy: bit for bit, in as many iterations."""
    mesh, ctx, r, qf, rng = _problem(fep, 'P1', 48, True)
    K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    b = rng.normal(size=ctx.n_dof)

    def setup_and_solve(sol, coarse_nodes):
        levels = sol.setup_amg(K_el, mesh['coordinates'], coarse_nodes=coarse_nodes, refresh=True)
        assert sol.amg_refresh is True
        x = sol.solve_host(r['K'], b, rtol=1e-11)
        assert sol.last['state'] == 1 and sol.last['precond'] == 'amg'
        return levels, x, sol.last['iters']

    sol = fep.KrylovSolver(ctx, qf)
    lv1, x1, it1 = setup_and_solve(sol, 30)
    lv2, x2, it2 = setup_and_solve(sol, 60)
    lv3, x3, it3 = setup_and_solve(sol, 30)
    assert len(lv1) >= 3 and lv2 != lv1 and lv3 == lv1                      # rebuilt at other sizes in between
    assert np.linalg.norm((r['K'] @ x2 - b)[qf]) <= 1e-9 * np.linalg.norm(b[qf])
    assert np.array_equal(x1, x3) and it1 == it3
    sol.close()
    fresh = fep.KrylovSolver(ctx, qf)
    lvf, xf, itf = setup_and_solve(fresh, 30)
    assert lvf == lv1 and np.array_equal(xf, x1) and np.array_equal(xf, x3) and itf == it1 == it3
    fresh.close()
    ctx.close()


@pytest.mark.parametrize('et,n', [('P1', 64), ('P2', 16), ('Q1', 32)])
def test_multigrid_refresh_reprojects_the_coarse_operators(fep, et, n):
    """`setup_amg(..., refresh=True)` (the default): every solve forms its coarse operators from ITS matrix with the
    transfers of the reference matrix (numeric Galerkin products on the device).  For the reference matrix itself these are
    the operators SciPy built at set-up, so the iteration counts agree; on a plastic tangent the solve needs fewer
    iterations than with the stale operators and reaches the same solution; run-to-run bitwise reproducible."""
    mesh, ctx, r, qf, rng = _problem(fep, et, n, True)
    K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    b = rng.normal(size=ctx.n_dof)
    res = {}
    for refresh in (False, True):
        sol = fep.KrylovSolver(ctx, qf)
        sol.setup_amg(K_el, mesh['coordinates'], coarse_nodes=30, refresh=refresh)
        assert sol.amg_refresh is refresh
        for name, K in (('elastic', K_el), ('tangent', r['K'])):
            x = sol.solve_host(K, b, rtol=1e-11)
            assert sol.last['state'] == 1
            assert np.linalg.norm((K @ x - b)[qf]) <= 1e-9 * np.linalg.norm(b[qf])
            assert np.array_equal(x, sol.solve_host(K, b, rtol=1e-11))
            res[refresh, name] = (x, sol.last['iters'])
        sol.close()
    assert abs(res[True, 'elastic'][1] - res[False, 'elastic'][1]) <= 1
    assert relerr(res[True, 'elastic'][0], res[False, 'elastic'][0]) <= 1e-8
    assert res[True, 'tangent'][1] <= res[False, 'tangent'][1]
    assert relerr(res[True, 'tangent'][0], res[False, 'tangent'][0]) <= 1e-7
    ctx.close()


@pytest.mark.parametrize('et,n', [('P1', 64), ('Q2', 12)])
def test_refresh_terms_listed_on_the_device_are_the_host_plan(fep, et, n, monkeypatch):
    """The terms of the numeric Galerkin products are listed on the device (plan_rows_kernel, one thread per row of the first
    factor) — FEP_AMG_PLAN=host lists them with fep_host.h's product_plan (the builder the sanitizer driver replays against the
    triple loop) and uploads the index pairs.  Same terms in the same order: the refreshed operators and with them every
    iterate of the solve are bit-identical."""
    needs_ablation_build(fep)
    mesh, ctx, r, qf, rng = _problem(fep, et, n, True)
    K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    b = rng.normal(size=ctx.n_dof)
    out = {}
    for mode in ('device', 'host'):
        monkeypatch.setenv('FEP_AMG_PLAN', mode)
        sol = fep.KrylovSolver(ctx, qf)
        sol.setup_amg(K_el, mesh['coordinates'], coarse_nodes=30, refresh=True)
        assert sol.amg_refresh
        out[mode] = [(sol.solve_host(K, b, rtol=1e-11), sol.last['iters'], sol.last['relres']) for K in (K_el, r['K'])]
        assert sol.last['state'] == 1
        sol.close()
    for (xd, itd, rd), (xh, ith, rh) in zip(out['device'], out['host']):
        assert itd == ith and rd == rh and np.array_equal(xd, xh)
    ctx.close()


@pytest.mark.parametrize('et,n', [('P1', 64), ('Q2', 12)])
def test_bottom_of_the_cycle_in_one_workgroup(fep, et, n, monkeypatch):
    """tail_kernel runs the last smoothed level and the coarsest solve under it in one launch; FEP_AMG_TAIL=0 keeps the eight
    launches it replaces.  The same operations (the block-Jacobi step's sums are associated differently): the same iteration
    counts, solutions to 1e-9, each form bit-reproducible."""
    needs_ablation_build(fep)
    mesh, ctx, r, qf, rng = _problem(fep, et, n, True)
    K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    b = rng.normal(size=ctx.n_dof)
    out = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('FEP_AMG_TAIL', mode)
        sol = fep.KrylovSolver(ctx, qf)
        sol.setup_amg(K_el, mesh['coordinates'], coarse_nodes=30)
        assert sol.amg_refresh and sol.amg_levels[-2][0] <= 3 * 384          # the tail's precondition holds on these meshes
        res = []
        for K in (K_el, r['K']):
            x = sol.solve_host(K, b, rtol=1e-11)
            assert sol.last['state'] == 1 and np.array_equal(x, sol.solve_host(K, b, rtol=1e-11))
            res.append((x, sol.last['iters']))
        out[mode] = res
        sol.close()
    for (xt, itt), (xl, itl) in zip(out['1'], out['0']):
        assert abs(itt - itl) <= 1 and relerr(xt, xl) <= 1e-9
    ctx.close()


@pytest.mark.parametrize('et,n', [('P1', 64), ('Q2', 12)])
def test_block_transfers_are_the_csr_transfers_in_single_precision(fep, et, n, monkeypatch):
    """The V-cycle applies its transfers in node blocks with single-precision values (prolong_block_kernel /
    restrict_block_kernel); FEP_AMG_BLOCK_TRANSFERS=0 keeps the double-precision CSR forms.  The same preconditioner up to seven
    digits of the transfers: the same iteration counts (+-2), the same solution, still symmetric (CG converges monotonically
    enough to meet 1e-11), run-to-run bit-identical."""
    needs_ablation_build(fep)
    mesh, ctx, r, qf, rng = _problem(fep, et, n, True)
    K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    b = rng.normal(size=ctx.n_dof)
    out = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('FEP_AMG_BLOCK_TRANSFERS', mode)
        sol = fep.KrylovSolver(ctx, qf)
        sol.setup_amg(K_el, mesh['coordinates'], coarse_nodes=30)
        res = []
        for K in (K_el, r['K']):
            x = sol.solve_host(K, b, rtol=1e-11)
            assert sol.last['state'] == 1 and np.array_equal(x, sol.solve_host(K, b, rtol=1e-11))
            assert np.linalg.norm((K @ x - b)[qf]) <= 1e-9 * np.linalg.norm(b[qf])
            res.append((x, sol.last['iters']))
        out[mode] = res
        sol.close()
    for (xb, itb), (xc, itc) in zip(out['1'], out['0']):
        assert abs(itb - itc) <= 2 and relerr(xb, xc) <= 1e-8
    ctx.close()


def test_drivers_with_multigrid_solver(fep):
    from conftest import load_golden
    g = load_golden('dp_p1_level1_trace')
    h = fep.solve_strip_footing('P1', level=1, linear_solver='amg')
    assert len(h['zeta']) == 16 and np.allclose(h['zeta'], g['zeta'], rtol=0, atol=1e-15)
    for k in range(16):
        assert relerr(h['U'][k], g['U_accepted'][k]) <= 1e-9, k
    # coarse operators are those of K_elast: ~40 iterations while the plastic zone is small, more near collapse
    assert h['counts'][-1] == (599, 171) and min(h['pcg_iters']) < 60 and max(h['pcg_iters']) < 5000
    t = load_golden('tsx')
    h = fep.solve_tsx_tunnel(t['coord'], t['elem'], 'P1', linear_solver='amg')
    assert len(h['zeta']) == 17 and h['n_plast'] == [0] * 13 + [1, 1, 2, 3]
    assert relerr(h['U'][-1], t['p1_U_final']) <= 1e-9
    a = fep.solve_strip_footing('P1', n_cells=48, max_steps=6)
    b = fep.solve_strip_footing('P1', n_cells=48, max_steps=6, linear_solver='amg')
    assert a['zeta'] == b['zeta'] and a['counts'] == b['counts']
    for k in range(6):
        assert relerr(a['U'][k], b['U'][k]) <= 1e-9, k


def test_inexact_newton_reaches_the_same_states_with_fewer_cg_iterations(fep):
    a = fep.solve_strip_footing('P1', n_cells=48, max_steps=6)
    b = fep.solve_strip_footing('P1', n_cells=48, max_steps=6, linear_solver='amg')
    c = fep.solve_strip_footing('P1', n_cells=48, max_steps=6, linear_solver='amg', pcg_forcing=1e-2)
    assert a['zeta'] == c['zeta'] and a['counts'] == c['counts']
    for k in range(6):
        assert relerr(a['U'][k], c['U'][k]) <= 1e-9, k
    assert sum(c['pcg_iters']) < 0.8 * sum(b['pcg_iters'])
    assert sum(c['newton_its']) <= sum(b['newton_its']) + 6            # at most one more Newton iterate per load step
    g = __import__('conftest').load_golden('dp_p1_level1_trace')
    h = fep.solve_strip_footing('P1', level=1, linear_solver='pcg', pcg_forcing=1e-2)
    assert len(h['zeta']) == 16 and np.allclose(h['zeta'], g['zeta'], rtol=0, atol=1e-15)
    for k in range(16):
        assert relerr(h['U'][k], g['U_accepted'][k]) <= 1e-9, k
    # every linear solve to two digits only: Newton converges linearly, the accepted states are the reference's
    d = fep.solve_strip_footing('P1', n_cells=48, max_steps=6, linear_solver='amg', pcg_inexact_rtol=1e-2)
    assert a['zeta'] == d['zeta'] and a['counts'] == d['counts']
    for k in range(6):
        assert relerr(a['U'][k], d['U'][k]) <= 1e-9, k
    assert sum(d['pcg_iters']) < 0.6 * sum(b['pcg_iters'])
    h = fep.solve_strip_footing('P1', level=1, linear_solver='amg', pcg_inexact_rtol=1e-2)
    assert len(h['zeta']) == 16 and np.allclose(h['zeta'], g['zeta'], rtol=0, atol=1e-15)
    for k in range(16):
        assert relerr(h['U'][k], g['U_accepted'][k]) <= 1e-9, k
    assert np.abs(np.array(h['pressure'][:15]) - g['pressure'][1:16]).max() <= 1e-8 * np.abs(g['pressure']).max()


def test_solver_rejects_foreign_patterns(fep):
    ip = np.array([0, 2, 3, 5, 7], dtype=np.int32)                 # rows 0 and 1 of node 0 differ in length
    ix = np.array([0, 1, 0, 2, 3, 2, 3], dtype=np.int32)
    with pytest.raises(fep.FepError, match='invalid argument'):
        fep.KrylovSolver((ip, ix), np.ones(4, dtype=bool), device=0)
    with pytest.raises(ValueError):
        fep.KrylovSolver((ip, ix), np.ones(3, dtype=bool), device=0)


@pytest.mark.parametrize('et', ['P1', 'P2', 'Q2'])
def test_transform_on_gpu_matches_host_restatement(fep, et):
    mesh = fep.square_mesh(9, et, 10)
    ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'], element_type=et)
    _, _, weight, _ = ctx.geometry()
    q = np.random.default_rng(1).normal(size=ctx.n_int)
    assert relerr(ctx.transform(q), fep.transform(q, mesh['elements'], weight)) <= 1e-13
    ctx.close()


def test_footing_driver_with_gpu_solver_reproduces_reference_trace(fep):
    """Same pins as the SuperLU-driven run (test_newton_gpu): the iterate never leaves the device here."""
    from conftest import load_golden
    g = load_golden('dp_p1_level1_trace')
    h = fep.solve_strip_footing('P1', level=1, linear_solver='pcg')
    assert len(h['zeta']) == 16 and np.allclose(h['zeta'], g['zeta'], rtol=0, atol=1e-15)
    assert np.abs(np.array(h['pressure'][:15]) - g['pressure'][1:16]).max() <= 1e-8 * np.abs(g['pressure']).max()
    for k in range(16):
        assert relerr(h['U'][k], g['U_accepted'][k]) <= 1e-9, k
    assert h['counts'][-1] == (599, 171)
    assert relerr(h['Ep'], g['Ep_final']) <= 1e-8
    assert h['pcg_iters'] and max(h['pcg_iters']) < 5000


def test_tsx_driver_with_gpu_solver(fep):
    from conftest import load_golden
    g = load_golden('tsx')
    h = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', linear_solver='pcg')
    assert len(h['zeta']) == 17 and h['n_plast'] == [0] * 13 + [1, 1, 2, 3]
    assert relerr(h['U'][-1], g['p1_U_final']) <= 1e-9
    assert abs(h['displ'][-1] - (-0.0019794496707526746)) <= 1e-9 * 0.0019794496707526746


def test_footing_48_cells_pcg_vs_direct(fep):
    a = fep.solve_strip_footing('P1', n_cells=48, max_steps=6)
    b = fep.solve_strip_footing('P1', n_cells=48, max_steps=6, linear_solver='pcg')
    assert a['zeta'] == b['zeta'] and a['counts'] == b['counts']
    for k in range(6):
        assert relerr(a['U'][k], b['U'][k]) <= 1e-9, k
    assert np.abs(np.array(a['pressure']) - np.array(b['pressure'])).max() <= 1e-8 * max(a['pressure'])


def test_sharded_newton_single_process_reproduces_reference_trace(fep):
    """dist_newton.solve_strip_footing_sharded with one rank (no process group): the sharded operations (weighted inner
    products, exchange, distributed conjugate gradients driven from the host) on the trivial partition — same pins as the
    single-GPU solver."""
    from conftest import load_golden
    g = load_golden('dp_p1_level1_trace')
    h = fep.solve_strip_footing_sharded('P1', level=1)
    assert len(h['zeta']) == 16 and np.allclose(h['zeta'], g['zeta'], rtol=0, atol=1e-15)
    assert np.abs(np.array(h['pressure'][:15]) - g['pressure'][1:16]).max() <= 1e-8 * np.abs(g['pressure']).max()
    for k in range(16):
        assert relerr(h['U'][k], g['U_accepted'][k]) <= 1e-9, k
    assert h['counts'][-1] == (599, 171)


@pytest.mark.parametrize('world,n_steps', [(2, 16), (3, 6)])
def test_sharded_newton_processes_vs_reference_trace(fep, tmp_path, world, n_steps):
    """BASELINE configs[3] as written ("... 1 vs 2 vs 4 vs 8 GPUs") end to end at the size the reference itself can run:
    `world` processes (here all on cuda:0, gloo), each with its element shard — iterate, K_r, F, plastic strain stay on
    the rank; hot path per shard + interface-force exchange; distributed block-Jacobi conjugate gradients on the
    sub-assembled K (local block SpMV + the same exchange + two scalar all-reduces per iteration).  Every rank must
    reproduce the reference driver's level-1 trace: load history exact, pressures 1e-8, accepted displacements 1e-9 (two
    ranks: all 16 load steps; three ranks — an interior shard with two cuts — the first six, to keep the suite short)."""
    import os
    import socket
    import subprocess
    import sys
    from conftest import load_golden
    g = load_golden('dp_p1_level1_trace')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dist_newton_worker.py')
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), str(tmp_path), str(n_steps if n_steps < 16 else 0)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    for p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, out[-3000:]
    n_pts = 0
    for r in range(world):
        d = np.load(tmp_path / f'rank{r}.npz')
        assert len(d['zeta']) == n_steps and np.allclose(d['zeta'], g['zeta'][:n_steps], rtol=0, atol=1e-15)
        assert np.abs(d['pressure'][:n_steps - 1] - g['pressure'][1:n_steps]).max() <= 1e-8 * np.abs(g['pressure']).max()
        for k in range(n_steps):
            assert relerr(d['U'][k], g['U_accepted'][k]) <= 1e-9, (r, k)
        # global branch counts on every rank: the reference's own (smooth, apex) pair of that accepting call
        assert (g['counts'] == d['counts'][-1]).all(axis=1).any() and (n_steps < 16 or tuple(d['counts'][-1]) == (599, 171))
        assert np.array_equal(d['counts'], np.load(tmp_path / 'rank0.npz')['counts'])
        assert int(d['n_calls']) == int(np.load(tmp_path / 'rank0.npz')['n_calls'])
        n_pts += int(d['n_local_points'])
    assert n_pts == 800                                              # 20 x 20 cells x 2 triangles, every point on one rank


@pytest.mark.gpu
def test_newton_354_cells_regression_guard(fep):
    """BASELINE configs[3]'s driver at 354 x 354 cells (250 632 P1 elements, 10 load steps) with the multigrid-CG solver and
    two-digit linear solves — `tools/newton_bench.py --n 354 --inexact 1e-2` — against the pins of
    tests/golden/newton_354_pins.json (written by tools/newton_pins.py, where the same history was also reached with
    ten-digit solves: pressures equal to `max_rel_pressure_difference`): load history exact, footing pressures to 1e-7,
    hot-path calls within 10 %, CG iterations within +50 % — so that later kernel work cannot break the end-to-end run
    unnoticed (reference loop DP:1028-1131)."""
    import json
    import os
    from conftest import GOLDEN
    pins = json.load(open(os.path.join(GOLDEN, 'newton_354_pins.json')))
    want = pins['inexact_1e-2']
    assert pins['max_rel_pressure_difference'] <= 1e-6
    h = fep.solve_strip_footing('P1', n_cells=354, max_steps=10, linear_solver='amg', pcg_rtol=1e-10, pcg_inexact_rtol=1e-2,
                                keep_U=False)
    assert [float(z) for z in h['zeta']] == want['zeta'] and len(h['zeta']) == 10
    got = np.array([float(p) for p in h['pressure']])
    assert np.abs(got - np.array(want['pressure'])).max() <= 1e-7 * np.abs(want['pressure']).max()
    assert abs(h['n_calls'] - want['hot_path_calls']) <= 0.1 * want['hot_path_calls']
    assert sum(h['pcg_iters']) <= 1.5 * want['pcg_iters_total']

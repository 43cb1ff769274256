"""
The gathered solve on the GPU (dist_newton.GatheredSolver): fep_csr_merge_f64 against its host statement, the merged K of
emulated shards against the whole-mesh context, and the sharded Newton drivers with the multigrid solver on K gathered to
one rank — in one process and in 2 / 3 processes on cuda:0 over gloo (tests/gathered_newton_worker.py).
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, dp_materials, load_golden, relerr
from meshes import rect as rect_mesh_of

pytestmark = pytest.mark.gpu


def _plans(fep, elem, n_n, world):
    plans = [fep.GatherPlan(fep.Partition(elem, n_n, r, world), elem, n_n) for r in range(world)]
    plans[0].build_merge([p.own_map() for p in plans])
    return plans


def _merge_dev(fep, plan, recv, launches=1):
    """fep_csr_merge_f64 + fep_gather_f64 on the tables of `plan`; (k, b) of every launch as host arrays."""
    import torch
    from importlib import import_module
    _lib = import_module('fem-elastoplasticity_amd._lib')
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    tab = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
           for a in (plan.first, plan.multi_ptr, plan.multi_src, plan.rhs_index)]
    R = torch.from_numpy(recv).to(dev)
    out = []
    for _ in range(launches):
        k = torch.full((plan.nnz,), float('nan'), dtype=torch.float64, device=dev)          # every value must be written
        b = torch.empty(2 * plan.n_n, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().fep_csr_merge_f64(0, st, plan.n_blocks, tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(),
                                                R.data_ptr(), k.data_ptr()), 'fep_csr_merge_f64')
        _lib.check(_lib.lib().fep_gather_f64(0, st, b.numel(), R.data_ptr(), tab[3].data_ptr(), b.data_ptr()), 'fep_gather_f64')
        out.append((k.cpu().numpy(), b.cpu().numpy()))
    return out


# sizes: fewer pairs than one 256-lane block, a few blocks with an odd tail, and many blocks; worlds with pairs of 1, 2 and
# 3 contributions (a node held by three ranks needs shards of a few elements)
@pytest.mark.parametrize('t,n,world,most', [('P1', 3, 4, 3), ('P1', 5, 6, 3), ('P2', 5, 7, 3), ('Q1', 3, 4, 3), ('P1', 41, 3, 2), ('Q2', 9, 2, 2)])
def test_merge_kernel_equals_host_statement_bitwise(fep, t, n, world, most):
    m = fep.square_mesh(n, t, 10)
    elem, n_n = m['elements'], m['coordinates'].shape[1]
    p0 = _plans(fep, elem, n_n, world)[0]
    cnt = np.diff(p0.multi_ptr)
    assert (p0.first >= 0).any() and (cnt == 2).any() and cnt.max() == most          # pairs of 1, 2 (and 3) contributions
    rng = np.random.default_rng(7)
    recv = rng.normal(size=p0.n_recv) * 10.0 ** rng.integers(-8, 8, size=p0.n_recv)      # sums whose order shows in the bits
    k_h, b_h = p0.merge_host(recv)
    (k1, b1), (k2, b2) = _merge_dev(fep, p0, recv, launches=2)
    assert k1.tobytes() == k_h.tobytes() and b1.tobytes() == b_h.tobytes()
    assert k2.tobytes() == k1.tobytes() and b2.tobytes() == b1.tobytes()


def test_merge_entry_point_checks_its_arguments(fep):
    import torch
    from importlib import import_module
    _lib = import_module('fem-elastoplasticity_amd._lib')
    l = _lib.lib()
    d = torch.zeros(16, dtype=torch.float64, device='cuda:0')
    i = torch.zeros(16, dtype=torch.int32, device='cuda:0')
    assert l.fep_csr_merge_f64(0, None, 0, None, None, None, None, None) == 0                 # nothing to do
    assert l.fep_csr_merge_f64(0, None, 2, None, i.data_ptr(), i.data_ptr(), d.data_ptr(), d.data_ptr()) == -1
    assert l.fep_csr_merge_f64(0, None, 2, i.data_ptr(), i.data_ptr(), i.data_ptr(), d.data_ptr() + 8, d.data_ptr()) == -1
    assert l.fep_csr_merge_f64(0, None, 2 ** 29, i.data_ptr(), i.data_ptr(), i.data_ptr(), d.data_ptr(), d.data_ptr()) == -5
    assert l.fep_csr_merge_f64(0, None, -1, None, None, None, None, None) == -1


@pytest.mark.parametrize('t,nx,ny,world', [('P1', 30, 45, 1), ('P1', 40, 60, 2), ('P1', 30, 45, 3), ('P2', 20, 30, 2), ('P2', 14, 21, 3),
                                           ('Q1', 24, 36, 2), ('Q1', 17, 25, 3)])
def test_merged_shards_reproduce_global_K(fep, t, nx, ny, world):
    """Shards stepped one after the other on cuda:0 (as test_shards_reproduce_global_step does), their K_r merged by the
    kernel: the global pattern is the whole-mesh context's, the merged values are its K (DESIGN §7 bounds: 1e-12 of the
    array maximum, 1e-11 per row against the row's own largest entry); one shard is the whole mesh, bit for bit."""
    elem, coord = rect_mesh_of(t, nx, ny, 10, 15)
    n_n = coord.shape[1]
    n_int = elem.shape[1] * fep.ELEMENT_SHAPE[fep.LagrangeElementType[t]][1]
    sh, bu, eta, c = dp_materials(n_int)
    x, y = coord
    U = np.array([2.5e-4 * y * (x / 10) + 1.2e-4 * x * (y > 5), -1.5e-4 * y * (x < 5) + 2.0e-4 * y * (x >= 5)])
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(sh, bu, eta, c)
    ref = ctx.step(U, np.zeros((4, n_int)), want=('K', 'F'))
    ip, ix = fep.global_pattern(elem, n_n)
    assert np.array_equal(ip, ctx.pattern()[0]) and np.array_equal(ix, ctx.pattern()[1])
    ctx.close()
    plans, segs = [], []
    for r in range(world):
        sc = fep.ShardedContext(elem, coord, r, world)
        sc.set_materials(sh, bu, eta, c)
        out = sc.ctx.step(U[:, sc.nodes], np.zeros((4, sc.ctx.n_int)), want=('K', 'F'))
        p = fep.GatherPlan(sc, elem, n_n)
        lip, lix = fep.global_pattern(sc.local_elements, sc.nodes.size)
        assert np.array_equal(lip, sc.ctx.pattern()[0]) and np.array_equal(lix, sc.ctx.pattern()[1])
        dofs = (2 * sc.nodes[:, None] + np.arange(2)[None, :]).ravel()
        segs.append(p.pack_host(out['K'].data, ref['F'][dofs]))                       # consistent right-hand side slices
        plans.append(p)
        sc.close()
    p0 = plans[0].build_merge([p.own_map() for p in plans])
    (k, b), = _merge_dev(fep, p0, np.concatenate(segs))
    kr = np.asarray(ref['K'].data)
    assert np.array_equal(b, ref['F'])
    if world == 1:
        assert k.tobytes() == kr.tobytes()
        return
    err = np.abs(k - kr)
    assert err.max() <= 1e-12 * np.abs(kr).max()
    row_max = np.maximum.reduceat(np.abs(kr), ip[:-1][np.diff(ip) > 0])
    row_err = np.maximum.reduceat(err, ip[:-1][np.diff(ip) > 0])
    assert (row_err <= 1e-11 * row_max).all()


@pytest.fixture(scope='module')
def single_amg(fep):
    """solve_strip_footing('P1', level=1, linear_solver='amg') per number of load steps, run once each."""
    cache = {}

    def run(n_steps):
        if n_steps not in cache:
            cache[n_steps] = fep.solve_strip_footing('P1', level=1, linear_solver='amg', max_steps=None if n_steps == 16 else n_steps)
        return cache[n_steps]
    return run


def _check_trace(d, g, n_steps, who):
    assert len(d['zeta']) == n_steps and np.allclose(d['zeta'], g['zeta'][:n_steps], rtol=0, atol=1e-15), who
    assert np.abs(np.asarray(d['pressure'])[:n_steps - 1] - g['pressure'][1:n_steps]).max() <= 1e-8 * np.abs(g['pressure']).max(), who
    for k in range(n_steps):
        assert relerr(d['U'][k], g['U_accepted'][k]) <= 1e-9, (who, k)
    last = tuple(int(v) for v in d['counts'][-1])
    assert (g['counts'] == np.array(last)).all(axis=1).any() and (n_steps < 16 or last == (599, 171)), who


def test_gathered_newton_single_process(fep, single_amg):
    """One rank, no process group: the merged matrix is the rank's own bit for bit, so the run is the single-GPU one,
    iteration count by iteration count, and meets the reference trace pins of the sharded tests."""
    g = load_golden('dp_p1_level1_trace')
    h = fep.solve_strip_footing_sharded('P1', level=1, linear_solver='amg')
    _check_trace(h, g, 16, 'one rank')
    ref = single_amg(16)
    assert list(h['pcg_iters']) == list(ref['pcg_iters'])
    assert h['n_calls'] == ref['n_calls']
    with pytest.raises(ValueError):
        fep.solve_strip_footing_sharded('P1', level=1, linear_solver='direct')


def _run_workers(tmp_path, world, job, timeout):
    """`world` (at most 3) fresh processes of the worker; on a timeout or a failure the others are killed, nothing is retried."""
    assert world <= 3
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gathered_newton_worker.py')
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), str(tmp_path), json.dumps(job)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, out[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return [np.load(tmp_path / f'rank{r}.npz') for r in range(world)]


def _same_on_all_ranks(ds, keys):
    for d in ds[1:]:
        for k in keys:
            assert np.array_equal(d[k], ds[0][k]), k


@pytest.mark.parametrize('world,n_steps', [(2, 16), (3, 6)])
def test_gathered_newton_processes_vs_reference_trace(fep, tmp_path, single_amg, world, n_steps):
    """The strip footing at level 1 on `world` processes with the gathered multigrid solve: the reference trace on every
    rank, identical histories across ranks, and CG iterations of the single-GPU multigrid class (at most 1.5 times its sum
    over the same steps, the margin of test_newton_354_cells_regression_guard: across ranks the interface rows are summed
    in another order, so counts may move by a few; block-Jacobi counts are hundreds of times larger)."""
    g = load_golden('dp_p1_level1_trace')
    ds = _run_workers(tmp_path, world, {'job': 'footing', 'level': 1, 'max_steps': None if n_steps == 16 else n_steps}, 600)
    for r, d in enumerate(ds):
        _check_trace(d, g, n_steps, r)
    _same_on_all_ranks(ds, ('zeta', 'counts', 'n_calls', 'pcg_iters'))
    assert sum(int(d['n_local_points']) for d in ds) == 800
    got, ref = int(ds[0]['pcg_iters'].sum()), int(sum(single_amg(n_steps)['pcg_iters']))
    print(f'world {world}, {n_steps} steps: {got} CG iterations gathered, {ref} on one GPU')
    assert got <= 1.5 * ref, f'{got} CG iterations on {world} ranks against {ref} on one GPU'


def test_gathered_newton_354_cells_two_processes(fep, tmp_path):
    """tests/golden/newton_354_pins.json with that guard's own tolerances, on two processes with the gathered solve."""
    want = json.load(open(os.path.join(GOLDEN, 'newton_354_pins.json')))['inexact_1e-2']
    ds = _run_workers(tmp_path, 2, {'job': 'footing', 'n_cells': 354, 'max_steps': 10, 'pcg_rtol': 1e-10, 'pcg_inexact_rtol': 1e-2,
                                    'keep_U': False}, 900)
    _same_on_all_ranks(ds, ('zeta', 'counts', 'n_calls', 'pcg_iters'))
    for d in ds:
        assert [float(z) for z in d['zeta']] == want['zeta'] and len(d['zeta']) == 10
        assert np.abs(d['pressure'] - np.array(want['pressure'])).max() <= 1e-7 * np.abs(want['pressure']).max()
        assert abs(int(d['n_calls']) - want['hot_path_calls']) <= 0.1 * want['hot_path_calls']
        got = int(d['pcg_iters'].sum())
        print(f'354 cells, 2 ranks: {got} CG iterations, pinned {want["pcg_iters_total"]}')
        assert got <= 1.5 * want['pcg_iters_total'], f'{got} CG iterations against the pinned {want["pcg_iters_total"]}'


def test_gathered_tsx_tunnel_two_processes(fep, tmp_path):
    g = load_golden('tsx')
    (tmp_path / 'a').mkdir()
    ds = _run_workers(tmp_path / 'a', 2, {'job': 'tsx'}, 600)
    _same_on_all_ranks(ds, ('zeta', 'n_plast', 'pcg_iters', 'n_calls', 'U_final'))
    for d in ds:
        assert len(d['zeta']) == 17 and d['n_plast'].tolist() == [0] * 13 + [1, 1, 2, 3]
        assert relerr(d['U_final'], g['p1_U_final']) <= 1e-9
        assert abs(float(d['displ'][-1]) - (-0.0019794496707526746)) <= 1e-9 * 0.0019794496707526746


def test_gathered_tsx_tunnel_refined_two_processes(fep, tmp_path):
    g = load_golden('tsx')
    h = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', refine=1, linear_solver='amg')
    ds = _run_workers(tmp_path, 2, {'job': 'tsx', 'refine': 1}, 600)
    _same_on_all_ranks(ds, ('zeta', 'n_plast', 'pcg_iters', 'n_calls', 'U_final'))
    for d in ds:
        assert d['zeta'].tolist() == list(h['zeta']) and d['n_plast'].tolist() == list(h['n_plast'])
        assert relerr(d['U_final'], h['U'][-1]) <= 1e-9


def test_gathered_tsx_tunnel_single_process_is_the_single_gpu_run(fep):
    g = load_golden('tsx')
    a = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', linear_solver='amg')
    b = fep.solve_tsx_tunnel_sharded(g['coord'], g['elem'], 'P1', linear_solver='amg')
    assert a['zeta'] == b['zeta'] and a['n_plast'] == b['n_plast'] and list(a['pcg_iters']) == list(b['pcg_iters'])
    assert np.array_equal(a['U'][-1], b['U'][-1]) and np.array_equal(a['F0'], b['F0'])


def test_sharded_tsx_tunnel_with_distributed_cg_single_process(fep):
    """The other solver of the sharded TSX driver (DistributedPCG), one rank: the pins of test_tsx_driver_with_gpu_solver."""
    g = load_golden('tsx')
    h = fep.solve_tsx_tunnel_sharded(g['coord'], g['elem'], 'P1', linear_solver='pcg')
    assert len(h['zeta']) == 17 and h['n_plast'] == [0] * 13 + [1, 1, 2, 3]
    assert relerr(h['U'][-1], g['p1_U_final']) <= 1e-9
    assert abs(h['displ'][-1] - (-0.0019794496707526746)) <= 1e-9 * 0.0019794496707526746


def test_capped_solve_is_nan_on_every_rank(fep, tmp_path):
    """A solve that runs out of iterations: NaN everywhere and the same `last` on both ranks, so that the load-step loop
    halves the step on all of them; the next, uncapped solve converges."""
    ds = _run_workers(tmp_path, 2, {'job': 'cap'}, 300)
    for d in ds:
        assert np.isnan(d['x']).all() and d['x'].size > 0
        assert d['last'].tolist() == ds[0]['last'].tolist() and int(d['last'][0]) == 1 and int(d['last'][2]) == 0
        assert bool(d['y_finite']) and d['last_full'].tolist() == ds[0]['last_full'].tolist() and int(d['last_full'][1]) == 1

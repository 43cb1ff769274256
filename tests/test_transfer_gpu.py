"""
State transfer across refinement on the GPU (fep_mesh_child_corners_*, fep_transfer_nodes_*, fep_transfer_points_*) against
the NumPy twin (transfer.py), bit for bit but for the sign bit of a NaN, on the cases of transfer_cases.py; the refusals;
graph replay; what the _dev forms write (tests/footprint.py).
"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import marked_cases as mc
import transfer_cases as tc

pytestmark = pytest.mark.gpu

DEV = 0
EINVAL, ESTATE = -1, -6                                       # include/fep.h
TYPES = ('P1', 'P2', 'P4')


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if dtype is None else a.astype(dtype)).to(f'cuda:{DEV}')


@pytest.fixture(scope='module')
def twin(fep):
    """The twin's results, computed once per (case, type, n_comp | n_rows) and left unchanged."""
    memo = {}

    def get(kind, name, t, n):
        key = (kind, name, t, n)
        if key not in memo:
            c = tc.case(name)
            ep, n_np, ech, n_nc, _, _ = tc.raised(name, t)
            if kind == 'nodes':
                u = tc.nodal_field(n_np, n)
                memo[key] = (u, fep.transfer_nodes_np(t, ep, ech, c['parent'], c['corners'], u, n_n_child=n_nc))
            else:
                q = tc.point_field(n, c['elem'].shape[1] * tc.N_Q[t])
                memo[key] = (q, fep.transfer_points_np(t, c['parent'], c['corners'], q))
        return memo[key]
    return get


@pytest.mark.parametrize('name', [c['name'] for c in tc.cases() if c['marked'] is not None])
def test_corner_codes(fep, name):
    import torch
    c = tc.case(name)
    with fep.DeviceMesh(c['coord'], c['elem'], DEV) as m:
        with pytest.raises(ValueError, match='mark'):
            m.child_corners()
        if c['curves']:
            m.set_curves(list(c['curves']))
        m.mark(c['marked'])
        host, again, dev = m.child_corners(), m.child_corners(), m.child_corners_dev()
        assert m.refine_marked()[2].tobytes() == c['parent'].tobytes()
    assert host.dtype == np.uint8 and host.shape == c['corners'].shape
    assert host.tobytes() == c['corners'].tobytes() == again.tobytes() == dev.cpu().numpy().tobytes() and dev.dtype == torch.uint8


def test_uniform_corners_on_the_device(fep):
    corners, parent = fep.uniform_corners(72)
    cd, pd = fep.uniform_corners(72, device=DEV)
    assert cd.cpu().numpy().tobytes() == corners.tobytes() and np.array_equal(pd.cpu().numpy(), parent) and cd.is_contiguous()


@pytest.mark.parametrize('t', TYPES)
def test_transfer_is_the_twins(fep, twin, t):
    import torch
    for name in tc.names(t):
        c = tc.case(name)
        ep, n_np, ech, n_nc, _, _ = tc.raised(name, t)
        parent, corners = c['parent'], c['corners']
        ep_d, ech_d, par_d, cor_d = _t(ep, np.int32), _t(ech, np.int32), _t(parent, np.int32), _t(corners)
        for n_comp in (1, 2, 4):
            u, want = twin('nodes', name, t, n_comp)
            host = fep.transfer_nodes(t, ep, ech, parent, corners, u, n_n_child=n_nc, device=DEV)
            dev = fep.transfer_nodes_dev(t, ep_d, ech_d, par_d, cor_d, _t(u), n_nc)
            again = fep.transfer_nodes_dev(t, ep_d, ech_d, par_d, cor_d, _t(u), n_nc)
            assert host.shape == want.shape == tuple(dev.shape) and tc.same_but_nan_sign(host, want), (name, n_comp)
            assert dev.cpu().numpy().tobytes() == host.tobytes() == again.cpu().numpy().tobytes(), (name, n_comp)
        u, want = twin('nodes', name, t, 2)                                       # the drivers' interleaved U
        flat = fep.transfer_nodes_dev(t, ep_d, ech_d, par_d, cor_d, _t(u).reshape(-1), n_nc)
        assert tuple(flat.shape) == (2 * n_nc,) and flat.cpu().numpy().tobytes() == want.tobytes()
        for n_rows in (1, 4):
            q, want = twin('points', name, t, n_rows)
            host = fep.transfer_points(t, parent, corners, q, device=DEV)
            dev = fep.transfer_points_dev(t, par_d, cor_d, _t(q))
            again = fep.transfer_points_dev(t, par_d, cor_d, _t(q))
            assert host.tobytes() == want.tobytes() == dev.cpu().numpy().tobytes() == again.cpu().numpy().tobytes(), (name, n_rows)
    torch.cuda.synchronize()


@pytest.mark.parametrize('t', TYPES)
def test_nonfinite_and_bad_children(fep, t):
    """A NaN at a node or a point, children with a bad parent or bad codes, a node of no element: the twin's bytes (whose sets
    test_transfer_host.py pins), and a clean call afterwards gives the clean bytes."""
    c = tc.case('unstructured' if t == 'P1' else 'tunnel-curved')
    ep, n_np, ech, n_nc, _, _ = tc.raised(c['name'], t)
    n_e, n_child, n_q = c['elem'].shape[1], c['parent'].size, tc.N_Q[t]
    u, q = tc.nodal_field(n_np, 2), tc.point_field(4, n_e * n_q)
    clean_u = fep.transfer_nodes(t, ep, ech, c['parent'], c['corners'], u, n_n_child=n_nc, device=DEV)
    clean_q = fep.transfer_points(t, c['parent'], c['corners'], q, device=DEV)
    parent, corners = c['parent'].copy(), c['corners'].copy()
    parent[3], parent[n_child // 2] = n_e, -1
    corners[:, n_child - 1], corners[:, 7], corners[:, 11] = (6, 0, 1), (0, 0, 1), (255, 1, 2)
    bad_u, bad_q = u.copy(), q.copy()
    bad_u[0, 1], bad_u[n_np - 1, 0], bad_q[3, 5 * n_q], bad_q[0, n_e * n_q - 1] = np.nan, np.inf, np.nan, -np.inf
    ep_bad = ep.copy()
    ep_bad[0, 20] = n_np                                                               # a parent element naming a node outside u
    want_u = fep.transfer_nodes_np(t, ep_bad, ech, parent, corners, bad_u, n_n_child=n_nc + 3)
    want_q = fep.transfer_points_np(t, parent, corners, bad_q)
    got_u = fep.transfer_nodes(t, ep_bad, ech, parent, corners, bad_u, n_n_child=n_nc + 3, device=DEV)
    got_q = fep.transfer_points(t, parent, corners, bad_q, device=DEV)
    assert np.isnan(want_u).any() and np.isnan(want_u[n_nc:]).all() and not np.isnan(want_u).all()
    assert tc.same_but_nan_sign(got_u, want_u) and tc.same_but_nan_sign(got_q, want_q)
    assert fep.transfer_nodes(t, ep, ech, c['parent'], c['corners'], u, n_n_child=n_nc, device=DEV).tobytes() == clean_u.tobytes()
    assert fep.transfer_points(t, c['parent'], c['corners'], q, device=DEV).tobytes() == clean_q.tobytes()


def test_no_children_is_legal(fep):
    tab = fep.transfer_tables('P2')
    u = np.ones((4, 2))
    out = np.full((5, 2), 7.0)
    ptr = fep._lib.ptr
    ep = np.zeros((6, 1), dtype=np.int32)
    rc = fep.lib().fep_transfer_nodes_host(DEV, 2, 2, 1, 4, 0, 5, ptr(ep), None, None, None, ptr(tab['shape_of_code']), ptr(tab['W']),
                                           ptr(u), ptr(out))
    assert rc == 0 and np.isnan(out).all()                                            # every node is a node of no child element
    rc = fep.lib().fep_transfer_points_host(DEV, 2, 1, 1, 0, None, None, ptr(tab['shape_of_code']), ptr(tab['near']), ptr(np.ones(7)), None)
    assert rc == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(fep):
    import torch
    c = tc.case('pair-10')
    t = 'P2'
    tab = fep.transfer_tables(t)
    ep, n_np, ech, n_nc, _, _ = tc.raised('pair-10', t)
    ep, ech, par = ep.astype(np.int32), ech.astype(np.int32), c['parent'].astype(np.int32)
    cor, soc, W, near = c['corners'], tab['shape_of_code'], tab['W'], tab['near']
    n_e, n_child = 2, par.size
    u, q = tc.nodal_field(n_np, 2), tc.point_field(4, n_e * 7)
    ptr = fep._lib.ptr
    lib = fep.lib()

    def nodes(elem_type=2, n_comp=2, counts=None, null=None, out=None):
        o = np.full((n_nc, n_comp if 1 <= n_comp <= 4 else 2), -7.5) if out is None else out
        args = [ptr(ep), ptr(ech), ptr(par), ptr(cor), ptr(soc), ptr(W), ptr(u), ptr(o)]
        if null is not None:
            args[null] = None
        rc = lib.fep_transfer_nodes_host(DEV, elem_type, n_comp, *(counts or (n_e, n_np, n_child, n_nc)), *args)
        return rc, bool((o == -7.5).all())

    def points(elem_type=2, n_rows=4, counts=None, null=None):
        o = np.full((max(n_rows, 1), n_child * 7), -7.5)
        args = [ptr(par), ptr(cor), ptr(soc), ptr(near), ptr(q), ptr(o)]
        if null is not None:
            args[null] = None
        rc = lib.fep_transfer_points_host(DEV, elem_type, n_rows, *(counts or (n_e, n_child)), *args)
        return rc, bool((o == -7.5).all())

    for elem_type in (0, 3, 4, 6):                                                     # Q1 and Q2 have no marked refinement
        assert nodes(elem_type=elem_type) == (EINVAL, True) and points(elem_type=elem_type) == (EINVAL, True)
    for n_comp in (0, 5, -1):
        assert nodes(n_comp=n_comp) == (EINVAL, True)
    for n_rows in (0, -2):
        assert points(n_rows=n_rows) == (EINVAL, True)
    for k in range(4):
        counts = [n_e, n_np, n_child, n_nc]
        counts[k] = -1
        assert nodes(counts=counts) == (EINVAL, True)
    assert points(counts=(-1, n_child)) == (EINVAL, True) and points(counts=(n_e, -1)) == (EINVAL, True)
    for null in range(8):
        assert nodes(null=null) == (EINVAL, True), null
    for null in range(6):
        assert points(null=null) == (EINVAL, True), null
    # an output that shares bytes with an input: the tail of u
    before = u.copy()
    rc = lib.fep_transfer_nodes_host(DEV, 2, 2, n_e, n_np, n_child, 1, ptr(ep), ptr(ech), ptr(par), ptr(cor), ptr(soc), ptr(W), ptr(u),
                                     ptr(u[n_np - 1:]))
    assert rc == EINVAL and u.tobytes() == before.tobytes()
    before = q.copy()
    rc = lib.fep_transfer_points_host(DEV, 2, 1, n_e, 1, ptr(par), ptr(cor), ptr(soc), ptr(near), ptr(q), ptr(q[0, 7:]))
    assert rc == EINVAL and q.tobytes() == before.tobytes()
    # the _dev forms, and the corner codes before any mark
    dev_out = torch.full((n_nc, 2), -7.5, dtype=torch.float64, device=f'cuda:{DEV}')
    d = [_t(a) for a in (ep, ech, par, cor, soc, W, u)]
    p = [C.c_void_p(a.data_ptr()) for a in d]
    assert lib.fep_transfer_nodes_dev(DEV, None, 3, 2, n_e, n_np, n_child, n_nc, *p, C.c_void_p(dev_out.data_ptr())) == EINVAL
    assert lib.fep_transfer_nodes_dev(DEV, None, 2, 2, n_e, n_np, n_child, n_np, *p, p[6]) == EINVAL              # u_child = u
    torch.cuda.synchronize()
    assert bool((dev_out == -7.5).all()) and d[6].cpu().numpy().tobytes() == u.tobytes()
    with fep.DeviceMesh(mc.PAIR_COORD, mc.PAIR_ELEM, DEV) as m:
        canary = np.full((3, 7), 99, dtype=np.uint8)
        assert lib.fep_mesh_child_corners_host(m._h, ptr(canary)) == ESTATE and (canary == 99).all()
        dev_canary = torch.full((3, 7), 99, dtype=torch.uint8, device=f'cuda:{DEV}')
        assert lib.fep_mesh_child_corners_dev(m._h, None, C.c_void_p(dev_canary.data_ptr())) == ESTATE
        m.mark([1, 0])
        assert lib.fep_mesh_child_corners_host(m._h, None) == EINVAL and lib.fep_mesh_child_corners_dev(m._h, None, None) == EINVAL
        torch.cuda.synchronize()
        assert bool((dev_canary == 99).all())
        assert m.child_corners().tobytes() == c['corners'].tobytes()
    assert lib.fep_mesh_child_corners_host(None, ptr(canary)) == EINVAL
    # a valid call on the same device still passes
    assert nodes() == (0, False) and points() == (0, False)


# ---- graph replay -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ('P1', 'P4'))
def test_graph_replay(fep, twin, t):
    """One warm call (it makes the owner scratch of the stream), then the same calls captured on a single stream and replayed
    on other inputs: the twin's bytes."""
    import torch
    name = 'tunnel-curved'
    c = tc.case(name)
    ep, n_np, ech, n_nc, _, _ = tc.raised(name, t)
    ep_d, ech_d, par_d, cor_d = _t(ep, np.int32), _t(ech, np.int32), _t(c['parent'], np.int32), _t(c['corners'])
    u, want_u = twin('nodes', name, t, 2)
    q, want_q = twin('points', name, t, 4)
    u_d, q_d = torch.zeros_like(_t(u)), torch.zeros_like(_t(q))
    out_u = torch.empty((n_nc, 2), dtype=torch.float64, device=f'cuda:{DEV}')
    out_q = torch.empty((4, c['parent'].size * tc.N_Q[t]), dtype=torch.float64, device=f'cuda:{DEV}')
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        fep.transfer_nodes_dev(t, ep_d, ech_d, par_d, cor_d, u_d, n_nc, out=out_u)          # warm: on the capture's stream
        fep.transfer_points_dev(t, par_d, cor_d, q_d, out=out_q)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fep.transfer_nodes_dev(t, ep_d, ech_d, par_d, cor_d, u_d, n_nc, out=out_u)
        fep.transfer_points_dev(t, par_d, cor_d, q_d, out=out_q)
    u_d.copy_(_t(u))
    q_d.copy_(_t(q))
    out_u.fill_(-1.0)
    out_q.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    assert out_u.cpu().numpy().tobytes() == want_u.tobytes() and out_q.cpu().numpy().tobytes() == want_q.tobytes()


# ---- footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', TYPES)
def test_footprint_of_the_dev_forms(fep, twin, t):
    """All outputs written, guards and inputs intact, and the result independent of what the memory held."""
    import torch
    name = 'tunnel-curved'
    c = tc.case(name)
    ep, n_np, ech, n_nc, _, _ = tc.raised(name, t)
    u, want_u = twin('nodes', name, t, 2)
    q, want_q = twin('points', name, t, 4)
    n_child = c['parent'].size
    for fill in (0xFF, 0x00):
        arena = fp.Arena(f'cuda:{DEV}', fill=fill)
        ins = [arena.put(a, name=n) for n, a in (('elem_parent', ep.astype(np.int32)), ('elem_child', ech.astype(np.int32)),
                                                 ('parent', c['parent'].astype(np.int32)), ('corners', c['corners']), ('u', u), ('q', q))]
        out_u = arena.take((n_nc, 2), torch.float64, name='u_child')
        out_q = arena.take((4, n_child * tc.N_Q[t]), torch.float64, name='q_child')
        out_c = arena.take((3, n_child), torch.uint8, name='corners_out')
        (ep_d, _), (ech_d, _), (par_d, _), (cor_d, _), (u_d, _), (q_d, _) = ins
        fep.transfer_nodes_dev(t, ep_d, ech_d, par_d, cor_d, u_d, n_nc, out=out_u)
        fep.transfer_points_dev(t, par_d, cor_d, q_d, out=out_q)
        with fep.DeviceMesh(c['coord'], c['elem'], DEV) as m:
            m.mark(c['marked'])
            rc = fep.lib().fep_mesh_child_corners_dev(m._h, m._stream(), C.c_void_p(out_c.data_ptr()))
            torch.cuda.synchronize()
        assert rc == 0
        assert fp.guards_intact(arena)
        for (view, snap), n in zip(ins, ('elem_parent', 'elem_child', 'parent', 'corners', 'u', 'q')):
            assert fp.unchanged(view, snap, n)
        if fill == 0xFF:
            assert fp.fully_written(out_u, name='u_child') and fp.fully_written(out_q, name='q_child')
            assert fp.fully_written(out_c, name='corners')
        assert out_u.cpu().numpy().tobytes() == want_u.tobytes() and out_q.cpu().numpy().tobytes() == want_q.tobytes()
        assert out_c.cpu().numpy().tobytes() == c['corners'].tobytes()


# ---- the drivers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver,tol', [('direct', 1e-10), ('amg', 1e-9)])                   # the tolerances of test_vm_gpu.py
def test_cyclic_driver_with_a_refinement_against_the_cpu_run(fep, solver, tol):
    """'direct' carries host arrays through the *_host forms, 'amg' device tensors through the *_dev forms.  Marks by geometry,
    so that a rounding difference cannot flip one."""
    from conftest import relerr
    ref = tc.cpu_adaptive_cycle()
    r = fep.solve_cutout_cyclic('P1', level=0, linear_solver=solver, adapt_at=(3,), mark=tc.near_corner)
    assert ref['failed_at'] is None and r['failed_at'] is None and r['zeta'] == ref['zeta'] and len(r['zeta']) == 17
    a, b = r['adapt'][0], ref['adapt'][0]
    for k in ('step', 'n_e', 'n_n', 'n_marked', 'n_child', 'eta', 'equilibration'):
        assert a[k] == b[k], k
    for k in ('parent', 'corners', 'coords', 'elem'):
        assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype, k
    assert relerr(r['f_ext'], ref['f_ext']) <= 1e-14 and r['n_plast'] == ref['n_plast']
    for k, (U, Ur) in enumerate(zip(r['U'], ref['U'])):
        assert U.shape == Ur.shape and relerr(U, Ur) <= tol, k
    assert relerr(a['U'], b['U']) <= tol and relerr(a['Ep'], b['Ep']) <= tol and relerr(a['s'], b['s']) <= tol
    assert relerr(r['Ep'], ref['Ep']) <= tol and abs(r['work'] - ref['work']) <= tol * abs(ref['work'])
    assert (r['pcg_iters'] is None) == (solver == 'direct')
    gap = tc.stress_gap(a, fep.MeshContext)
    print('stress gap', solver, gap)
    assert gap <= tc.STRESS_TOL_GPU


def test_cyclic_driver_marks_by_the_indicator(fep):
    r = fep.solve_cutout_cyclic('P1', level=0, linear_solver='amg', adapt_at=(3, 7), mark='zz', theta=0.5)
    assert r['failed_at'] is None and len(r['zeta']) == 18 and [row['step'] for row in r['adapt']] == [3, 7]
    for row in r['adapt']:
        assert row['n_child'] > row['n_e'] and row['n_marked'] > 0 and row['eta'] > 0
    assert r['adapt'][1]['n_e'] == r['adapt'][0]['n_child'] and r['U'][-1].shape == (2, r['adapt'][1]['coords'].shape[1])


def test_tsx_materials_go_along(fep):
    """Two layers on P2, on the GPU: the next round's material arrays are transfer_points_np of the round's."""
    coord, elem = mc.tunnel()
    upper = np.repeat(coord[1][elem].mean(axis=0) > 0, 7)
    mats = (np.where(upper, 25000.0, 30000.0), np.where(upper, 100000.0 / 3, 40000.0), 0.3, 12.0)
    h = fep.solve_tsx_tunnel(coord, elem, 'P2', adapt=1, mark=mc.near_tunnel, materials=mats, transfer_materials=True, n_load_steps=4,
                             curves=[fep.tsx_tunnel.TSX_HOLE])
    a, b = h['adapt']
    assert b['n_e'] == a['n_child'] > a['n_e'] and a['corners'].shape == (3, a['n_child'])
    for i in (0, 1):
        want = fep.transfer_points_np('P2', a['parent'], a['corners'], a['materials'][i])
        assert b['materials'][i].tobytes() == want.tobytes() and set(np.unique(want)) == set(np.unique(mats[i]))
        assert np.array_equal(want, np.repeat(a['materials'][i][::7][a['parent']], 7))      # a child is of its parent's layer
    assert b['materials'][2:] == (0.3, 12.0) and abs(h['zeta'][-1] - 1) < 1e-12

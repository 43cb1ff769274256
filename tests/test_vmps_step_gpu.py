"""The step of a plane-stress von Mises context (fep_api.hip: the staged plan of run_step with p1_point_vmps_kernel / point_vmps_kernel<NP, NQ>
and the context's own assembly) on every element type and route, the closed forms through the whole stack, and the cyclic
driver with `plane_stress=True`.

The per-entry comparison is that of test_model_step_routes_gpu.py with its bounds as they are (tests/elem_ref.py,
test_element_route_gpu.C_E / C_K / C_F; DESIGN.md section 7: 1e-13 of the array maximum and 1e-12 per point for s, ds, ep): E
against ElemRef.strain(U), the point outputs against the restatement (tests/vmps_ref.py) applied to the KERNEL's E, K and F
against ElemRef.assemble of the KERNEL's ds and s.  Cases: vmps_cases.build, the meshes and flags of model_step_cases."""
import functools
from importlib import import_module

import numpy as np
import pytest
import scipy.sparse as ssp
import scipy.sparse.linalg as spla

import exact_cases as xc
import model_step_cases as msc
import vmps_cases as vc
from conftest import relerr, relerr_points
from e0_field_ref import z_of
from elem_ref import ElemRef, ratio
from footprint import scrub
from routes import assert_route
from test_element_route_gpu import C_E, C_F, C_K, C_RECORD
from vmps_ref import VMPSRefContext, vmps_return_map

pytestmark = pytest.mark.gpu

TOL, TOL_PT = 1e-13, 1e-12
EVERY = ('E', 's', 'ds', 'ind_p', 'K', 'F')
CASES = [(t, r, n) for t in msc.TYPES for r in msc.ROUTES[t] for n in vc.STEP_NAMES]


def _same(a, b, keys=('E', 's', 'ds', 'ind_p', 'F')):
    return all(np.array_equal(a[k], b[k]) for k in keys) and np.array_equal(a['K'].data, b['K'].data) \
        and (a['n_smooth'], a['n_apex']) == (b['n_smooth'], b['n_apex'])


def _context(fep, monkeypatch, route, elem, coord):
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    ctx = fep.MeshContext(elem, coord)
    assert_route(ctx, 'patch' if route == 'default' else route)
    return ctx


def _check_points(full, ep, Ep, mats, z, accept, what):
    """Stage 2: the point outputs against the restatement on the kernel's strain (z: e0 (4, 1), per point (4, n), or None)."""
    o = vmps_return_map(full['E'], Ep, *mats, apply_plastic_strain=accept, e0=z)
    excl = np.abs(o['crit']) < vc.VM_CRIT_FLOOR * np.asarray(mats[3])
    keep = ~excl
    assert excl.mean() <= msc.MAX_EXCLUDED and 0.2 <= o['ind_p'].mean() <= 0.8, (excl.sum(), o['ind_p'].mean())
    assert np.array_equal(full['ind_p'][keep], o['ind_p'][keep])
    assert full['n_apex'] == 0 and full['n_smooth'] == int(full['ind_p'].sum())
    e_s = (relerr(full['s'], o['s']), relerr_points(full['s'], o['s']))
    e_ds = (relerr(full['ds'][:, keep], o['ds'][:, keep]), relerr_points(full['ds'][:, keep], o['ds'][:, keep]))
    print(f'[points] {what}: left out {int(excl.sum())}, s {e_s[0]:.1e} / {e_s[1]:.1e}, ds {e_ds[0]:.1e} / {e_ds[1]:.1e}')
    assert e_s[0] <= TOL and e_s[1] <= TOL_PT and e_ds[0] <= TOL and e_ds[1] <= TOL_PT
    assert not full['s'][3].any()
    if accept:
        e_p = (relerr(ep, o['ep']), relerr_points(ep, o['ep']))
        print(f'[points] ep {e_p[0]:.1e} / {e_p[1]:.1e}')
        assert e_p[0] <= TOL and e_p[1] <= TOL_PT and not np.array_equal(ep, Ep)
    else:
        assert np.array_equal(ep, Ep)


def _check_assembly(t, route, full, elem, coord, tab, pattern, what):
    """Stage 3: K and F against the float64 assembly of the kernel's ds and s, per entry."""
    ref = ElemRef(elem, coord, tab, pattern=pattern)
    if route == 'node':
        rec = ElemRef(elem, coord, tab, pattern=pattern, record=True)
        K, S_K, F, S_F = rec.assemble(full['ds'], full['s'])
        Kx, W_K, Fx, W_F = ref.assemble(full['ds'], full['s'], widened=True)
        x_K, x_F = ratio(full['K'].data, Kx, W_K), ratio(full['F'], Fx, W_F)
        assert x_K <= C_K[t] + C_RECORD and x_F <= C_F[t] + C_RECORD, (x_K, x_F)
    else:
        K, S_K, F, S_F = ref.assemble(full['ds'], full['s'])
    r_K, r_F = ratio(full['K'].data, K, S_K), ratio(full['F'], F, S_F)
    print(f'[ratios] {what} K {r_K:.2f} F {r_F:.2f}')
    assert r_K <= C_K[t] and r_F <= C_F[t], (r_K, r_F)


# ---------------------------------------------------------------------------------------
# 11: the step, per entry, on every route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t,route,name', CASES)
def test_step_vs_reference_per_entry(fep, monkeypatch, t, route, name):
    c = vc.build(t, name)
    elem, coord, U, Ep, mats, e0, accept = (c[k] for k in ('elem', 'coord', 'U', 'ep', 'mats', 'e0', 'accept'))
    what = f'vmps {t} {route} {name}'
    ctx = _context(fep, monkeypatch, route, elem, coord)
    try:
        n_int = ctx.n_int
        ctx.set_model('vmps')
        ctx.set_materials(*mats)
        tag = 'p1_point_vmps_kernel' if t == 'P1' else f'point_vmps_kernel<{elem.shape[0]}, {msc.NQ[t]}>'
        assert ctx.model == 'vmps' and ctx.kernel_names(0).startswith(tag) and ctx.kernel_names(1).startswith(tag)
        kw = {} if e0 is None else {'e0': e0}
        ep = Ep.copy()
        if accept:
            scrub(ctx, U, Ep, kw)
        full = ctx.step(U, ep, apply_plastic_strain=accept, want=EVERY, **kw)
        scrub(ctx, U, Ep, kw)
        kf = ctx.step(U, Ep.copy(), want=('K', 'F'), **kw)
        scrub(ctx, U, Ep, kw)
        pts = ctx.step(U, Ep.copy(), want=('s', 'ds', 'ind_p'), **kw)
        scrub(ctx, U, Ep, kw)
        K2, F2 = ctx.assemble(full['ds'], full['s'])
        none = ctx.step(U, None, want=EVERY, **kw)
        zero = ctx.step(U, np.zeros((4, n_int)), want=EVERY, **kw)
        pattern = ctx.pattern()
    finally:
        ctx.close()
    # the output subsets and the _host form's own scratch: bit for bit the full-output step
    assert np.array_equal(kf['K'].data, full['K'].data) and np.array_equal(kf['F'], full['F'])
    assert all(np.array_equal(pts[k], full[k]) for k in ('s', 'ds', 'ind_p'))
    assert np.array_equal(K2.data, full['K'].data) and np.array_equal(F2, full['F'])
    assert _same(none, zero)
    for r in (kf, pts):
        assert (r['n_smooth'], r['n_apex']) == (full['n_smooth'], full['n_apex'])
    tab = fep.element_tables(t)
    E, S_E = ElemRef(elem, coord, tab, pattern=pattern).strain(U)
    r_E = ratio(full['E'], E, S_E)
    print(f'[E] {what}: ratio {r_E:.2f}')
    assert r_E <= C_E[t]
    _check_points(full, ep, Ep, mats, e0, accept, what)
    _check_assembly(t, route, full, elem, coord, tab, pattern, what)


def _step_dev(ctx, U, Ep, accept=False, e0=None, field=None, scale=1.0, graph=False):
    """fep_step_dev / fep_step_field_dev on torch tensors, directly or as one replay of a captured graph -> the dict of a step."""
    import torch
    dev = torch.device('cuda', 0)
    f64 = dict(dtype=torch.float64, device=dev)
    n = ctx.n_int
    Ud = torch.from_numpy(np.ascontiguousarray(np.asarray(U).reshape(-1, order='F'))).to(dev)
    Epd = torch.from_numpy(np.array(Ep)).to(dev)
    fd = None if field is None else torch.from_numpy(np.ascontiguousarray(field)).to(dev)
    o = {'e_out': torch.zeros((3, n), **f64), 's': torch.zeros((4, n), **f64), 'ds': torch.zeros((9, n), **f64),
         'ind_p': torch.zeros(n, dtype=torch.uint8, device=dev), 'k_data': torch.zeros(ctx.nnz, **f64),
         'f_out': torch.zeros(ctx.n_dof, **f64), 'counts': torch.zeros(2, dtype=torch.int64, device=dev)}

    def call():
        ctx.step_dev(torch.cuda.current_stream().cuda_stream, Ud.data_ptr(), ep=Epd.data_ptr(), accept=accept, e0=e0,
                     e0_field=None if fd is None else fd.data_ptr(), e0_scale=scale, **{k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for v in o.values():
            v.zero_()
        Epd.copy_(torch.from_numpy(np.array(Ep)).to(dev))               # the capture ran nothing; the replay is the one run
        g.replay()
    else:
        call()
    torch.cuda.synchronize()
    cnt = o['counts'].cpu().numpy()
    return {'E': o['e_out'].cpu().numpy(), 's': o['s'].cpu().numpy(), 'ds': o['ds'].cpu().numpy(),
            'ind_p': o['ind_p'].cpu().numpy().astype(bool), 'K': o['k_data'].cpu().numpy(), 'F': o['f_out'].cpu().numpy(),
            'n_smooth': int(cnt[0]), 'n_apex': int(cnt[1]), 'ep': Epd.cpu().numpy()}


@pytest.mark.parametrize('t,route', [('P1', 'node'), ('Q2', 'default'), ('P2', 'coo')])
def test_dev_and_host_forms_agree_and_a_captured_graph_replays_the_step(fep, monkeypatch, t, route):
    """fep_step_dev = fep_step_host bit for bit, accepting and not, and one replay of the captured launch sequence = the direct
    launch bit for bit (fep_ctx_set_model allocated the scratch: nothing is allocated during the capture).  The process keeps
    the default number of hardware queues."""
    c = vc.build(t, 'block257')
    ctx = _context(fep, monkeypatch, route, c['elem'], c['coord'])
    try:
        ctx.set_model('vmps')
        ctx.set_materials(*c['mats'])
        for accept in (False, True):
            ep = c['ep'].copy()
            host = ctx.step(c['U'], ep, e0=c['e0'], apply_plastic_strain=accept, want=EVERY)
            direct = _step_dev(ctx, c['U'], c['ep'], accept, c['e0'])
            replay = _step_dev(ctx, c['U'], c['ep'], accept, c['e0'], graph=True)
            assert 0 < host['n_smooth'] < ctx.n_int
            for got in (direct, replay):
                for k in ('E', 's', 'ds', 'ind_p', 'F'):
                    assert np.array_equal(got[k], host[k]), (accept, k)
                assert np.array_equal(got['K'], host['K'].data) and np.array_equal(got['ep'], ep)
                assert (got['n_smooth'], got['n_apex']) == (host['n_smooth'], 0)
    finally:
        ctx.close()


@pytest.mark.parametrize('t,route', [(t, r) for t in msc.TYPES for r in msc.ROUTES[t]])
def test_field_step_vs_reference_per_entry(fep, monkeypatch, t, route):
    """step(e0_field=, e0_scale=): point k runs on e0 + e0_scale * e0_field[:, k] (e0_field_ref.z_of applied to the restatement);
    host and device forms bit-equal; a field whose columns all equal z is the plain step with e0 = z."""
    c = vc.build(t, 'block257')
    elem, coord, U, Ep, mats = (c[k] for k in ('elem', 'coord', 'U', 'ep', 'mats'))
    rng = np.random.default_rng(msc.seed('vmps field', t, route))
    n = Ep.shape[1]
    y = vc.YIELD / (2 * vc.SHEAR)
    field, scale, e0 = y * rng.normal(0, 0.2, size=(4, n)), 0.37, y * rng.normal(0, 0.2, size=(4, 1))
    zc = y * rng.normal(0, 0.2, size=(4, 1))
    what = f'vmps field {t} {route}'
    ctx = _context(fep, monkeypatch, route, elem, coord)
    try:
        ctx.set_model('vmps')
        ctx.set_materials(*mats)
        ep = Ep.copy()
        full = ctx.step(U, ep, e0=e0, apply_plastic_strain=True, want=EVERY, e0_field=field, e0_scale=scale)
        dev = _step_dev(ctx, U, Ep, True, e0, field, scale)
        kf = ctx.step(U, Ep.copy(), e0=e0, want=('K', 'F'), e0_field=field, e0_scale=scale)
        const = ctx.step(U, Ep.copy(), want=EVERY, e0_field=np.repeat(zc, n, axis=1), e0_scale=1.0)
        plain = ctx.step(U, Ep.copy(), want=EVERY, e0=zc)
        nofield = ctx.step(U, Ep.copy(), e0=e0, want=EVERY)
        pattern = ctx.pattern()
    finally:
        ctx.close()
    for k in ('E', 's', 'ds', 'ind_p', 'F'):
        assert np.array_equal(dev[k], full[k]), k
    assert np.array_equal(dev['K'], full['K'].data) and np.array_equal(dev['ep'], ep) and dev['n_smooth'] == full['n_smooth']
    assert np.array_equal(kf['K'].data, full['K'].data) and np.array_equal(kf['F'], full['F'])
    assert _same(const, plain) and not np.array_equal(nofield['s'], full['s'])
    _check_points(full, ep, Ep, mats, z_of(e0, field, scale), True, what)
    _check_assembly(t, route, full, elem, coord, fep.element_tables(t), pattern, what)


# ---------------------------------------------------------------------------------------
# 10: the kernels share the return map
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'Q1'])
def test_point_kernels_share_the_return_map(fep, monkeypatch, t):
    """The mesh-free kernel fed a step's E reproduces the step's s, ds, ind_p, counters and ep byte for byte (257 elements: two
    workgroups and more, the last one partial)."""
    c = vc.build(t, 'block257')
    elem, coord, U, ep = c['elem'], c['coord'], c['U'], c['ep']
    rng = np.random.default_rng(5)
    _, _, mats, e0 = vc.state(t, elem, coord, rng)                      # per-point materials and an initial strain
    ctx = _context(fep, monkeypatch, 'node' if t == 'P1' else 'default', elem, coord)
    try:
        ctx.set_model('vmps')
        ctx.set_materials(*mats)
        assert ctx.n_int > 256 and ctx.n_int % 256 != 0
        for accept in (False, True):
            ep_step = ep.copy()
            step = ctx.step(U, ep_step, e0=e0, apply_plastic_strain=accept, want=EVERY)
            free = vc.dev_return_map(step['E'], 'C', ep, e0, mats, accept)
            assert 0.2 <= step['ind_p'].mean() <= 0.8
            for k in ('s', 'ds', 'ind_p'):
                assert np.array_equal(free[k], step[k]), k
            assert (free['n_smooth'], free['n_apex']) == (step['n_smooth'], step['n_apex'])
            assert np.array_equal(free['ep'], ep_step) and np.array_equal(ep_step, ep) == (not accept)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# 14: what the step forms write
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t,route', [('P1', 'node'), ('P2', 'default'), ('P2', 'coo'), ('Q2', 'default')])
def test_step_forms_write_their_outputs_and_nothing_else(fep, monkeypatch, t, route):
    """The forms of test_footprint_gpu.py (every output, K,F-only, accepting, assemble) and the field step on tests/footprint.py
    arenas: every output element written, guards and inputs intact, every form the bits of the full-output one."""
    from test_footprint_gpu import _all_forms
    c = vc.build(t, 'block257')
    ctx = _context(fep, monkeypatch, route, c['elem'], c['coord'])
    try:
        ctx.set_model('vmps')
        ctx.set_materials(*c['mats'])
        e0 = None if c['e0'] is None else np.ascontiguousarray(c['e0']).ravel()
        A = _all_forms(ctx, f'vmps {t} {route}', c['U'], c['ep'], e0=e0, forms='ABFH')
        assert 0 < int(A['ind_p'].sum()) < ctx.n_int
        rng = np.random.default_rng(14)
        field = vc.YIELD / (2 * vc.SHEAR) * rng.normal(0, 0.2, size=(4, ctx.n_int))
        A = _all_forms(ctx, f'vmps field {t} {route}', c['U'], c['ep'], e0=e0, forms='AB', field=field, scale=0.37)
        assert 0 < int(A['ind_p'].sum()) < ctx.n_int
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# 15 (a): uniaxial tension through the whole stack
# ---------------------------------------------------------------------------------------
SIGMAS = (300.0, 440.0, 520.0, 600.0)                                   # two elastic steps, two past sigma_y = 450
SIZE = (4.0, 2.0)
# the CPU restatement's run of the same loop against the closed form, per type: max over the steps of |U - U_exact| / max|U_exact|
# (tests/vmps_ref.py, SuperLU), rounded up to two digits; the bound of the GPU run is eight times it
UNIAXIAL_CPU = {'P1': 8.1e-16, 'P2': 5.4e-16, 'Q1': 1.1e-15, 'Q2': 9.7e-16, 'P4': 1.3e-15}


def _uniaxial_problem(fep, t):
    """The 2 x 2 cell rectangle, u_x = 0 on x = 0 and u_y = 0 on y = 0, the unit traction in x on the side x = 4: its load
    vector is the internal force of the uniform unit stress (1, 0, 0) at the free DOFs (the divergence theorem; the elements
    are affine and the tables integrate the shape functions' derivatives exactly), summed on the host."""
    from meshes import rect
    elem, coord = rect(t, 2, 2, *SIZE)
    ref = VMPSRefContext(elem, coord, *fep.element_tables(t))
    ref.set_materials(*vc.UNIFORM)
    f = ref.orc.internal_force(ref.c['B'], ref.c['weight'], np.array([[1.0], [0.0], [0.0], [0.0]]) * np.ones((1, ref.n_int)))
    free = np.stack([coord[0] != 0, coord[1] != 0])
    f = np.where(free.flatten(order='F'), np.asarray(f).ravel(), 0.0)
    exact = []
    for s in SIGMAS:
        e = vc.uniaxial(s)[0] if s > vc.SIGMA_Y else np.array([s / vc.YOUNG, -vc.POISSON * s / vc.YOUNG, 0.0])
        exact.append(np.stack([e[0] * coord[0], e[1] * coord[1]]))
    return elem, coord, free, f, exact, ref.n_int


def _uniaxial_run(fep, t, make):
    """The cyclic driver's loop (newton._load_history_loop, direct solve) on the load factors SIGMAS -> (U per step, n_plast)."""
    newton = import_module(fep.__name__ + '.newton')
    elem, coord, free, f, exact, n_int = _uniaxial_problem(fep, t)
    ctx = make(elem, coord, *fep.element_tables(t))
    ctx.set_model('vmps')
    ctx.set_materials(*vc.UNIFORM)
    hist = {'zeta': [], 'U': [], 'n_plast': [], 'n_calls': 0}
    ops = newton.make_ops(ctx, free.flatten(order='F'), 'direct', 1e-11)
    try:
        K_elast = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']

        def accepted(r, zeta, U, its):
            hist['U'].append(ops.host(U).reshape((2, -1), order='F').copy())
            hist['n_plast'].append(int(r['n_smooth']))
        newton._load_history_loop(ops, K_elast, ops.vec(f), SIGMAS, hist, accepted=accepted)
    finally:
        ops.close()
        ctx.close()
    assert hist['failed_at'] is None
    err = max(np.abs(U - Ux).max() / np.abs(Ux).max() for U, Ux in zip(hist['U'], exact))
    return err, hist['n_plast'], n_int


@functools.lru_cache(maxsize=None)
def _uniaxial_cpu(t):
    return _uniaxial_run(vc.fep, t, VMPSRefContext)


@pytest.mark.parametrize('t', msc.TYPES)
def test_uniaxial_tension_is_the_closed_form(fep, t):
    """U is the linear field of the closed form at every node after each of the four steps, and every point is plastic after
    yield.  The CPU restatement's error is re-measured here and has to be the recorded figure."""
    cpu, n_plast_cpu, n_int = _uniaxial_cpu(t)
    err, n_plast, _ = _uniaxial_run(fep, t, lambda *a: fep.MeshContext(*a))
    bound = vc.MARGIN * UNIAXIAL_CPU[t]
    print(f"'{t}': {cpu:.1e}   GPU {err:.1e} (<= {bound:.1e})")
    assert cpu <= UNIAXIAL_CPU[t] <= 2 * cpu + 1e-17
    assert n_plast == n_plast_cpu == [0, 0, n_int, n_int]
    assert err <= bound


# ---------------------------------------------------------------------------------------
# 15 (b): the elastic Lame ring in plane stress
# ---------------------------------------------------------------------------------------
LAME_CASES = ('P1 ring, pressure', 'P2 ring, pressure', 'P4 ring, pressure', 'Q1 rect', 'Q2 rect')


def lame_plane_stress(coord, centre):
    """u_r = ((1 - nu) A r + (1 + nu) B / r) / E, A = p a^2 / (b^2 - a^2), B = A b^2: the thick-walled cylinder with free ends."""
    dx, dy = coord[0] - centre[0], coord[1] - centre[1]
    r = np.hypot(dx, dy)
    A = xc.PRESSURE * xc.A_IN ** 2 / (xc.B_OUT ** 2 - xc.A_IN ** 2)
    B = A * xc.B_OUT ** 2
    ur = ((1 - xc.NU) * A * r + (1 + xc.NU) * B / r) / xc.YOUNG
    return np.stack([ur * dx / r, ur * dy / r])


@pytest.mark.parametrize('name', LAME_CASES)
def test_elastic_lame_field_in_plane_stress_converges_at_the_order_of_the_element(fep, name):
    """K is the 'vmps' context's K at U = 0 with a yield stress nothing reaches (the elastic plane-stress stiffness).  The two
    finest levels of the exact_cases case (ring meshes for the triangles with the pressure on the inner wall; the unit square
    off the axis with the field on its boundary for Q1 and Q2): exact_cases' order rule on the GPU's own errors."""
    c = xc.CASES[name]
    errs = []
    for level in c['levels'][-2:]:
        m = xc.mesh(fep, c['kind'], c['et'], level, device=None)
        xc.check_mesh(c, level, m)
        ctx = fep.MeshContext(m['elem'], m['coord'], *xc.tables(fep, c))
        try:
            ctx.set_model('vmps')
            ctx.set_materials(xc.SHEAR, xc.BULK, 0.0, 1e30)
            r = ctx.step(np.zeros(ctx.n_dof), want=('K',))
            assert (r['n_smooth'], r['n_apex']) == (0, 0)
            K = ssp.csr_matrix(r['K'])
        finally:
            ctx.close()
        f = np.zeros(K.shape[0])
        if c['load'] == 'pressure':
            edges, tr, (hat, dhat, wf) = xc.wall_traction(m, c['et'])
            f = xc.flat(np.asarray(fep.load_traction(edges, m['coord'], tr, hat, dhat, wf)))
        fixed = xc.dof_mask(m['fixed'][c['load']])
        u = xc.flat(lame_plane_stress(m['coord'], m['centre']))
        U = np.where(fixed, u, 0.0)
        free = np.flatnonzero(~fixed)
        U[free] = spla.splu(ssp.csc_matrix(K[free][:, free])).solve((f - K @ U)[free])
        e = U - u
        errs.append((float(np.abs(e).max() / np.abs(u).max()), float(np.sqrt((e @ (K @ e)) / (u @ (K @ u))))))
    o_max, o_en = xc.orders(errs)[0]
    least_max, least_en = xc.rule(name)
    print(f'{name}: errors {errs}, orders {o_max:.2f} {o_en:.2f} (>= {least_max}, {least_en})')
    assert o_max >= least_max and o_en >= least_en


# ---------------------------------------------------------------------------------------
# 16: the driver
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_cycle():
    from vm_cases import top_load
    return vc.fep.solve_cutout_cyclic('P1', level=0, context_factory=VMPSRefContext, linear_solver='direct',
                                      f_ext=top_load('P1', 0, (0, 200.0)), plane_stress=True)


def test_cyclic_driver_in_plane_stress(fep):
    """plane_stress=True against the same call on the CPU restatement with the direct solve; it is another problem than plane
    strain; plane_stress=False is the call without the keyword bit for bit."""
    from vm_cases import cpu_cycle
    ref = _cpu_cycle()
    assert ref['failed_at'] is None and max(ref['n_plast']) > 0
    r = fep.solve_cutout_cyclic('P1', level=0, linear_solver='direct', plane_stress=True)
    assert r['failed_at'] is None and r['zeta'] == ref['zeta'] and r['n_plast'] == ref['n_plast']
    for k, (U, Ur) in enumerate(zip(r['U'], ref['U'])):
        print(k, relerr(U, Ur))
        assert relerr(U, Ur) <= 1e-9, k
    assert relerr(r['Ep'], ref['Ep']) <= 1e-9 and abs(r['work'] - ref['work']) <= 1e-9 * abs(ref['work'])
    assert np.abs(r['Ep'][[0, 1, 3]].sum(axis=0)).max() <= 1e-14 * np.abs(r['Ep']).max()          # the plastic strain stays traceless
    strain = cpu_cycle('P1', 200.0)
    print('n_plast', r['n_plast'], strain['n_plast'], 'work', r['work'], strain['work'])
    assert r['n_plast'] != strain['n_plast'] or abs(r['work'] - strain['work']) > 1e-6 * abs(strain['work'])
    a = fep.solve_cutout_cyclic('P1', level=0, linear_solver='direct', plane_stress=False)
    b = fep.solve_cutout_cyclic('P1', level=0, linear_solver='direct')
    assert a['n_plast'] == b['n_plast'] and a['work'] == b['work'] and np.array_equal(a['Ep'], b['Ep'])
    assert all(np.array_equal(x, y) for x, y in zip(a['U'], b['U']))

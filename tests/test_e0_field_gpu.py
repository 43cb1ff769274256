"""
The initial strain per integration point (fep_step_field_*, fep_return_map_field_*, fep_ctx_point_coords_*) against the
element-by-element float64 reference (tests/elem_ref.py) and the models' restatements applied with the strain of each point
(tests/e0_field_ref.py), entry by entry; then solve_tsx_tunnel with `in_situ` / `body_force` end to end.

A step with a field runs staged for every model, Drucker-Prager too: p1_point_field_kernel<MODEL> / point_field_kernel<MODEL,
NP, NQ>, then what fep_assemble_dev launches for the route; the 'vmi' model (von Mises with isotropic hardening) through two
wrappers with names of their own, p1_point_vmi_field_kernel and point_vmi_field_kernel<NP, NQ>, which take the curve.  The cases (tests/e0_field_cases.py, decided on the CPU by
test_e0_field_host.py): dp, vm, mc, vmi (on the five curves of model_step_cases.py) x P1, P2, Q1, Q2, P4 x every route of the type x the block255 / block256 / block257 meshes
(n_int modulo the 256 lanes: 256 - NQ, 0, NQ) and one unstructured mesh; a field drawn independently in all four rows at
every point, in half of the cases beside a uniform e0 with scale = 0.37.

The three decoupled stages of test_model_step_routes_gpu.py, with its bounds as they are:
  1. E against ElemRef.strain within C_E; bit-equal to a plain Drucker-Prager step's E where that module asserts it
  2. s, ds, ind_p, the counters and the accepted ep against the restatement on the kernel's E: 1e-13 of the array maximum,
     1e-12 per point; points under the floors (at most 0.5 %) left out of flag / ds / counters
  3. K, F against ElemRef.assemble of the kernel's ds / s within C_K / C_F (C_RECORD on the node route)
and bit for bit: K,F-only / K-only / F-only = full output; ep_prev None = zeros; scale 0 with any finite field = a field of
zeros; a field whose columns all equal z (scale 1, no uniform part) = the plain step with e0 = z (vm, mc, vmi: every type and
route, in E, s, ds, ind_p, K, F and the counters: the return maps are compiled without contraction for this claim; dp: the P1
node route, whose plain full-output step runs the same point body; dp on the element routes, whose plain step forms its strain
in element_kernel, is held to stages 2 and 3 instead).
Containment: a NaN, and an infinity, at the last lane of workgroup 0 and at the first lane of workgroup 1.

End to end (direct solver): the K0 box at rest under its own weight, the uniform field against the reference's traces, a
depth-varying stress against the same driver on the CPU context.
K0 box, measured: test_k0_box_stays_at_rest's docstring and DESIGN.md section 7.
"""
import ctypes

import numpy as np
import pytest

import e0_field_cases as fcases
import e0_field_ref as fref
import loads_exact
from conftest import dp_materials, load_golden, relerr, relerr_points
from elem_ref import U_RND, ElemRef, ratio
from footprint import scrub
from routes import assert_route
from test_element_route_gpu import C_E, C_F, C_K, C_RECORD

pytestmark = pytest.mark.gpu

TOL, TOL_PT = 1e-13, 1e-12
EVERY = ('E', 's', 'ds', 'ind_p', 'K', 'F')
POINT_KEYS = ('s', 'ds', 'ind_p')


def _same(a, b, keys=('E', 's', 'ds', 'ind_p', 'F')):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys) and np.array_equal(a['K'].data, b['K'].data, equal_nan=True) \
        and (a['n_smooth'], a['n_apex']) == (b['n_smooth'], b['n_apex'])


def _context(fep, monkeypatch, c, model, route):
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    ctx = fep.MeshContext(c['elem'], c['coord'])
    assert_route(ctx, 'patch' if route == 'default' else route)
    return ctx


def _set_curve(ctx, model, curve):
    if model == 'vmi':
        tag = 'p1_point_vmi_kernel' if ctx.n_p == 3 else f'point_vmi_kernel<{ctx.n_p}, {ctx.n_q}>'
        assert ctx.kernel_names(0).startswith(tag + ' + '), ctx.kernel_names(0)
        if curve is not None:
            ctx.set_hardening(*curve)


def _check_points(model, got, ep_got, E, Ep, mats, z, accept, what, generator_conditions=True, curve=None):
    """Stage 2: the outputs of a step against the restatement on the kernel's strain E."""
    o = fref.return_map(model, E, Ep, mats, z, accept, curve=curve)
    excl = fcases.excluded(model, o, mats, curve)
    keep = ~excl
    if generator_conditions:
        fcases.check_conditions(model, o, excl, curve)
    assert excl.mean() <= fcases.MAX_EXCLUDED
    assert np.array_equal(got['ind_p'][keep], o['ind_p'][keep])
    assert got['n_smooth'] + got['n_apex'] == int(got['ind_p'].sum())
    if keep.all():
        assert (got['n_smooth'], got['n_apex']) == (o['n_smooth'], o['n_apex'])
    else:
        n_out = int(excl.sum())
        assert abs(got['n_smooth'] - o['n_smooth']) <= n_out and abs(got['n_apex'] - o['n_apex']) <= n_out
    e_s = (relerr(got['s'], o['s']), relerr_points(got['s'], o['s']))
    e_ds = (relerr(got['ds'][:, keep], o['ds'][:, keep]), relerr_points(got['ds'][:, keep], o['ds'][:, keep]))
    print(f'[points] {what}: left out {int(excl.sum())} of {excl.size}, s {e_s[0]:.1e} / {e_s[1]:.1e}, ds {e_ds[0]:.1e} / {e_ds[1]:.1e}')
    assert e_s[0] <= TOL and e_s[1] <= TOL_PT and e_ds[0] <= TOL and e_ds[1] <= TOL_PT
    if accept:
        e_p = (relerr(ep_got, o['ep']), relerr_points(ep_got, o['ep']))
        print(f'[points] ep {e_p[0]:.1e} / {e_p[1]:.1e}')
        assert e_p[0] <= TOL and e_p[1] <= TOL_PT
        assert not np.array_equal(ep_got, Ep)
        if model == 'vmi':                                              # kappa beside strains a thousandth of its size: each alone too
            for rows in (slice(0, 3), slice(3, 4)):
                assert relerr(ep_got[rows], o['ep'][rows]) <= TOL and relerr_points(ep_got[rows], o['ep'][rows]) <= TOL_PT
            el = ~got['ind_p'] & keep
            assert np.array_equal(ep_got[3][el], Ep[3][el]) and (ep_got[3] > Ep[3])[got['ind_p'] & keep].all()
    elif Ep is not None:
        assert np.array_equal(ep_got, Ep)


def _check_assembly(t, route, got, elem, coord, tab, pattern, what):
    """Stage 3: K and F of a step against ElemRef.assemble of its own ds and s."""
    ref = ElemRef(elem, coord, tab, pattern=pattern)
    if route == 'node':
        rec = ElemRef(elem, coord, tab, pattern=pattern, record=True)
        K, S_K, F, S_F = rec.assemble(got['ds'], got['s'])
        Kx, W_K, Fx, W_F = ref.assemble(got['ds'], got['s'], widened=True)
        x_K, x_F = ratio(got['K'].data, Kx, W_K), ratio(got['F'], Fx, W_F)
        assert x_K <= C_K[t] + C_RECORD and x_F <= C_F[t] + C_RECORD, (x_K, x_F)
    else:
        K, S_K, F, S_F = ref.assemble(got['ds'], got['s'])
    r_K, r_F = ratio(got['K'].data, K, S_K), ratio(got['F'], F, S_F)
    print(f'[ratios] {what}: K {r_K:.2f} F {r_F:.2f}')
    assert r_K <= C_K[t], ('K', r_K)
    assert r_F <= C_F[t], ('F', r_F)


@pytest.mark.parametrize('model,t,route,name', fcases.grid())
def test_field_step_vs_reference_per_entry(fep, monkeypatch, model, t, route, name):
    c = fcases.build(model, t, name)
    elem, coord, U, Ep, mats, e0, accept = (c[k] for k in ('elem', 'coord', 'U', 'ep', 'mats', 'e0', 'accept'))
    field, scale, curve = c['field'], c['scale'], c['curve']
    kw = dict(e0_field=field, e0_scale=scale, **({} if e0 is None else {'e0': e0}))
    rng = np.random.default_rng(fcases.seed(model, t, name) + 1)
    zc = fcases.eps_y(model) * rng.normal(0, 0.2, size=(4, 1))              # the constant field of the pin
    ctx = _context(fep, monkeypatch, c, model, route)
    try:
        n_int = ctx.n_int
        ctx.set_materials(*dp_materials(n_int))
        E_dp = ctx.step(U, np.zeros((4, n_int)), want=EVERY)['E'].copy()
        if model != 'dp':
            ctx.set_model(model)
        ctx.set_materials(*mats)
        _set_curve(ctx, model, curve)
        ep = Ep.copy()
        # scrub between the forms: none may pass its pin with what the call before left in the context's device buffers
        if accept:
            scrub(ctx, U, Ep, kw)
        full = ctx.step(U, ep, apply_plastic_strain=accept, want=EVERY, **kw)
        scrub(ctx, U, Ep, kw)
        kf = ctx.step(U, Ep.copy(), want=('K', 'F'), **kw)
        scrub(ctx, U, Ep, kw)
        k_only = ctx.step(U, Ep.copy(), want=('K',), **kw)
        scrub(ctx, U, Ep, kw)
        f_only = ctx.step(U, Ep.copy(), want=('F',), **kw)
        none = ctx.step(U, None, want=EVERY, **kw)
        zero = ctx.step(U, np.zeros((4, n_int)), want=EVERY, **kw)
        e0kw = {} if e0 is None else {'e0': e0}
        scale0 = ctx.step(U, Ep.copy(), want=EVERY, e0_field=field * 3.0 + 1.0, e0_scale=0.0, **e0kw)
        zeros = ctx.step(U, Ep.copy(), want=EVERY, e0_field=np.zeros((4, n_int)), e0_scale=scale, **e0kw)
        const = ctx.step(U, Ep.copy(), want=EVERY, e0_field=np.repeat(zc, n_int, axis=1), e0_scale=1.0)
        plain = ctx.step(U, Ep.copy(), want=EVERY, e0=zc)
        pattern = ctx.pattern()
    finally:
        ctx.close()
    what = f'{model} {t} {route} {name}'
    # bitwise pins
    assert np.array_equal(kf['K'].data, full['K'].data) and np.array_equal(kf['F'], full['F'])
    assert np.array_equal(k_only['K'].data, full['K'].data) and np.array_equal(f_only['F'], full['F'])
    for r in (kf, k_only, f_only):
        assert (r['n_smooth'], r['n_apex']) == (full['n_smooth'], full['n_apex'])
    assert _same(none, zero)
    assert _same(scale0, zeros)
    if model != 'dp' or route == 'node':
        assert _same(const, plain), 'constant field against the plain step'
    else:
        _check_points(model, const, Ep, const['E'], Ep, mats, np.repeat(zc, n_int, axis=1), False, what + ' constant field',
                      generator_conditions=False)
        _check_assembly(t, route, const, elem, coord, fep.element_tables(t), pattern, what + ' constant field')
    # the field is read: the step differs from the one without it
    assert not np.array_equal(full['s'], zeros['s'])
    # 1. strain
    tab = fep.element_tables(t)
    E, S_E = ElemRef(elem, coord, tab, pattern=pattern).strain(U)
    r_E = ratio(full['E'], E, S_E)
    print(f'[E] {what}: ratio {r_E:.2f}')
    assert r_E <= C_E[t], ('E', r_E)
    if t != 'P1' or route == 'node':
        assert np.array_equal(full['E'], E_dp)
    # 2. return map on the kernel's strain, 3. assembly of the kernel's ds and s
    _check_points(model, full, ep, full['E'], Ep, mats, fref.z_of(e0, field, scale), accept, what, curve=curve)
    _check_assembly(t, route, full, elem, coord, tab, pattern, what)


def _contributors(elem, n_q, k, pattern, n_n):
    """The F entries and K entries the element of point k contributes to."""
    nodes = np.unique(elem[:, k // n_q])
    dofs = np.concatenate([2 * nodes, 2 * nodes + 1])
    f_hit = np.zeros(2 * n_n, dtype=bool)
    f_hit[dofs] = True
    indptr, indices = pattern
    rows = np.repeat(np.arange(2 * n_n), np.diff(indptr))
    return f_hit, f_hit[rows] & f_hit[indices]


def _poisoned(fep, monkeypatch, model, t, bad):
    """`bad` at one point of the field: the last lane of workgroup 0 (point 255) and the first lane of workgroup 1 (point 256).
    Every other point's outputs and every F entry / K entry without a contributing element of the poisoned point are the
    clean run's bits, and the clean step afterwards returns the earlier bits; then ds and K are finite."""
    c = fcases.build(model, t, 'block257')
    elem, coord, U, Ep, mats, e0 = (c[k] for k in ('elem', 'coord', 'U', 'ep', 'mats', 'e0'))
    e0kw = {} if e0 is None else {'e0': e0}
    ctx = _context(fep, monkeypatch, c, model, 'node' if t == 'P1' else 'default')
    finite = True
    try:
        n_int, n_q = ctx.n_int, ctx.n_q
        assert n_int >= 257
        if model != 'dp':
            ctx.set_model(model)
        ctx.set_materials(*mats)
        _set_curve(ctx, model, c['curve'])
        pattern = ctx.pattern()

        def run(f):
            p = Ep.copy()
            return ctx.step(U, p, apply_plastic_strain=True, want=EVERY, e0_field=f, e0_scale=c['scale'], **e0kw), p
        clean, ep_clean = run(c['field'])
        for k in (255, 256):
            f_hit, k_hit = _contributors(elem, n_q, k, pattern, ctx.n_n)
            others = np.arange(n_int) != k
            f = c['field'].copy()
            f[1, k] = bad
            got, ep_got = run(f)
            for key in POINT_KEYS:
                assert np.array_equal(got[key][..., others], clean[key][..., others]), (key, k, bad)
            assert np.array_equal(ep_got[:, others], ep_clean[:, others])
            assert np.array_equal(got['F'][~f_hit], clean['F'][~f_hit])
            assert np.array_equal(got['K'].data[~k_hit], clean['K'].data[~k_hit])
            assert np.isnan(got['s'][:, k]).any() and not got['ind_p'][k]              # never hidden
            again, ep_again = run(c['field'])
            assert _same(again, clean) and np.array_equal(ep_again, ep_clean)
            ok = bool(np.isfinite(got['ds']).all() and np.isfinite(got['K'].data).all())
            print(f'[poison] {model} {t} point {k} {bad}: contained; ds and K finite: {ok}; ds at the point {got["ds"][:, k]}')
            finite = finite and ok
    finally:
        ctx.close()
    assert finite, 'ds / K not finite'


@pytest.mark.parametrize('model', fcases.MODELS)
@pytest.mark.parametrize('t', fcases.TYPES)
def test_nan_in_one_field_point_is_contained(fep, monkeypatch, model, t):
    _poisoned(fep, monkeypatch, model, t, np.nan)


@pytest.mark.parametrize('model', fcases.MODELS)
@pytest.mark.parametrize('t', fcases.TYPES)
def test_infinity_in_one_field_point_is_contained(fep, monkeypatch, model, t):
    """An infinite initial strain counts as a NaN (fep.h): the point comes back elastic with a NaN stress for every model."""
    _poisoned(fep, monkeypatch, model, t, np.inf)


# ---- mesh-free -------------------------------------------------------------------------------------------------------------
def _dev_field_return_map(fep, model, e, order, p, e0, field, scale, mats, accept):
    import torch
    dev = torch.device('cuda', 0)
    n = mats[0].size
    up = lambda v: torch.from_numpy(np.array(v, dtype=np.float64, order='C')).to(dev)     # noqa: E731
    ed = up(e.T if order == 'F' else e)
    ps, cs = (3, 1) if order == 'F' else (1, n)
    pd = None if p is None else up(p)
    md = [up(m) for m in mats]
    fd = up(field)
    f64 = dict(dtype=torch.float64, device=dev)
    S, DS = torch.zeros((4, n), **f64), torch.zeros((9, n), **f64)
    ind, cnt = torch.zeros(n, dtype=torch.uint8, device=dev), torch.full((2,), -1, dtype=torch.int64, device=dev)
    e0v = None if e0 is None else np.ascontiguousarray(e0, dtype=np.float64).ravel()
    rc = fep.lib().fep_return_map_field_dev(fep.hotpath.MODELS[model], 0, torch.cuda.current_stream().cuda_stream, n, ed.data_ptr(),
                                            ps, cs, None if e0v is None else e0v.ctypes.data_as(ctypes.c_void_p), fd.data_ptr(),
                                            float(scale), None if pd is None else pd.data_ptr(), *(m.data_ptr() for m in md),
                                            int(accept), S.data_ptr(), DS.data_ptr(), ind.data_ptr(), cnt.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    k = cnt.cpu().numpy()
    return {'s': S.cpu().numpy(), 'ds': DS.cpu().numpy(), 'ind_p': ind.cpu().numpy().astype(bool), 'n_smooth': int(k[0]),
            'n_apex': int(k[1]), 'ep': None if pd is None else pd.cpu().numpy()}


def _refused(fep, n):
    import torch
    E, Ep, mats, e0, field = fcases.mesh_free('vmi', n, 0)
    dev = torch.device('cuda', 0)
    up = lambda v: torch.from_numpy(np.array(v, dtype=np.float64, order='C')).to(dev)     # noqa: E731
    ed, pd, fd, md = up(E), up(Ep), up(field), [up(m) for m in mats]
    S, DS = torch.full((4, n), 7.0, dtype=torch.float64, device=dev), torch.full((9, n), 7.0, dtype=torch.float64, device=dev)
    ind, cnt = torch.full((n,), 7, dtype=torch.uint8, device=dev), torch.full((2,), -1, dtype=torch.int64, device=dev)
    e0v = np.ascontiguousarray(e0, dtype=np.float64).ravel()
    assert fep.hotpath.MODELS['vmi'] == 5
    for accept in (0, 1):
        rc = fep.lib().fep_return_map_field_dev(5, 0, torch.cuda.current_stream().cuda_stream, n, ed.data_ptr(), 1, n,
                                                e0v.ctypes.data_as(ctypes.c_void_p), fd.data_ptr(), fcases.SCALE, pd.data_ptr(),
                                                *(m.data_ptr() for m in md), accept, S.data_ptr(), DS.data_ptr(), ind.data_ptr(),
                                                cnt.data_ptr())
        torch.cuda.synchronize()
        assert rc == -1                                                                   # FEP_EINVAL
        assert bool((S == 7.0).all()) and bool((DS == 7.0).all()) and bool((ind == 7).all()) and cnt.tolist() == [-1, -1]
        assert np.array_equal(pd.cpu().numpy(), Ep) and np.array_equal(fd.cpu().numpy(), field)
        ep_h = Ep.copy()
        with pytest.raises(ValueError):
            fep.construct_constitutive_problem_field('vmi', E, field, ep_h, *mats, apply_plastic_strain=bool(accept), e0=e0,
                                                     e0_scale=fcases.SCALE)
        assert np.array_equal(ep_h, Ep)


@pytest.mark.parametrize('model', fcases.MODELS)
@pytest.mark.parametrize('n', fcases.MESH_FREE_N)
def test_mesh_free_field_return_map(fep, model, n):
    """fep_return_map_field_dev and _host: both strain orders, accept on and off, with and without the uniform part.  The pair
    has no place for a curve and refuses 'vmi' (a field reaches that model through a context's step): FEP_EINVAL, nothing
    written."""
    if model == 'vmi':
        _refused(fep, n)
        return
    for seed in range(8):                                               # the first draw without a point under the floors
        E, Ep, mats, e0, field = fcases.mesh_free(model, n, seed)
        o = fref.return_map(model, E, Ep, mats, fref.z_of(e0, field, fcases.SCALE), False)
        if not fcases.excluded(model, o, mats).any():
            break
    else:
        raise AssertionError('no draw keeps every point above the floors')
    for order in ('C', 'F'):
        for accept in (False, True):
            for e0_, scale in ((e0, fcases.SCALE), (None, 1.0)):
                z = fref.z_of(e0_, field, scale)
                o = fref.return_map(model, E, Ep, mats, z, accept)
                if fcases.excluded(model, o, mats).any():
                    continue
                dev = _dev_field_return_map(fep, model, E, order, Ep, e0_, field, scale, mats, accept)
                ep_h = Ep.copy()
                host = fep.construct_constitutive_problem_field(model, np.asarray(E, order=order), field, ep_h, *mats,
                                                                apply_plastic_strain=accept, e0=e0_, e0_scale=scale)
                for got, ep_got in ((dev, dev['ep']), (host, ep_h)):
                    assert np.array_equal(got['ind_p'], o['ind_p'])
                    assert (got['n_smooth'], got['n_apex']) == (o['n_smooth'], o['n_apex'])
                    for k in ('s', 'ds'):
                        assert relerr(got[k], o[k]) <= TOL and relerr_points(got[k], o[k]) <= TOL_PT, (k, order, accept)
                    if accept:
                        assert relerr(ep_got, o['ep']) <= TOL and relerr_points(ep_got, o['ep']) <= TOL_PT
                    else:
                        assert np.array_equal(ep_got, Ep)
                assert all(np.array_equal(dev[k], host[k]) for k in POINT_KEYS)


def test_field_entry_points_refuse_null_field_and_unknown_model(fep):
    l = fep.lib()
    n = 4
    a = np.zeros((9, n))
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)                     # noqa: E731
    args = (p(a), 1, n, None)
    tail = (None, p(a), p(a), p(a), p(a), 0, p(a), p(a), None, None)
    assert l.fep_return_map_field_host(0, 0, n, *args, None, 1.0, *tail) == -1            # FEP_EINVAL: NULL field
    assert l.fep_return_map_field_host(3, 0, n, *args, p(a), 1.0, *tail) == -1            # unknown model
    assert l.fep_return_map_field_host(-1, 0, n, *args, p(a), 1.0, *tail) == -1
    assert l.fep_return_map_field_dev(0, 0, None, n, *args, None, 1.0, *tail) == -1
    assert l.fep_return_map_field_dev(7, 0, None, n, *args, p(a), 1.0, *tail) == -1
    c = fcases.build('dp', 'P1', 'block256')
    ctx = fep.MeshContext(c['elem'], c['coord'])
    try:
        ctx.set_materials(*c['mats'])
        u = np.zeros(ctx.n_dof)
        assert l.fep_step_field_host(ctx.handle, p(u), None, None, 1.0, None, 0, *([None] * 7)) == -1
        with pytest.raises(ValueError):
            ctx.step(u, e0_field=np.zeros((4, ctx.n_int + 1)))
    finally:
        ctx.close()


# ---- point coordinates -----------------------------------------------------------------------------------------------------
def _curved_wall_p4(fep):
    g = load_golden('tsx')
    m = fep.create_midpoints_P4(g['coord'], g['elem'], curves=[fep.tsx_tunnel.TSX_HOLE])
    return np.ascontiguousarray(m['elem_ext'], dtype=np.int64), np.ascontiguousarray(m['coord_ext'])


@pytest.mark.parametrize('t,name', [(t, n) for t in fcases.TYPES for n in fcases.names(t)] + [('P4', 'curved wall')])
def test_point_coords(fep, t, name):
    import torch
    elem, coord = _curved_wall_p4(fep) if name == 'curved wall' else (fcases.build('dp', t, name)[k] for k in ('elem', 'coord'))
    ref, scale = fref.point_coords(fep, t, elem, coord)
    ctx = fep.MeshContext(elem, coord)
    try:
        host = ctx.point_coords()
        xq = torch.full((2, ctx.n_int), float('nan'), dtype=torch.float64, device=torch.device('cuda', 0))
        ctx.point_coords_dev(torch.cuda.current_stream().cuda_stream, xq.data_ptr())
        torch.cuda.synchronize()
        n_p = ctx.n_p
    finally:
        ctx.close()
    assert np.array_equal(xq.cpu().numpy(), host)
    worst = (np.abs(host - ref) / (n_p * U_RND * scale)).max()
    print(f'[xq] {t} {name}: worst |delta| / (n_p u sum|terms|) = {worst:.3f}')
    assert worst <= 1.0


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', fcases.K0_TYPES)
def test_k0_box_stays_at_rest(fep, t):
    """Measured on MI355X: |F0| over its bound at the free DOFs 0.20 (P1), 0.19 (Q1); largest accepted |U| over the largest
    displacement under the body force alone 3.9e-16 (P1), 9.3e-16 (Q1), bound 1e-9.  (On P2 the same box gave |F0| = 107
    bounds: its quadrature table integrates cubics to 1.4e-13 only, tests/e0_field_cases.K0_TYPES.)"""
    b = fcases.k0_box(t)
    elem, coord, mats = b['elem'], b['coord'], b['mats']
    h = fep.solve_tsx_tunnel(coord, elem, t, n_load_steps=4, monitor=(0, 0), in_situ=b['in_situ'], body_force=b['body_force'],
                             materials=mats)
    assert len(h['zeta']) == 4 and h['n_plast'] == [0] * 4
    # F0 at the free DOFs: assembly bound + volume-load bound
    ctx = fep.MeshContext(elem, coord)
    try:
        ctx.set_materials(*mats)
        pattern, weight = ctx.pattern(), ctx.geometry()[2].ravel()
        K_el = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
        f_V = ctx.load_volume(uniform=b['body_force'])
        xq = ctx.point_coords()
    finally:
        ctx.close()
    assert np.array_equal(h['s0_field'], b['in_situ'](xq[0], xq[1]))
    tab = fep.element_tables(t)
    _, _, _, S_F = ElemRef(elem, coord, tab, pattern=pattern).assemble(None, h['s0_field'])
    tt = fep.LagrangeElementType[t]
    hatp = fep.get_local_basis_volume(tt, fep.get_quadrature_volume(tt)[0])[0]
    f_int = np.array([[b['body_force'][0]], [b['body_force'][1]]]) * np.ones((1, weight.size))
    lim_V, _ = loads_exact.volume_bound(elem, coord.shape[1], f_int, hatp, weight)
    bound = C_F[t] * U_RND * np.asarray(S_F).reshape(-1, 2).T + lim_V
    free = h['Q']
    r_F0 = (np.abs(h['F0'])[free] / bound[free]).max()
    print(f'[k0] {t}: |F0| over its bound at the free DOFs: {r_F0:.3f}')
    assert r_F0 <= 1.0
    # the displacement the body force alone would cause, one elastic solve
    import scipy.sparse.linalg as sspl
    qf = free.flatten(order='F')
    u_ref = np.abs(sspl.spsolve(K_el[qf][:, qf].tocsc(), f_V.flatten(order='F')[qf])).max()
    r_U = max(np.abs(u).max() for u in h['U']) / u_ref
    print(f'[k0] {t}: largest accepted |U| / largest |U| under the body force alone = {r_U:.3e} (u_ref {u_ref:.3e})')
    assert r_U <= 1e-9
    for zeta, s in zip(h['zeta'], h['s']):
        assert relerr_points(s, zeta * h['s0_field']) <= 1e-12


def test_uniform_field_reproduces_the_reference_trace_p1(fep):
    g = load_golden('tsx')
    h = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', in_situ=fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 0.0, 0.0))
    assert len(h['zeta']) == 17 and np.allclose(h['zeta'], g['p1_zeta'], rtol=0, atol=1e-15)
    assert h['n_plast'] == g['p1_nplast'].tolist() == [0] * 13 + [1, 1, 2, 3]
    assert relerr(h['F0'], g['p1_F0']) <= 1e-12
    assert relerr(h['U'][12], g['p1_U_step13']) <= 1e-10
    assert relerr(h['U'][-1], g['p1_U_final']) <= 1e-10
    assert abs(h['displ'][-1] - (-0.0019794496707526746)) <= 1e-10 * 0.0019794496707526746


def test_uniform_field_reproduces_the_reference_trace_p2(fep, tsx_csv_dir):
    g = load_golden('tsx_p2_trace')
    h = fep.solve_tsx_tunnel(element_type='P2', mesh_dir=tsx_csv_dir,
                             in_situ=fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 0.0, 0.0))
    assert len(h['zeta']) == 17 == len(g['zeta']) and np.allclose(h['zeta'], g['zeta'], rtol=0, atol=1e-15)
    assert h['n_plast'] == g['nplast'].tolist() and h['n_plast'][-1] > 0
    assert relerr(h['F0'], g['F0']) <= 1e-12
    for k, step in enumerate(g['steps']):
        assert relerr(h['U'][int(step)], g['U_steps'][k]) <= 1e-10, step
    assert np.abs(np.array(h['displ']) - g['U_mon']).max() <= 1e-10 * np.abs(g['U_mon']).max()


def test_depth_varying_stress_against_the_cpu_context(fep):
    """The tunnel under a stress that grows with depth and its body force: the GPU run against the same driver on the CPU
    context (tests/e0_field_ref.FieldContext); crown and invert move by different amounts, and the uniform run differs."""
    g = load_golden('tsx')
    coord, elem = g['coord'], g['elem']
    grad = 0.4                                                          # stress per unit of height: -11 at y = 0, -31 at the bottom
    kw = dict(in_situ=fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 0.0, (45.0 / 11.0 * grad, grad, 0.0, 60.0 / 11.0 * grad)),
              body_force=(0.0, -grad))
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', **kw)
    r = fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=fref.FieldContext, **kw)
    uni = fep.solve_tsx_tunnel(coord, elem, 'P1', in_situ=fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 0.0, 0.0))
    assert len(h['zeta']) == len(r['zeta']) == 17 and h['n_plast'] == r['n_plast']
    print('[depth] plastic points per step:', h['n_plast'])
    for a, b in zip(h['U'], r['U']):
        assert relerr(a, b) <= 1e-9
    wall = np.flatnonzero(np.abs((coord[0] / 2.1875) ** 2 + (coord[1] / 1.75) ** 2 - 1) < 1e-3)
    crown, invert = wall[np.argmax(coord[1, wall])], wall[np.argmin(coord[1, wall])]
    u_c, u_i = h['U'][-1][1, crown], h['U'][-1][1, invert]
    print(f'[depth] crown {u_c:.6e} invert {u_i:.6e}; uniform run: {uni["U"][-1][1, crown]:.6e} {uni["U"][-1][1, invert]:.6e}')
    assert abs(abs(u_c) - abs(u_i)) > 1e-3 * max(abs(u_c), abs(u_i))
    assert relerr(uni['U'][-1], h['U'][-1]) > 1e-3

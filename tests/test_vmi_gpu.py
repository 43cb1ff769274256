"""The von Mises model with isotropic hardening on a piecewise-linear curve on the GPU: the mesh-free kernel
(return_map_vmi_kernel; fep_return_map_vmi_host / _dev) against the fixtures of the high-precision reference with the bounds of
DESIGN.md section 7 (vmi_cases.bound) and against the NumPy restatement (tests/vmi_ref.py), the step of a 'vmi' context on
every route, the interface of the model and its curve, the non-finite rules with kappa as a fifth component, capture, staging
beyond the ring and the cyclic driver with and without refinement.  Bounds against the restatement: s, ds, ep, E 1e-13 of the
array maximum and 1e-12 per point; K, F 1e-12 and 1e-11 per row; accepted displacements 1e-10 (1e-9 with multigrid)."""
import ctypes
import functools

import numpy as np
import pytest

import model_step_cases as msc
import staging_cases as sc
from conftest import dp_materials, relerr, relerr_points, relerr_rows
from meshes import jitter, rect
from model_ref import bytes_equal, check_points
from test_vm_gpu import MESHES
from vm_cases import BULK, HARDENING, SHEAR, YIELD
from vmi_cases import (CRIT_FLOOR, away_from_breakpoints, check, check_flags, cpu_cycle, curve, dev_return_map, errors, fixture,
                       launches, merge, points, state_rows)
from vmi_ref import VMIRefContext, vmi_return_map

pytestmark = pytest.mark.gpu

TOL, TOL_PT, TOL_K, TOL_K_ROW = 1e-13, 1e-12, 1e-12, 1e-11
EVERY = ('E', 's', 'ds', 'ind_p', 'K', 'F')
FEP_EINVAL, FEP_ESTATE = -1, -6


def _host(fep, e, p, mats, crv, accept, e0):
    r = fep.construct_constitutive_problem_vmi(e, p, *mats, crv, apply_plastic_strain=accept, e0=e0)
    return dict(r, n_smooth=r['n_plast'], n_apex=0)


# ---------------------------------------------------------------------------------------
# the mesh-free kernel against the high-precision fixture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('launch', range(8))
def test_mesh_free_kernel_against_the_high_precision_fixture(fep, launch):
    fix = fixture()
    idx, e0, c = launches(fix)[launch]
    crv = curve(c)
    mats = [fix[k][idx] for k in ('G', 'K', 'm3', 'm4')]
    e, p = fix['e'][:, idx], fix['p'][:, idx]
    errs = {}
    for order in 'CF':
        ev = np.asfortranarray(e) if order == 'F' else np.ascontiguousarray(e)
        for accept in (True, False):
            ph = p.copy()
            host = _host(fep, ev, ph, mats, crv, accept, e0)
            dev = dev_return_map(e, order, p, e0, mats, crv, accept)
            for got in (host, dev):
                check_flags(fix, idx, got)
                keys = ('s', 'ds', 'ep') if accept else ('s', 'ds')
                errs = merge(errs, errors(fix, {k: got[k] for k in keys}, idx))
            if not accept:
                assert np.array_equal(ph, p) and np.array_equal(dev['ep'], p)
            for k in ('s', 'ds', 'ind_p'):                              # the two entry points launch the same kernel
                assert np.array_equal(host[k], dev[k]), k
    check(errs)


# ---------------------------------------------------------------------------------------
# the mesh-free kernel against the restatement
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('n', [1, 255, 257, 1000])
def test_mesh_free_kernel_against_the_restatement(fep, n, order):
    for c in (2, 3):
        crv = curve(c)
        for uniform in (True, False):
            e, p, e0, mats = points(n, uniform, 100 + n + c, crv)
            ev = np.asfortranarray(e) if order == 'F' else np.ascontiguousarray(e)
            for with_ep, accept in ((False, False), (True, False), (True, True)):
                for z in (None, e0):
                    ref = vmi_return_map(e, p if with_ep else None, *mats, crv, apply_plastic_strain=accept, e0=z)
                    # conditions on the inputs, asserted on the restatement: nothing within rounding of a decision
                    assert (np.abs(ref['crit']) >= CRIT_FLOOR * mats[3]).all()
                    landed = vmi_return_map(e, p if with_ep else None, *mats, crv, apply_plastic_strain=True, e0=z)
                    assert away_from_breakpoints(landed, crv)
                    if n > 1:                                            # (one point is all or nothing)
                        assert 0.2 <= ref['ind_p'].mean() <= 0.8, ref['ind_p'].mean()
                    ph = p.copy() if with_ep else None
                    host = _host(fep, ev, ph, mats, crv, accept, z)
                    dev = dev_return_map(e, order, p if with_ep else None, z, mats, crv, accept)
                    for got in (host, dev):
                        assert np.array_equal(got['ind_p'], ref['ind_p']) and got['n_smooth'] == ref['n_plast'] and got['n_apex'] == 0
                        check_points(got, ref, ('s', 'ds'), TOL, TOL_PT)
                        if accept:
                            check_points(got, ref, ('ep',), TOL, TOL_PT)
                            assert np.array_equal(got['ep'][3][~ref['ind_p']], p[3][~ref['ind_p']])
                    if with_ep and not accept:                           # a non-accepting call leaves the state alone
                        assert np.array_equal(ph, p) and np.array_equal(dev['ep'], p)
                    if accept:
                        assert host['ep'] is ph


# ---------------------------------------------------------------------------------------
# the step of a 'vmi' context
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(fep, t):
    """Jittered mesh of type t (test_vm_gpu.MESHES), the CPU context on it, a displacement at which about half of the points
    yield on either curve, a state with kappa spread over the curves, per-point materials, an initial strain and a field."""
    rng = np.random.default_rng(170 + len(t) + ord(t[1]))
    elem, coord = rect(t, *MESHES[t])
    coord = jitter(elem, coord, 0.15, rng)
    ref = VMIRefContext(elem, coord, *fep.element_tables(fep.LagrangeElementType[t]))
    n = ref.n_int
    assert n > 256 and n % 256 != 0
    ref.set_materials(SHEAR, BULK, HARDENING, YIELD)
    U = rng.normal(0, 1.0, size=(2, coord.shape[1]))
    flat = vmi_return_map(ref.orc.strain(ref.c['B'], U), None, *ref.m, (np.zeros(1), np.zeros(1)))
    U *= 1.5 * YIELD / np.median(flat['crit'] + YIELD)
    ep = state_rows(rng, n, 0.1 * YIELD / (2 * SHEAR), 0.02)
    f = rng.uniform(0.6, 1.4, n)
    per_point = (SHEAR * f, BULK * f[::-1], HARDENING * rng.uniform(0, 2, n), YIELD * rng.uniform(0.6, 1.4, n))
    e0 = rng.normal(0, 0.2 * YIELD / (2 * SHEAR), size=(4, 1))
    field = rng.normal(0, 0.4 * YIELD / (2 * SHEAR), size=(4, n))
    return elem, coord, ref, U, ep, per_point, e0, field


def _check_step(got, ref, crv, landed, want_points=True):
    share = ref['ind_p'].mean()
    print('plastic share', share)
    assert 0.2 <= share <= 0.8
    assert np.abs(ref['crit']).min() > 0 and away_from_breakpoints(landed, crv)
    assert got['n_smooth'] == ref['n_smooth'] and got['n_apex'] == 0
    if want_points:
        assert np.array_equal(got['ind_p'], ref['ind_p'])
        check_points(got, ref, ('E', 's', 'ds'), TOL, TOL_PT)
    K, Kr, F, Fr = got['K'], ref['K'], np.asarray(got['F']), np.asarray(ref['F'])
    ek = abs(K - Kr).max() / abs(Kr).max()
    print('K', ek, relerr_rows(K, Kr), 'F', relerr(F, Fr), relerr_rows(F.reshape(-1, 2), Fr.reshape(-1, 2)))
    assert ek <= TOL_K and relerr_rows(K, Kr) <= TOL_K_ROW
    assert relerr(F, Fr) <= TOL_K and relerr_rows(F.reshape(-1, 2), Fr.reshape(-1, 2)) <= TOL_K_ROW


def _ref_step(ref, U, ep, e0=None, accept=False):
    """(the step of the restatement, the state an accepting call would leave: for the distance to the breakpoints)"""
    landed = np.zeros((4, ref.n_int)) if ep is None else ep.copy()
    ref.step(U, landed, e0=e0, apply_plastic_strain=True)
    r = ref.step(U, ep, e0=e0, apply_plastic_strain=accept)
    return r, {'ep': landed, 'ind_p': r['ind_p']}


def _expect_names(ctx, t, route):
    tag = 'p1_point_vmi_kernel' if t == 'P1' else f'point_vmi_kernel<{ctx.n_p}, {ctx.n_q}>'
    tail = {'node': 'p1_node_lds_kernel<', 'patch': ' + fixup_kernel', 'coo': 'csr_reduce'}[route]
    for which in (0, 1):
        names = ctx.kernel_names(which)
        assert names.startswith(tag + ' + ') and tail in names, names
        assert ('element_kernel<' in names) == (route != 'node') and 'fused' not in names


@pytest.mark.parametrize('t,route', [(t, r) for t in MESHES for r in msc.ROUTES[t]])
def test_step_of_a_vmi_context(fep, monkeypatch, t, route):
    elem, coord, ref, U, ep, per_point, e0, field = _case(fep, t)
    uniform = (SHEAR, BULK, HARDENING, YIELD)
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    ctx = fep.MeshContext(elem, coord)
    try:
        ctx.set_model('vmi')
        assert ctx.model == 'vmi'
        _expect_names(ctx, t, 'patch' if route == 'default' else route)
        for c in (2, 3):
            crv = curve(c)
            ctx.set_hardening(*crv)
            ref.set_hardening(*crv)
            assert all(np.array_equal(a, b) for a, b in zip(ctx.hardening, crv))
            for mats in (uniform, per_point):
                ctx.set_materials(*mats)
                ref.set_materials(*mats)
                ep_g, ep_r = ep.copy(), ep.copy()                       # every output, accepting
                got = ctx.step(U, ep_g, apply_plastic_strain=True, want=EVERY)
                want, landed = _ref_step(ref, U, ep_r, accept=True)
                _check_step(got, want, crv, landed)
                print('ep', relerr(ep_g, ep_r), relerr_points(ep_g, ep_r))
                assert relerr(ep_g, ep_r) <= TOL and relerr_points(ep_g, ep_r) <= TOL_PT
                assert not np.array_equal(ep_r, ep) and (ep_g[3] >= ep[3]).all()
                assert np.array_equal(ep_g[3] > ep[3], want['ind_p'])
            ctx.set_materials(*uniform)
            ref.set_materials(*uniform)
            want, landed = _ref_step(ref, U, ep.copy())
            ep_g = ep.copy()                                            # K, F only: ds / s travel through the context's scratch
            got = ctx.step(U, ep_g, want=('K', 'F'))
            assert sorted(k for k in got if k in EVERY) == ['F', 'K'] and np.array_equal(ep_g, ep)
            _check_step(got, want, crv, landed, want_points=False)
            want, landed = _ref_step(ref, U, None)                      # no state given = zeros
            _check_step(ctx.step(U, None, want=EVERY), want, crv, landed)
            plain = ctx.step(U, ep.copy(), e0=e0, want=EVERY)           # with an initial strain
            want, landed = _ref_step(ref, U, ep.copy(), e0=e0)
            _check_step(plain, want, crv, landed)
            z = e0 + 0.37 * field                                       # an initial strain per point
            got = ctx.step(U, ep.copy(), e0=e0, e0_field=field, e0_scale=0.37, want=EVERY)
            want, landed = _ref_step(ref, U, ep.copy(), e0=z)
            _check_step(got, want, crv, landed)
            if t in ('P1', 'Q2'):                                       # a field of equal columns is the plain call, bit for bit
                same = ctx.step(U, ep.copy(), e0_field=np.repeat(e0, ctx.n_int, axis=1), want=EVERY)
                assert bytes_equal(same, plain) and np.array_equal(same['E'], plain['E'])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# the interface of the model and its curve
# ---------------------------------------------------------------------------------------
def _set_hardening(fep, ctx, kappa, slope, n_seg=None):
    k, s = np.ascontiguousarray(kappa, dtype=np.float64), np.ascontiguousarray(slope, dtype=np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                     # noqa: E731
    return fep.lib().fep_ctx_set_hardening(ctx.handle, k.size if n_seg is None else n_seg, vp(k), vp(s))


@pytest.mark.parametrize('t', ['P1', 'Q1'])
def test_model_and_curve_interface(fep, t):
    elem, coord, _, U, ep, _, _, _ = _case(fep, t)
    n = ep.shape[1]
    crv = curve(2)
    mats = (SHEAR, BULK, HARDENING, YIELD)
    Udp = U * 0.05
    dp = fep.MeshContext(elem, coord)
    dp.set_materials(*dp_materials(n))
    vm = fep.MeshContext(elem, coord)
    vm.set_model('vm')
    vm.set_materials(*mats)
    ep_vm = ep.copy()
    ep_vm[3] = -(ep[0] + ep[1])
    before_dp, before_vm = dp.step(Udp, np.zeros((4, n))), vm.step(U, ep_vm.copy())
    ctxs = [fep.MeshContext(elem, coord) for _ in range(4)]
    try:
        a, b, c, d = ctxs
        a.set_model('vmi'); a.set_materials(*mats); a.set_hardening(*crv)       # noqa: E702
        b.set_materials(*mats); b.set_model('vmi'); b.set_hardening(*crv)       # noqa: E702
        c.set_model('vmi'); c.set_hardening(*crv); c.set_materials(*mats)       # noqa: E702
        d.set_model('vmi'); d.set_materials(*mats)                              # noqa: E702
        ra = a.step(U, ep.copy())
        assert ra['n_smooth'] > 0
        assert bytes_equal(ra, b.step(U, ep.copy())) and bytes_equal(ra, c.step(U, ep.copy())) and bytes_equal(ra, a.step(U, ep.copy()))
        # without a call: one segment of slope 0, the plane-strain von Mises step on p33 = -(p11 + p22)
        flat = d.step(U, ep.copy())
        assert not bytes_equal(flat, ra) and np.array_equal(flat['ind_p'], before_vm['ind_p'])
        check_points(flat, before_vm, ('s', 'ds'), TOL, TOL_PT)
        assert d.hardening[0].tolist() == [0.0] and d.hardening[1].tolist() == [0.0] and vm.hardening is None
        l = fep.lib()
        m = ctypes.c_int(-1)
        assert l.fep_ctx_model(a.handle, ctypes.byref(m)) == 0 and m.value == 5 == fep.hotpath.MODELS['vmi']
        for bad in (4, 6, 7, -1):                                       # 4 stays unassigned
            assert l.fep_ctx_set_model(a.handle, bad) == FEP_EINVAL
        assert l.fep_ctx_model(a.handle, ctypes.byref(m)) == 0 and m.value == 5
        # the curve belongs to a 'vmi' context
        assert _set_hardening(fep, vm, *crv) == FEP_ESTATE and _set_hardening(fep, dp, *crv) == FEP_ESTATE
        with pytest.raises(fep.FepError):
            vm.set_hardening(*crv)
        assert l.fep_ctx_set_hardening(None, 1, None, None) == FEP_EINVAL
        # bad curves are refused and change nothing
        k8, s8 = crv
        bad_curves = [(k8, s8, 0), (np.arange(9.0), np.zeros(9), 9), (k8 + 1e-4, s8, None), (k8[[0, 2, 1, 3]], s8[:4], None),
                      (k8[[0, 1, 1, 3]], s8[:4], None), (np.array([0.0, np.nan]), s8[:2], None),
                      (k8[:2], np.array([1.0, np.nan]), None), (np.array([0.0, np.inf]), s8[:2], None)]
        for k, s, n_seg in bad_curves:
            assert _set_hardening(fep, a, k, s, n_seg) == FEP_EINVAL
        assert l.fep_ctx_set_hardening(a.handle, 2, None, None) == FEP_EINVAL
        with pytest.raises(ValueError):
            a.set_hardening(k8[:3], s8[:2])
        with pytest.raises(ValueError):                                 # 2G + a + slope <= 0 for the context's materials
            a.set_hardening([0.0, 1e-3], [0.0, -2 * SHEAR - HARDENING])
        assert bytes_equal(ra, a.step(U, ep.copy())) and all(np.array_equal(x, y) for x, y in zip(a.hardening, crv))
        for which in (0, 1):
            assert 'vmi_kernel' in a.kernel_names(which) and 'vmi' not in dp.kernel_names(which) and 'vmi' not in vm.kernel_names(which)
        # the mesh-free pair with a field refuses the model, as it refuses 'vmps'
        e = np.zeros((3, n))
        with pytest.raises(ValueError):
            fep.construct_constitutive_problem_field('vmi', e, ep, ep, *[np.full(n, v) for v in mats])
        one = np.zeros(4)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)                # noqa: E731
        assert l.fep_return_map_field_host(5, 0, 1, vp(one), 1, 1, None, vp(one), 1.0, None, vp(one), vp(one), vp(one), vp(one), 0,
                                           None, None, None, None) == FEP_EINVAL
        # the mesh-free entry point refuses a bad curve too
        assert l.fep_return_map_vmi_host(0, 1, vp(one), 1, 1, None, None, vp(one), vp(one), vp(one), vp(one), 0, vp(one), vp(one), 0,
                                         None, None, None, None) == FEP_EINVAL
        # the contexts beside them compute what they computed before
        assert bytes_equal(before_dp, dp.step(Udp, np.zeros((4, n)))) and bytes_equal(before_vm, vm.step(U, ep_vm.copy()))
    finally:
        for x in ctxs + [dp, vm]:
            x.close()


# ---------------------------------------------------------------------------------------
# non-finite values: kappa is a fifth component of the trial state
# ---------------------------------------------------------------------------------------
def test_non_finite_strain_and_kappa_are_contained(fep):
    n = 257
    crv = curve(2)
    e, p, e0, mats = points(n, False, 7, crv)
    clean = _host(fep, e, p.copy(), mats, crv, False, None)
    clean_acc_p = p.copy()
    clean_acc = _host(fep, e, clean_acc_p, mats, crv, True, None)
    assert 0.2 < clean['ind_p'].mean() < 0.8 and clean['ind_p'][[0, 63, 64, n - 1]].any()
    poisons = [('strain', k, np.nan) for k in (0, 63, 64, n - 1)] + [('kappa', 100, np.nan), ('kappa', 101, np.inf),
                                                                       ('kappa', 102, -np.inf)]
    for what, k, v in poisons:
        e2, p2 = e.copy(), p.copy()
        if what == 'strain':
            e2[k % 3, k] = v
        else:
            p2[3, k] = v
        for accept in (False, True):
            for call in ('host', 'dev'):
                ph = p2.copy()
                got = _host(fep, e2, ph, mats, crv, accept, None) if call == 'host' else dev_return_map(e2, 'C', p2, None, mats, crv, accept)
                state = ph if call == 'host' else got['ep']
                ref = clean_acc if accept else clean
                assert not got['ind_p'][k] and np.isnan(got['s'][:, k]).any() and np.isfinite(got['ds']).all(), (what, k, call)
                d = vmi_return_map(np.zeros((3, 1)), None, *[m[k:k + 1] for m in mats], crv)['ds'][:, 0]  # the elastic tangent
                assert relerr(got['ds'][:, k], d) <= TOL
                assert np.array_equal(state[:, k], p2[:, k], equal_nan=True)
                rest = np.arange(n) != k
                for key in ('s', 'ds', 'ind_p'):
                    assert np.array_equal(got[key][..., rest], ref[key][..., rest]), (what, k, key)
                assert np.array_equal(state[:, rest], (clean_acc_p if accept else p)[:, rest])
                assert got['n_smooth'] == int(ref['ind_p'][rest].sum()) and got['n_apex'] == 0
        again = _host(fep, e, p.copy(), mats, crv, False, None)          # it leaves no trace
        assert all(np.array_equal(again[key], clean[key]) for key in ('s', 'ds', 'ind_p')) and again['n_smooth'] == clean['n_smooth']


# ---------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'Q2'])
def test_vmi_step_dev_is_graph_capturable(fep, t):
    """fep_step_dev of a 'vmi' context allocates nothing (fep_ctx_set_model did): its first call on device buffers is captured,
    with K and F through the context's scratch, replayed, and equal bit for bit to the host-array entry point.  The curve
    travels as a kernel argument, so the replay runs on the curve of the capture."""
    import torch
    elem, coord, _, U, ep, _, _, _ = _case(fep, t)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(SHEAR, BULK, HARDENING, YIELD)
    ctx.set_model('vmi')
    ctx.set_hardening(*curve(2))
    n = ctx.n_int
    ep_h = ep.copy()
    want = ctx.step(U, ep_h, apply_plastic_strain=True, want=('ind_p', 'K', 'F'))
    dev = torch.device('cuda', 0)
    f64 = dict(dtype=torch.float64, device=dev)
    Ud = torch.from_numpy(np.ascontiguousarray(U.reshape(-1, order='F'))).to(dev)
    Ep = torch.from_numpy(ep.copy()).to(dev)
    ind = torch.zeros(n, dtype=torch.uint8, device=dev); Kd = torch.zeros(ctx.nnz, **f64); F = torch.zeros(ctx.n_dof, **f64)   # noqa: E702
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.step_dev(torch.cuda.current_stream().cuda_stream, Ud.data_ptr(), ep=Ep.data_ptr(), accept=True, ind_p=ind.data_ptr(),
                     k_data=Kd.data_ptr(), f_out=F.data_ptr(), counts=cnt.data_ptr())
    for x in (Kd, F, ind, cnt):
        x.zero_()
    Ep.copy_(torch.from_numpy(ep))
    ctx.set_hardening(*curve(3))                                        # the captured launch keeps the curve it was captured with
    g.replay()
    torch.cuda.synchronize()
    assert want['n_smooth'] > 0 and tuple(cnt.cpu().tolist()) == (want['n_smooth'], 0)
    assert np.array_equal(Kd.cpu().numpy(), want['K'].data) and np.array_equal(F.cpu().numpy(), want['F'])
    assert np.array_equal(ind.cpu().numpy().astype(bool), want['ind_p']) and np.array_equal(Ep.cpu().numpy(), ep_h)
    ctx.close()


# ---------------------------------------------------------------------------------------
# staging: a host call longer than the ring
# ---------------------------------------------------------------------------------------
def test_host_call_longer_than_the_ring_equals_the_device_call(fep):
    n = sc.N_POINTS
    assert 72 * n > sc.SLOTS * sc.SLOT_BYTES                             # ds alone does not fit the ring of pinned slots
    crv = curve(2)
    e, p, _, mats = points(sc.N_BASE, False, 3, crv)
    e, p, mats = sc.tile(e, n), sc.tile(p, n), tuple(sc.tile(m, n) for m in mats)
    s, ds = sc.pageable((4, n)), sc.pageable((9, n))                     # ordinary memory: staged through the ring
    ind, counts, ph = sc.pageable(n, np.uint8), np.zeros(2, dtype=np.int64), sc.place('pageable', p)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                     # noqa: E731
    k, sl = np.ascontiguousarray(crv[0]), np.ascontiguousarray(crv[1])
    rc = fep.lib().fep_return_map_vmi_host(0, n, vp(e), 1, n, None, vp(ph), *(vp(m) for m in mats), k.size, vp(k), vp(sl), 1,
                                           vp(s), vp(ds), vp(ind), vp(counts))
    assert rc == 0
    dev = dev_return_map(e, 'C', p, None, mats, crv, True)
    assert 0.2 < dev['ind_p'].mean() < 0.8 and (int(counts[0]), int(counts[1])) == (dev['n_smooth'], 0)
    assert np.array_equal(s, dev['s']) and np.array_equal(ds, dev['ds']) and np.array_equal(ind.astype(bool), dev['ind_p'])
    assert np.array_equal(ph, dev['ep']) and not np.array_equal(ph, p)


# ---------------------------------------------------------------------------------------
# the cyclic driver
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver,tol', [('direct', 1e-10), ('amg', 1e-9)])
@pytest.mark.parametrize('t', ['P1', 'Q2'])
def test_cyclic_driver_with_isotropic_hardening_against_the_cpu_run(fep, t, solver, tol):
    ref = cpu_cycle(t)
    assert ref['failed_at'] is None and max(ref['n_plast']) > 0
    r = fep.solve_cutout_cyclic(t, level=0, linear_solver=solver, hardening=0.0, isotropic=15000.0)
    assert r['failed_at'] is None and r['zeta'] == ref['zeta']
    assert r['n_plast'] == ref['n_plast']
    for k, (U, Ur) in enumerate(zip(r['U'], ref['U'])):
        print(k, relerr(U, Ur))
        assert relerr(U, Ur) <= tol, k
    assert relerr(r['Ep'], ref['Ep']) <= tol and abs(r['work'] - ref['work']) <= tol * abs(ref['work'])
    assert np.array_equal(r['kappa'], r['Ep'][3]) and (r['kappa'] >= 0).all() and r['kappa'].max() > 0
    assert np.array_equal(r['eps_p_bar'], np.sqrt(2 / 3) * r['kappa'])


def test_kappa_crosses_a_refinement_with_the_plastic_strain(fep):
    """One refinement in the middle of the cycle (P1, level 0, multigrid): the new context runs on the same curve, and row 3 of
    the transferred state is, bit for bit, the kappa of the parent point the transfer names (transfer_points copies a parent's
    rows; P1 has one point per element)."""
    table = ([0.0, 0.002, 0.01], [450.0, 480.0, 500.0])
    zetas = fep.vonmises.cycle_factors(4)
    kw = dict(level=0, linear_solver='amg', hardening=2000.0, isotropic=table)
    r = fep.solve_cutout_cyclic('P1', adapt_at=[3], zetas=zetas, **kw)
    assert r['failed_at'] is None and len(r['adapt']) == 1
    row = r['adapt'][0]
    parent_run = fep.solve_cutout_cyclic('P1', zetas=zetas[:4], **kw)   # the same history up to the refinement, on the parent mesh
    assert parent_run['failed_at'] is None and parent_run['n_plast'][-1] > 0
    kappa_parent = parent_run['Ep'][3]
    assert kappa_parent.max() > 0 and row['n_child'] > row['n_e']
    assert np.array_equal(row['Ep'][3], kappa_parent[row['parent']])
    assert np.array_equal(row['Ep'][:3], parent_run['Ep'][:3][:, row['parent']])
    assert (r['kappa'] >= 0).all() and (row['Ep'][3] >= 0).all() and r['kappa'].shape == (row['n_child'],)
    assert (r['kappa'] >= row['Ep'][3]).all() and r['kappa'].max() > row['Ep'][3].max()

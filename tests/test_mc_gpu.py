"""The Mohr-Coulomb kernels, the step of a Mohr-Coulomb context and the strip-footing driver on the GPU against the NumPy
restatement (tests/mc_ref.py).  Bounds: DESIGN.md section 7 — s, ds, ep 1e-13 of the array maximum and 1e-12 per point;
K, F 1e-12 of the array maximum and 1e-11 per row (F: a row per node); accepted displacements 1e-10 (1e-9 with the
multigrid solver).  Every input keeps the floors of tests/mc_cases.py, asserted on the restatement alone."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import dp_materials, relerr, relerr_points, relerr_rows
from mc_cases import (COHESION, EPS_Y, FOOTING, MIN_SHARE, P_BULK, P_SHEAR, SIN_PHI, cpu_footing, points, shares,
                      well_conditioned)
from mc_ref import MCRefContext, mc_return_map
from meshes import jitter, rect
from model_ref import bytes_equal, check_points, dev_return_map
from vm_cases import BULK as VM_BULK, HARDENING, SHEAR as VM_SHEAR, YIELD

pytestmark = pytest.mark.gpu

TOL, TOL_PT, TOL_K, TOL_K_ROW = 1e-13, 1e-12, 1e-12, 1e-11


def _check_points(got, ref, keys=('s', 'ds')):
    check_points(got, ref, keys, TOL, TOL_PT)


def _check_branches(got, ref):
    assert np.array_equal(got['ind_p'], ref['branch'] != 0)
    assert (got['n_smooth'], got['n_apex']) == (ref['n_smooth'], ref['n_apex'])


# ---------------------------------------------------------------------------------------
# the mesh-free kernel
# ---------------------------------------------------------------------------------------
def _dev_return_map(fep, e, order, p, sh, bu, sp, c, accept, e0):
    """fep_return_map_mc_dev -> the same dict as the host entry point, 'ep' the device copy of p."""
    return dev_return_map(fep, 'mc', e, order, p, e0, (sh, bu, sp, c), accept)


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('n', [1, 255, 257, 1000])
def test_mesh_free_return_map_host_and_dev(fep, n, order):
    for uniform in (True, False):
        e, p, e0, sh, bu, sp, c = points(n, uniform, 100 + n)
        ev = np.asfortranarray(e) if order == 'F' else np.ascontiguousarray(e)
        for with_ep, accept in ((False, False), (True, False), (True, True)):
            for z in (None, e0):
                ref = mc_return_map(e, p if with_ep else None, sh, bu, sp, c, apply_plastic_strain=accept, e0=z)
                assert well_conditioned(ref)
                if n == 1000:
                    print(shares(ref))
                    assert (shares(ref) >= MIN_SHARE).all()
                ph = p.copy() if with_ep else None
                host = fep.construct_constitutive_problem_mc(ev, ph, sh, bu, sp, c, apply_plastic_strain=accept, e0=z)
                dev = _dev_return_map(fep, e, order, p if with_ep else None, sh, bu, sp, c, accept, z)
                for got in (host, dev):
                    _check_branches(got, ref)
                    _check_points(got, ref)
                    if accept:
                        _check_points(got, ref, keys=('ep',))
                if with_ep and not accept:                                       # a non-accepting call leaves ep alone
                    assert np.array_equal(ph, p) and np.array_equal(dev['ep'], p)
                if accept:
                    assert host['ep'] is ph and np.array_equal(ph, p) == (not ref['ind_p'].any())   # (n = 1: maybe elastic)
    # accept without a plastic strain to update: the device entry point computes the same and writes nothing
    e, p, e0, sh, bu, sp, c = points(n, True, 100 + n)
    ref = mc_return_map(e, None, sh, bu, sp, c)
    got = _dev_return_map(fep, e, order, None, sh, bu, sp, c, True, None)
    _check_branches(got, ref)
    _check_points(got, ref)


# ---------------------------------------------------------------------------------------
# the step of a Mohr-Coulomb context
# ---------------------------------------------------------------------------------------
MESHES = {'P1': (12, 12), 'P2': (6, 6), 'Q1': (9, 9), 'Q2': (6, 6), 'P4': (5, 5)}      # as tests/test_vm_gpu.py
UNIFORM = (P_SHEAR, P_BULK, SIN_PHI, COHESION)


def _draw_case(fep, t, seed):
    rng = np.random.default_rng(seed)
    elem, coord = rect(t, *MESHES[t])
    coord = jitter(elem, coord, 0.15, rng)
    tab = fep.element_tables(fep.LagrangeElementType[t])
    ref = MCRefContext(elem, coord, *tab)
    n = ref.n_int
    assert n > 256 and n % 256 != 0                                         # several workgroups, the last one partial
    ref.set_materials(*UNIFORM)
    # growing eightfold from left to right, so that the right part is strained far enough for the apex
    U = rng.normal(0, 1.0, size=(2, coord.shape[1])) * (0.5 + 3.5 * coord[0] / coord[0].max())
    # without p and e0 the yield value is f = t * a - 2 c cos(phi) at U * t: the median point goes onto the yield surface
    r = mc_return_map(ref.orc.strain(ref.c['B'], U), None, *ref.m)
    k0 = 2 * COHESION * np.sqrt(1 - SIN_PHI ** 2)
    U *= k0 / np.median(r['f'] + k0)
    ep = EPS_Y * rng.normal(0, 0.25, size=(4, n))
    ep[[0, 1, 3]] -= (ep[0] + ep[1] + ep[3]) / 3 * rng.uniform(0.8, 1.0, n)
    f = rng.uniform(0.6, 1.4, n)
    per_point = (P_SHEAR * f, P_BULK * f[::-1], rng.uniform(0.2, 0.6, n), COHESION * rng.uniform(0.6, 1.4, n))
    e0 = EPS_Y * rng.normal(0, 0.2, size=(4, 1))
    return elem, coord, ref, U, ep, per_point, e0


@functools.lru_cache(maxsize=None)
def _case(fep, t):
    """Jittered mesh of type t (non-affine geometry), the CPU context on it, and a displacement / plastic strain at which
    about half of the points yield: the first seed whose points keep the floors in every call of the tests below."""
    for seed in range(170, 230):
        elem, coord, ref, U, ep, per_point, e0 = case = _draw_case(fep, t, seed + len(t) + ord(t[1]))
        ok = True
        for mats in (UNIFORM, per_point):
            ref.set_materials(*mats)
            ok = ok and well_conditioned(ref.step(U, ep.copy()))
        for p, z in ((None, None), (ep.copy(), e0)):                        # (ends on the uniform materials)
            ref.set_materials(*UNIFORM)
            ok = ok and well_conditioned(ref.step(U, p, e0=z))
        if ok:
            return case
    raise AssertionError('no seed keeps the floors')


def _check_step(got, ref, want_points=True):
    share = ref['ind_p'].mean()
    print('plastic share', share, np.bincount(ref['branch'], minlength=5))
    assert 0.2 <= share <= 0.8
    assert well_conditioned(ref)
    assert (got['n_smooth'], got['n_apex']) == (ref['n_smooth'], ref['n_apex'])
    if want_points:
        assert np.array_equal(got['ind_p'], ref['ind_p'])
        _check_points(got, ref, keys=('E', 's', 'ds'))
    K, Kr, F, Fr = got['K'], ref['K'], np.asarray(got['F']), np.asarray(ref['F'])
    ek = abs(K - Kr).max() / abs(Kr).max()
    print('K', ek, relerr_rows(K, Kr), 'F', relerr(F, Fr), relerr_rows(F.reshape(-1, 2), Fr.reshape(-1, 2)))
    assert ek <= TOL_K and relerr_rows(K, Kr) <= TOL_K_ROW
    assert relerr(F, Fr) <= TOL_K and relerr_rows(F.reshape(-1, 2), Fr.reshape(-1, 2)) <= TOL_K_ROW


@pytest.mark.parametrize('t', list(MESHES))
def test_step_of_a_mohr_coulomb_context(fep, t):
    elem, coord, ref, U, ep, per_point, e0 = _case(fep, t)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_model('mc')
    assert ctx.model == 'mc'
    every = ('E', 's', 'ds', 'ind_p', 'K', 'F')
    try:
        for mats in (UNIFORM, per_point):
            ctx.set_materials(*mats)
            ref.set_materials(*mats)
            # every output, accepting
            ep_g, ep_r = ep.copy(), ep.copy()
            got = ctx.step(U, ep_g, apply_plastic_strain=True, want=every)
            want = ref.step(U, ep_r, apply_plastic_strain=True)
            _check_step(got, want)
            print('ep', relerr(ep_g, ep_r), relerr_points(ep_g, ep_r))
            assert relerr(ep_g, ep_r) <= TOL and relerr_points(ep_g, ep_r) <= TOL_PT
            assert not np.array_equal(ep_r, ep)
        ctx.set_materials(*UNIFORM)
        ref.set_materials(*UNIFORM)
        want = ref.step(U, ep.copy())
        # K, F only: ds / s travel through the context's scratch
        ep_g = ep.copy()
        got = ctx.step(U, ep_g, want=('K', 'F'))
        assert sorted(k for k in got if k in every) == ['F', 'K'] and np.array_equal(ep_g, ep)
        _check_step(got, want, want_points=False)
        # no plastic strain given = zeros; with an initial strain
        _check_step(ctx.step(U, None, want=every), ref.step(U, None))
        _check_step(ctx.step(U, ep.copy(), e0=e0, want=every), ref.step(U, ep.copy(), e0=e0))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------
# the interface of the model switch
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'Q1'])
def test_model_switch_interface(fep, t):
    elem, coord, _, U, ep, _, _ = _case(fep, t)
    n = elem.shape[1] * fep.ELEMENT_SHAPE[fep.LagrangeElementType[t]][1]
    Udp = U * 0.5
    dp = fep.MeshContext(elem, coord)
    dp.set_materials(*dp_materials(n))
    vm = fep.MeshContext(elem, coord)
    vm.set_model('vm')
    vm.set_materials(VM_SHEAR, VM_BULK, HARDENING, YIELD)
    Uvm = U * 30.0                                                          # steel yields at a larger strain than the soil
    dp_before, vm_before = dp.step(Udp, np.zeros((4, n))), vm.step(Uvm, ep.copy())
    assert dp_before['n_smooth'] + dp_before['n_apex'] > 0 and vm_before['n_smooth'] > 0
    a = fep.MeshContext(elem, coord)
    a.set_model('mc')
    a.set_materials(*UNIFORM)
    b = fep.MeshContext(elem, coord)
    b.set_materials(*UNIFORM)
    b.set_model('mc')
    try:
        ra, rb = a.step(U, ep.copy()), b.step(U, ep.copy())
        assert ra['n_smooth'] > 0 and ra['n_apex'] > 0
        assert bytes_equal(ra, rb)                                         # the model before or after the materials
        assert bytes_equal(ra, a.step(U, ep.copy()))                       # two calls
        for which in (0, 1):
            assert 'mc_kernel' in a.kernel_names(which)
            assert 'mc' not in dp.kernel_names(which) and 'mc' not in vm.kernel_names(which)
            assert 'vm_kernel' in vm.kernel_names(which) and 'vm' not in a.kernel_names(which)
        # the Drucker-Prager and the von Mises context beside them
        assert bytes_equal(dp_before, dp.step(Udp, np.zeros((4, n))))
        assert bytes_equal(vm_before, vm.step(Uvm, ep.copy()))
        l = fep.lib()
        m = ctypes.c_int(-1)
        assert l.fep_ctx_model(a.handle, ctypes.byref(m)) == 0 and m.value == 2
        assert l.fep_ctx_model(vm.handle, ctypes.byref(m)) == 0 and m.value == 1
        assert l.fep_ctx_model(dp.handle, ctypes.byref(m)) == 0 and m.value == 0
        assert l.fep_ctx_set_model(a.handle, 7) == -1 and l.fep_ctx_set_model(None, 2) == -1       # FEP_EINVAL
        assert l.fep_ctx_model(a.handle, ctypes.byref(m)) == 0 and m.value == 2                    # a refused call changes nothing
        with pytest.raises(ValueError):
            a.set_model('tresca')
        assert a.model == 'mc'
        # back to Drucker-Prager: a context that never was a Mohr-Coulomb one computes the same
        b.set_model('dp')
        b.set_materials(*dp_materials(n))
        assert b.model == 'dp' and bytes_equal(dp_before, b.step(Udp, np.zeros((4, n))))
    finally:
        for c in (a, b, dp, vm):
            c.close()


# ---------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'Q2'])
def test_mohr_coulomb_step_dev_is_graph_capturable(fep, t):
    """fep_step_dev of a Mohr-Coulomb context allocates nothing (fep_ctx_set_model did): its first call on device buffers
    is captured, with K and F through the context's scratch, replayed, and equal bit for bit to the host-array entry point."""
    import torch
    elem, coord, _, U, ep, _, _ = _case(fep, t)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(*UNIFORM)
    ctx.set_model('mc')
    n = ctx.n_int
    want = ctx.step(U, ep.copy(), want=('ind_p', 'K', 'F'))
    dev = torch.device('cuda', 0)
    f64 = dict(dtype=torch.float64, device=dev)
    Ud = torch.from_numpy(np.ascontiguousarray(U.reshape(-1, order='F'))).to(dev)
    Ep = torch.from_numpy(ep).to(dev)
    ind = torch.zeros(n, dtype=torch.uint8, device=dev); Kd = torch.zeros(ctx.nnz, **f64); F = torch.zeros(ctx.n_dof, **f64)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.step_dev(torch.cuda.current_stream().cuda_stream, Ud.data_ptr(), ep=Ep.data_ptr(), ind_p=ind.data_ptr(),
                     k_data=Kd.data_ptr(), f_out=F.data_ptr(), counts=cnt.data_ptr())
    for x in (Kd, F, ind, cnt):
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert want['n_smooth'] > 0 and tuple(cnt.cpu().tolist()) == (want['n_smooth'], want['n_apex'])
    assert np.array_equal(Kd.cpu().numpy(), want['K'].data) and np.array_equal(F.cpu().numpy(), want['F'])
    assert np.array_equal(ind.cpu().numpy().astype(bool), want['ind_p'])
    ctx.close()


# ---------------------------------------------------------------------------------------
# the strip-footing driver
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver,tol', [('direct', 1e-10), ('amg', 1e-9)])
@pytest.mark.parametrize('case', FOOTING)
def test_footing_driver_against_the_cpu_run(fep, case, solver, tol):
    t, n_cells, max_steps = case
    ref = cpu_footing(*case)
    r = fep.solve_strip_footing(t, n_cells=n_cells, max_steps=max_steps, model='mc', linear_solver=solver)
    assert len(r['zeta']) == len(ref['zeta']) == max_steps and r['zeta'] == ref['zeta']
    assert [tuple(c) for c in r['counts']] == [tuple(c) for c in ref['counts']]
    assert r['prandtl_nc'] == ref['prandtl_nc']
    for k, (U, Ur) in enumerate(zip(r['U'], ref['U'])):
        print(k, relerr(U, Ur))
        assert relerr(U, Ur) <= tol, k
    assert relerr(r['pressure'], ref['pressure']) <= tol
    assert (r['pcg_iters'] is None) == (solver == 'direct')

"""The von Mises kernels, the step of a von Mises context and the cyclic driver on the GPU against the NumPy restatement
(tests/vm_ref.py).  Bounds: DESIGN.md section 7 — s, ds, ep 1e-13 of the array maximum and 1e-12 per point; K, F 1e-12
of the array maximum and 1e-11 per row (F: a row per node, its two components, as K's rows are compared against their
own largest entry); accepted displacements 1e-10 (1e-9 with the multigrid solver)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import dp_materials, relerr, relerr_points, relerr_rows
from meshes import jitter, rect
from model_ref import bytes_equal, check_points, dev_return_map, traceless
from vm_cases import BULK, HARDENING, SHEAR, YIELD, cpu_cycle
from vm_ref import VMRefContext, vm_return_map

pytestmark = pytest.mark.gpu

TOL, TOL_PT, TOL_K, TOL_K_ROW = 1e-13, 1e-12, 1e-12, 1e-11


def _check_points(got, ref, keys=('s', 'ds')):
    check_points(got, ref, keys, TOL, TOL_PT)


# ---------------------------------------------------------------------------------------
# 5, 6: the mesh-free kernel
# ---------------------------------------------------------------------------------------
def _points(n, uniform, seed):
    rng = np.random.default_rng(seed)
    one = np.ones(n)
    f = one if uniform else rng.uniform(0.6, 1.4, n)
    e = rng.normal(0, 3e-3, size=(3, n))
    p = traceless(rng, n, 1e-3)
    e0 = rng.normal(0, 1e-3, size=(4, 1))
    return e, p, e0, SHEAR * f, BULK * f[::-1], HARDENING * one if uniform else HARDENING * rng.uniform(0, 2, n), YIELD * f


def _dev_return_map(fep, e, order, p, sh, bu, a, Y, accept, e0):
    """fep_return_map_vm_dev -> the same dict as the host entry point, 'ep' the device copy of p."""
    r = dev_return_map(fep, 'vm', e, order, p, e0, (sh, bu, a, Y), accept)
    assert r['n_apex'] == 0
    return dict(r, n_plast=r['n_smooth'])


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('n', [1, 255, 257, 1000])
def test_mesh_free_return_map_host_and_dev(fep, n, order):
    for uniform in (True, False):
        e, p, e0, sh, bu, a, Y = _points(n, uniform, 100 + n)
        ev = np.asfortranarray(e) if order == 'F' else np.ascontiguousarray(e)
        for with_ep, accept in ((False, False), (True, False), (True, True)):
            for z in (None, e0):
                ref = vm_return_map(e, p if with_ep else None, sh, bu, a, Y, apply_plastic_strain=accept, e0=z)
                assert (np.abs(ref['crit']) >= 1e-9 * Y).all()                   # no point sits on the yield surface
                ph = p.copy() if with_ep else None
                host = fep.construct_constitutive_problem_vm(ev, ph, sh, bu, a, Y, apply_plastic_strain=accept, e0=z)
                dev = _dev_return_map(fep, e, order, p if with_ep else None, sh, bu, a, Y, accept, z)
                for got in (host, dev):
                    assert np.array_equal(got['ind_p'], ref['ind_p']) and got['n_plast'] == ref['n_plast']
                    _check_points(got, ref)
                    if accept:
                        _check_points(got, ref, keys=('ep',))
                if with_ep and not accept:                                       # a non-accepting call leaves ep alone
                    assert np.array_equal(ph, p) and np.array_equal(dev['ep'], p)
                if accept:
                    assert host['ep'] is ph
    # accept without a plastic strain to update: the device entry point computes the same and writes nothing
    e, p, e0, sh, bu, a, Y = _points(n, True, 100 + n)
    ref = vm_return_map(e, None, sh, bu, a, Y)
    got = _dev_return_map(fep, e, order, None, sh, bu, a, Y, True, None)
    assert np.array_equal(got['ind_p'], ref['ind_p']) and got['n_plast'] == ref['n_plast']
    _check_points(got, ref)


def test_vm_kernel_without_hardening_is_the_dp_kernel_without_friction(fep):
    """a = 0, Y = sqrt(2) c, traceless p: the two kernels compute the same law (eta = 0: no pressure term, no apex)."""
    rng = np.random.default_rng(6)
    n = 1000
    sh, bu, _, c = dp_materials(n)
    sh, c = sh * rng.uniform(0.7, 1.3, n), c * rng.uniform(0.7, 1.3, n)
    e = rng.normal(0, 1.2e-4, size=(3, n))
    p = traceless(rng, n, 4e-5)
    p_dp, p_vm = p.copy(), p.copy()
    dp = fep.construct_constitutive_problem(e, p_dp, sh, bu, np.zeros(n), c, apply_plastic_strain=True)
    vm = fep.construct_constitutive_problem_vm(e, p_vm, sh, bu, np.zeros(n), np.sqrt(2) * c, apply_plastic_strain=True)
    assert dp['n_apex'] == 0 and 0.2 < dp['n_smooth'] / n < 0.9
    assert np.array_equal(vm['ind_p'], dp['ind_p']) and vm['n_plast'] == dp['n_smooth']
    _check_points(vm, dp, keys=('s', 'ds', 'ep'))


# ---------------------------------------------------------------------------------------
# 7: the step of a von Mises context
# ---------------------------------------------------------------------------------------
MESHES = {'P1': (12, 12), 'P2': (6, 6), 'Q1': (9, 9), 'Q2': (6, 6), 'P4': (5, 5)}


@functools.lru_cache(maxsize=None)
def _case(fep, t):
    """Jittered mesh of type t (non-affine geometry), the CPU context on it, and a displacement / plastic strain at which
    about half of the points yield."""
    rng = np.random.default_rng(70 + len(t) + ord(t[1]))
    elem, coord = rect(t, *MESHES[t])
    coord = jitter(elem, coord, 0.15, rng)
    tab = fep.element_tables(fep.LagrangeElementType[t])
    ref = VMRefContext(elem, coord, *tab)
    n = ref.n_int
    assert n > 256 and n % 256 != 0                                         # several workgroups, the last one partial
    ref.set_materials(SHEAR, BULK, HARDENING, YIELD)
    U = rng.normal(0, 1.0, size=(2, coord.shape[1]))
    nrm = vm_return_map(ref.orc.strain(ref.c['B'], U), None, *ref.m)['crit'] + YIELD
    U *= YIELD / np.median(nrm)                                             # the median point sits on the yield surface
    ep = traceless(rng, n, 0.1 * YIELD / (2 * SHEAR))
    f = rng.uniform(0.6, 1.4, n)
    per_point = (SHEAR * f, BULK * f[::-1], HARDENING * rng.uniform(0, 2, n), YIELD * rng.uniform(0.6, 1.4, n))
    e0 = rng.normal(0, 0.2 * YIELD / (2 * SHEAR), size=(4, 1))
    return elem, coord, ref, U, ep, per_point, e0


def _check_step(got, ref, want_points=True):
    share = ref['ind_p'].mean()
    print('plastic share', share)
    assert 0.2 <= share <= 0.8
    assert np.abs(ref['crit']).min() > 0
    assert got['n_smooth'] == ref['n_smooth'] and got['n_apex'] == 0
    if want_points:
        assert np.array_equal(got['ind_p'], ref['ind_p'])
        _check_points(got, ref, keys=('E', 's', 'ds'))
    K, Kr, F, Fr = got['K'], ref['K'], np.asarray(got['F']), np.asarray(ref['F'])
    ek = abs(K - Kr).max() / abs(Kr).max()
    print('K', ek, relerr_rows(K, Kr), 'F', relerr(F, Fr), relerr_rows(F.reshape(-1, 2), Fr.reshape(-1, 2)))
    assert ek <= TOL_K and relerr_rows(K, Kr) <= TOL_K_ROW
    assert relerr(F, Fr) <= TOL_K and relerr_rows(F.reshape(-1, 2), Fr.reshape(-1, 2)) <= TOL_K_ROW


@pytest.mark.parametrize('t', list(MESHES))
def test_step_of_a_von_mises_context(fep, t):
    elem, coord, ref, U, ep, per_point, e0 = _case(fep, t)
    uniform = (SHEAR, BULK, HARDENING, YIELD)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_model('vm')
    assert ctx.model == 'vm'
    every = ('E', 's', 'ds', 'ind_p', 'K', 'F')
    try:
        for mats in (uniform, per_point):
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
        ctx.set_materials(*uniform)
        ref.set_materials(*uniform)
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
# 8: the interface of the model switch
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'Q1'])
def test_model_switch_interface(fep, t):
    elem, coord, _, U, ep, _, _ = _case(fep, t)
    n = elem.shape[1] * fep.ELEMENT_SHAPE[fep.LagrangeElementType[t]][1]
    Udp = U * 0.05                                                          # the Drucker-Prager demo material yields earlier
    dp = fep.MeshContext(elem, coord)
    dp.set_materials(*dp_materials(n))
    assert dp.model == 'dp'
    before = dp.step(Udp, np.zeros((4, n)))
    assert before['n_smooth'] + before['n_apex'] > 0
    a = fep.MeshContext(elem, coord)
    a.set_model('vm')
    a.set_materials(SHEAR, BULK, HARDENING, YIELD)
    b = fep.MeshContext(elem, coord)
    b.set_materials(SHEAR, BULK, HARDENING, YIELD)
    b.set_model('vm')
    try:
        ra, rb = a.step(U, ep.copy()), b.step(U, ep.copy())
        assert ra['n_smooth'] > 0
        assert bytes_equal(ra, rb)                                         # the model before or after the materials
        assert bytes_equal(ra, a.step(U, ep.copy()))                       # two calls
        for which in (0, 1):
            assert a.kernel_names(which) != dp.kernel_names(which) and 'vm_kernel' in a.kernel_names(which)
            assert 'vm' not in dp.kernel_names(which)
        assert bytes_equal(before, dp.step(Udp, np.zeros((4, n))))         # the Drucker-Prager context beside them
        l = fep.lib()
        m = ctypes.c_int(-1)
        assert l.fep_ctx_model(a.handle, ctypes.byref(m)) == 0 and m.value == 1
        assert l.fep_ctx_model(dp.handle, ctypes.byref(m)) == 0 and m.value == 0
        assert l.fep_ctx_set_model(a.handle, 7) == -1 and l.fep_ctx_set_model(None, 1) == -1       # FEP_EINVAL
        assert l.fep_ctx_model(None, ctypes.byref(m)) == -1 and l.fep_ctx_model(a.handle, None) == -1
        assert l.fep_ctx_model(a.handle, ctypes.byref(m)) == 0 and m.value == 1                    # a refused call changes nothing
        with pytest.raises(ValueError):
            a.set_model('tresca')
        # back to Drucker-Prager: a context that never was a von Mises one computes the same
        b.set_model('dp')
        b.set_materials(*dp_materials(n))
        assert b.model == 'dp' and bytes_equal(before, b.step(Udp, np.zeros((4, n))))
    finally:
        for c in (a, b, dp):
            c.close()


# ---------------------------------------------------------------------------------------
# 9: capture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ['P1', 'Q2'])
def test_von_mises_step_dev_is_graph_capturable(fep, t):
    """fep_step_dev of a von Mises context allocates nothing (fep_ctx_set_model did): its first call on device buffers is
    captured, with K and F through the context's scratch, replayed, and equal bit for bit to the host-array entry point."""
    import torch
    elem, coord, _, U, ep, _, _ = _case(fep, t)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(SHEAR, BULK, HARDENING, YIELD)
    ctx.set_model('vm')
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
    assert want['n_smooth'] > 0 and tuple(cnt.cpu().tolist()) == (want['n_smooth'], 0)
    assert np.array_equal(Kd.cpu().numpy(), want['K'].data) and np.array_equal(F.cpu().numpy(), want['F'])
    assert np.array_equal(ind.cpu().numpy().astype(bool), want['ind_p'])
    ctx.close()


# ---------------------------------------------------------------------------------------
# 10: the cyclic driver
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver,tol', [('direct', 1e-10), ('amg', 1e-9)])
@pytest.mark.parametrize('t', ['P1', 'Q2'])
def test_cyclic_driver_against_the_cpu_run(fep, t, solver, tol):
    ref = cpu_cycle(t, 200.0)
    assert ref['failed_at'] is None and max(ref['n_plast']) > 0
    r = fep.solve_cutout_cyclic(t, level=0, linear_solver=solver)
    assert r['failed_at'] is None and r['zeta'] == ref['zeta']
    assert relerr(r['f_ext'], ref['f_ext']) <= 1e-14                        # the traction kernel against the host sum
    assert r['n_plast'] == ref['n_plast']
    for k, (U, Ur) in enumerate(zip(r['U'], ref['U'])):
        print(k, relerr(U, Ur))
        assert relerr(U, Ur) <= tol, k
    assert relerr(r['Ep'], ref['Ep']) <= tol and abs(r['work'] - ref['work']) <= tol * abs(ref['work'])
    assert (r['pcg_iters'] is None) == (solver == 'direct')

"""The mesh-free kernel of the plane-stress von Mises model (return_map_vmps_kernel; fep_return_map_vmps_host / _dev) on the
GPU: against the fixtures of the high-precision reference with the bounds of DESIGN.md section 7 (vmps_cases.bound), on the
yield surface, at the wave and workgroup edges with every wave diverging in the Newton loop, against the plane-strain kernel
at the out-of-plane strain that makes its s33 vanish, on non-finite input (rules 1 and 2 of section 7), and on arenas that
show what the two entry points wrote."""
import functools

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401
from vmps_cases import (BULK, HARDENING, MARGIN, SHEAR, UNIT, YIELD, check, check_flags, check_surface, dev_return_map,
                        equivalence_points, errors, fixture, groups, merge, plane_strain_z3, surface_errors)
from vmps_ref import vmps_return_map

pytestmark = pytest.mark.gpu


def _host(fep, e, p, e0, mats, accept):
    r = fep.construct_constitutive_problem_vmps(e, p, *mats, apply_plastic_strain=accept, e0=e0)
    return dict(r, n_smooth=r['n_plast'], n_apex=0)


# ---------------------------------------------------------------------------------------
# 7, 8: the fixtures, and the yield surface
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['C', 'F'])
def test_kernel_against_the_high_precision_fixtures(fep, order):
    """Host and device entry points, both strain orders, with and without accept, and a launch without a plastic strain
    (ep_prev = NULL) on the points whose plastic strain is zero.  Every plastic point comes back on the yield surface."""
    fix = fixture()
    errs, surf = {}, {}
    for idx, e0 in groups(fix):
        n = idx.size
        assert n > 256 and n % 256 != 0
        e, p = fix['e'][:, idx], fix['p'][:, idx]
        ev = np.asfortranarray(e) if order == 'F' else np.ascontiguousarray(e)
        mats = [np.ascontiguousarray(fix[k][idx]) for k in ('G', 'K', 'm3', 'm4')]
        for accept in (False, True):
            ph = p.copy()
            host = _host(fep, ev, ph, e0, mats, accept)
            dev = dev_return_map(e, order, p, e0, mats, accept)
            for got, ep in ((host, ph), (dev, dev['ep'])):
                check_flags(fix, idx, got)
                assert not got['s'][3].any()
                if accept:
                    errs = merge(errs, errors(fix, dict(s=got['s'], ds=got['ds'], ep=ep), idx))
                    for k, v in surface_errors(fix, got['s'], ep, idx).items():
                        surf[k] = max(surf.get(k, 0.0), v)
                else:                                                   # a non-accepting call leaves ep alone
                    errs = merge(errs, errors(fix, dict(s=got['s'], ds=got['ds']), idx))
                    assert np.array_equal(ep, p)
        virgin = np.flatnonzero(~fix['p'][:, idx].any(axis=0))
        assert virgin.size >= 64
        sub = idx[virgin]
        m1 = [np.ascontiguousarray(fix[k][sub]) for k in ('G', 'K', 'm3', 'm4')]
        for got in (_host(fep, np.ascontiguousarray(fix['e'][:, sub]), None, e0, m1, False),
                    dev_return_map(fix['e'][:, sub], order, None, e0, m1, True)):
            check_flags(fix, sub, got)
            errs = merge(errs, errors(fix, dict(s=got['s'], ds=got['ds']), sub))
    check(errs)
    check_surface(surf)


# ---------------------------------------------------------------------------------------
# 9: launch shapes
# ---------------------------------------------------------------------------------------
N_MAX = 257


@functools.lru_cache(maxsize=None)
def _alternating():
    """257 steel points, elastic at the even lanes (half the yield radius) and plastic at the odd ones (overshoots 1.2 to 30,
    so that the lanes of a wave leave the loop after different numbers of iterations), and each of them launched alone."""
    rng = np.random.default_rng(9)
    n = N_MAX
    a = HARDENING * rng.uniform(0, 2, n)
    mats = [SHEAR * np.ones(n), BULK * np.ones(n), a, YIELD * np.ones(n)]
    e = rng.normal(size=(3, n))
    nrm = vmps_return_map(e, None, *mats)['crit'] + YIELD
    e *= YIELD * np.where(np.arange(n) % 2 == 0, 0.5, 10 ** rng.uniform(np.log10(1.2), 1.5, n)) / nrm
    ref = vmps_return_map(e, None, *mats)
    assert np.array_equal(ref['ind_p'], np.arange(n) % 2 == 1) and np.unique(ref['its'][1::2]).size >= 3
    alone = [dev_return_map(e[:, k:k + 1], 'C', np.zeros((4, 1)), None, [m[k:k + 1] for m in mats], True) for k in range(n)]
    return e, mats, {k: np.concatenate([r[k] for r in alone], axis=-1) for k in ('s', 'ds', 'ind_p', 'ep')}, \
        [r['n_smooth'] for r in alone]


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_launch_shapes_with_every_wave_diverging(fep, n):
    e, mats, alone, counts = _alternating()
    got = dev_return_map(e[:, :n], 'C', np.zeros((4, n)), None, [m[:n] for m in mats], True)
    for k in ('s', 'ds', 'ind_p', 'ep'):
        assert np.array_equal(got[k], alone[k][..., :n]), k
    assert (got['n_smooth'], got['n_apex']) == (n // 2, 0) and counts[:n] == [k % 2 for k in range(n)]
    assert np.array_equal(got['ind_p'], np.arange(n) % 2 == 1)


# ---------------------------------------------------------------------------------------
# 12: the plane-strain kernel with the out-of-plane strain free
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('a', [0.0, HARDENING])
def test_plane_strain_kernel_at_vanishing_s33_agrees(fep, a):
    """fep_return_map_vm_dev at z3*, solved per point on the host from the plane-strain restatement, and
    fep_return_map_vmps_dev: s[0:3] and the new p.  Bound: eight times what the two restatements give for the same comparison,
    measured here (per point, over the point's largest stress / plastic strain component)."""
    e, p, mats = equivalence_points(a)
    n = e.shape[1]
    r = vmps_return_map(e, p, *mats, True)
    plastic = np.flatnonzero(r['ind_p'])
    assert plastic.size >= 24
    sol = plane_strain_z3(e[:, plastic], p[:, plastic], mats)
    got = dev_return_map(e, 'C', p, None, [np.full(n, m) for m in mats], True)
    cpu, gpu = [0.0, 0.0], [0.0, 0.0]
    for (z3, q), k in zip(sol, plastic):
        ps = dev_return_map(e[:, k:k + 1], 'C', p[:, k:k + 1], np.array([0.0, 0.0, 0.0, z3]), [np.full(1, m) for m in mats], True,
                            entry='fep_return_map_vm_dev')
        assert ps['ind_p'][0] and got['ind_p'][k]
        for w, (s3, ep3, s, ep) in ((cpu, (q['s'], q['ep'], r['s'], r['ep'])), (gpu, (ps['s'], ps['ep'], got['s'], got['ep']))):
            w[0] = max(w[0], np.abs(s3[0:3, 0] - s[0:3, k]).max() / np.abs(s[:, k]).max())
            w[1] = max(w[1], np.abs(ep3[:, 0] - ep[:, k]).max() / np.abs(ep[:, k]).max())
    print('restatements', cpu, 'kernels', gpu)
    assert gpu[0] <= MARGIN * max(cpu[0], UNIT) and gpu[1] <= MARGIN * max(cpu[1], UNIT)


# ---------------------------------------------------------------------------------------
# 13: non-finite values
# ---------------------------------------------------------------------------------------
NAN, INF = float('nan'), float('inf')
N_POINTS = 3 * 256 + 1
LANES = (0, 63, 64, 255, 256, N_POINTS - 1)                             # the wave and workgroup edges of the ballot counters
# (array, row, value): a NaN in each of the four trial-strain components (component 3 lives in the plastic strain alone), and
# +-Inf in a normal strain
POISONS = (('e', 0, NAN), ('e', 1, NAN), ('e', 2, NAN), ('p', 3, NAN), ('e', 0, INF), ('e', 1, -INF))


@pytest.mark.parametrize('accept', [False, True])
def test_a_non_finite_trial_strain_is_elastic_with_a_nan_stress_and_contained(fep, accept):
    """Rule 1: ind_p = 0, the elastic tangent C, at least one NaN in s, p untouched, counted nowhere.  Rule 2: every clean
    point of the launch holds the bits of the launch without the poison.  The poisoned point is a plastic one."""
    fix = fixture()
    idx = np.flatnonzero((fix['family'] == 0) & ~fix['with_e0'])
    pts = idx[np.arange(N_POINTS) % idx.size]
    pts[list(LANES)] = idx[np.flatnonzero(fix['label'][idx] == 1)[0]]
    e, p = fix['e'][:, pts].copy(), fix['p'][:, pts].copy()
    mats = [np.ascontiguousarray(fix[k][pts]) for k in ('G', 'K', 'm3', 'm4')]
    clean = dev_return_map(e, 'C', p, None, mats, accept)
    assert clean['ind_p'][list(LANES)].all() and 0 < clean['n_smooth'] < N_POINTS
    ed, pd = e.copy(), p.copy()
    for lane, (arr, row, val) in zip(LANES, POISONS):
        (ed if arr == 'e' else pd)[row, lane] = val
    got = dev_return_map(ed, 'C', pd, None, mats, accept)
    dirty = np.zeros(N_POINTS, dtype=bool)
    dirty[list(LANES)] = True
    elastic = np.flatnonzero(~clean['ind_p'])[0]
    C = clean['ds'][:, elastic]                                         # uniform G, K: every elastic point's tangent
    assert np.array_equal(C, vmps_return_map(np.zeros((3, 1)), None, *[m[:1] for m in mats])['ds'][:, 0])
    for lane in LANES:
        assert not got['ind_p'][lane] and np.isnan(got['s'][:, lane]).any() and np.array_equal(got['ds'][:, lane], C), lane
    assert np.array_equal(got['ep'][:, dirty].view(np.int64), pd[:, dirty].view(np.int64))
    assert (got['n_smooth'], got['n_apex']) == (clean['n_smooth'] - len(LANES), 0)
    for k in ('s', 'ds', 'ind_p', 'ep'):
        assert np.array_equal(got[k][..., ~dirty], clean[k][..., ~dirty]), k
    host = _host(fep, ed, pd.copy(), None, mats, False)                 # the host entry point: the same bits, NaNs included
    for k in ('s', 'ds', 'ind_p'):
        assert np.ascontiguousarray(host[k]).tobytes() == np.ascontiguousarray(got[k]).tobytes(), k
    # a NaN in component 3 of e0 poisons every point of a launch
    every = dev_return_map(e, 'C', p, np.array([0.0, 0.0, 0.0, NAN]), mats, accept)
    assert not every['ind_p'].any() and np.isnan(every['s'][3]).all() and (every['n_smooth'], every['n_apex']) == (0, 0)
    assert np.array_equal(every['ep'], p) and np.array_equal(every['ds'], np.repeat(C.reshape(9, 1), N_POINTS, axis=1))


# ---------------------------------------------------------------------------------------
# 14: what the mesh-free entry points write
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 257])
@pytest.mark.parametrize('where', ['dev', 'host'])
def test_mesh_free_entry_points_write_their_outputs_and_nothing_else(fep, where, n):
    """tests/footprint.py: inputs and outputs in one poisoned arena with guard bands (device memory for _dev, host memory for
    _host): every output element is written, the guards, the strain, the materials and, unless accepting, the plastic strain
    keep their bits; accepting, the plastic strain of the elastic points does."""
    import ctypes
    import torch
    from footprint import Arena, fully_written, guards_intact, same_bits, unchanged
    e, mats, _, _ = _alternating()
    e, mats = e[:, :n], [m[:n] for m in mats]
    rng = np.random.default_rng(n)
    p = rng.normal(0, 1e-4, size=(4, n))
    p[3] = -(p[0] + p[1])
    e0 = np.zeros(4)
    first = None
    for accept in (False, True):
        for fill in (0xFF, 0x00):
            a = Arena('cuda:0' if where == 'dev' else 'cpu', fill=fill, capacity=4 << 20)
            ev, e_in = a.put(e, name='e')
            pv, p_in = a.put(p, name='ep')
            md = [a.put(m, name=f'material {i}') for i, m in enumerate(mats)]
            o = {'s': a.take((4, n), name='s'), 'ds': a.take((9, n), name='ds'), 'ind_p': a.take((n,), torch.uint8, name='ind_p'),
                 'counts': a.take((2,), torch.int64, name='counts')}
            tail = [n, ev.data_ptr(), 1, n, e0.ctypes.data_as(ctypes.c_void_p), pv.data_ptr(), *(m.data_ptr() for m, _ in md),
                    int(accept), o['s'].data_ptr(), o['ds'].data_ptr(), o['ind_p'].data_ptr(), o['counts'].data_ptr()]
            if where == 'dev':
                assert fep.lib().fep_return_map_vmps_dev(0, torch.cuda.current_stream().cuda_stream, *tail) == 0
                torch.cuda.synchronize()
            else:
                assert fep.lib().fep_return_map_vmps_host(0, *tail) == 0
            assert guards_intact(a)
            if fill == 0xFF:
                for k, v in o.items():
                    assert fully_written(v, name=k)
            assert unchanged(ev, e_in, 'strain')
            for i, (m, m_in) in enumerate(md):
                assert unchanged(m, m_in, f'material {i}')
            elastic = o['ind_p'] == 0
            assert int(o['counts'][0]) == int(o['ind_p'].sum()) == n // 2 and int(o['counts'][1]) == 0
            if accept:
                assert same_bits(pv[:, elastic], p_in[:, elastic], 'ep where ind_p is false')
                assert n == 1 or not torch.equal(pv, p_in)
            else:
                assert unchanged(pv, p_in, 'ep')
            if first is None:
                first = {k: v.clone() for k, v in o.items()}
            for k in o:                                                 # neither the fill nor the accept flag changes a bit
                assert same_bits(o[k], first[k], k)


def test_model_switch_and_the_mesh_free_field_pair(fep):
    """fep_ctx_set_model takes FEP_MODEL_VMPS = 3 and names the chain; the mesh-free pair with a field keeps its three models
    (FEP_EINVAL for this one: a field goes through the step of a context)."""
    import ctypes
    from meshes import rect
    elem, coord = rect('Q1', 3, 3)
    ctx = fep.MeshContext(elem, coord)
    try:
        ctx.set_model('vmps')
        ctx.set_materials(SHEAR, BULK, HARDENING, YIELD)
        m = ctypes.c_int(-1)
        assert fep.lib().fep_ctx_model(ctx.handle, ctypes.byref(m)) == 0 and m.value == 3 == fep.hotpath.MODELS['vmps']
        assert fep.lib().fep_ctx_set_model(ctx.handle, 4) == -1 and ctx.model == 'vmps'
        for which in (0, 1):
            assert ctx.kernel_names(which).startswith('point_vmps_kernel<4, 4> + element_kernel<4, 4, false')
        K = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
        assert abs(K - K.T).max() <= 1e-12 * abs(K).max() and np.isfinite(K.data).all()          # symmetric to rounding
    finally:
        ctx.close()
    e, p = np.zeros((3, 4)), np.zeros((4, 4))
    with pytest.raises(ValueError):
        fep.construct_constitutive_problem_field('vmps', e, p, p, SHEAR, BULK, HARDENING, YIELD)

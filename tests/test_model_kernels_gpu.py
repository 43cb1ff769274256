"""The point kernels of a context's step and the mesh-free kernel of the same model instantiate one return map
(model_return_map in csrc/fep_kernels.hip.h) and do nothing between the strain and the point outputs: fed the step's own
strain, the mesh-free entry point has to reproduce the step's point outputs byte for byte.  The 'vmi' model (isotropic
hardening on a curve) has kernels and a return map of its own (vmi_return_map, p1_point_vmi_kernel, point_vmi_kernel<NP, NQ>,
return_map_vmi_kernel) under the same claim: every element type, on the eight- and the four-segment curve."""
import numpy as np
import pytest

import test_mc_gpu
import test_vm_gpu
from conftest import dp_materials
from model_ref import dev_return_map
from test_vmi_gpu import _case as vmi_case
from vmi_cases import curve, dev_return_map as vmi_dev_return_map

pytestmark = pytest.mark.gpu


def _state(fep, model, t):
    """(elem, coord, U, ep, per-point materials, e0) on the jittered mesh of test_vm_gpu.MESHES: the state of the model's own
    step test; for Drucker-Prager the von Mises one at the 0.05 of test_vm_gpu.test_model_switch_interface (the demo material
    yields earlier), the demo materials +-40 % per point."""
    elem, coord, _, U, ep, per_point, e0 = (test_mc_gpu if model == 'mc' else test_vm_gpu)._case(fep, t)
    if model == 'dp':
        n = ep.shape[1]
        rng = np.random.default_rng(5)
        per_point = tuple(m * rng.uniform(0.6, 1.4, n) for m in dp_materials(n))
        U, ep, e0 = 0.05 * U, 0.05 * ep, 0.05 * e0
    return elem, coord, U, ep, per_point, e0


@pytest.mark.parametrize('t', ['P1', 'Q1'])
@pytest.mark.parametrize('model', ['dp', 'vm', 'mc'])
def test_point_kernels_share_the_return_map(fep, model, t):
    """288 elements (P1) or 324 points (Q1): two workgroups, the second one partial.  Drucker-Prager on Q1 steps through the
    fused element_kernel, which calls the same dp_return_map."""
    elem, coord, U, ep, mats, e0 = _state(fep, model, t)
    ctx = fep.MeshContext(elem, coord)
    try:
        ctx.set_model(model)
        ctx.set_materials(*mats)
        n = ctx.n_int
        assert 256 < n < 512 and n == {'P1': 288, 'Q1': 324}[t]
        names = ctx.kernel_names(0)
        tag = {'dp': '', 'vm': 'vm_', 'mc': 'mc_'}[model]
        assert names.startswith('element_kernel<4, 4, true' if (model, t) == ('dp', 'Q1') else
                                f'p1_point_{tag}kernel' if t == 'P1' else f'point_{tag}kernel<4, 4>'), names
        for accept in (False, True):
            ep_step = ep.copy()
            step = ctx.step(U, ep_step, e0=e0, apply_plastic_strain=accept, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
            free = dev_return_map(fep, model, step['E'], 'C', ep, e0, mats, accept)
            share = step['ind_p'].mean()
            print(model, t, accept, 'plastic share', share, step['n_smooth'], step['n_apex'])
            assert 0.2 <= share <= 0.8
            for k in ('s', 'ds', 'ind_p'):
                assert np.array_equal(free[k], step[k]), k
            assert (free['n_smooth'], free['n_apex']) == (step['n_smooth'], step['n_apex'])
            assert np.array_equal(free['ep'], ep_step)
            assert np.array_equal(ep_step, ep) == (not accept)
    finally:
        ctx.close()


@pytest.mark.parametrize('c', [2, 3])
@pytest.mark.parametrize('t', list(test_vm_gpu.MESHES))
def test_vmi_point_kernels_share_the_return_map(fep, t, c):
    """The step of a 'vmi' context (state of test_vmi_gpu._case: two workgroups or more, the last one partial) and
    fep_return_map_vmi_dev on the step's own strain, state, materials and curve."""
    elem, coord, _, U, ep, mats, e0, _ = vmi_case(fep, t)
    crv = curve(c)
    ctx = fep.MeshContext(elem, coord)
    try:
        ctx.set_model('vmi')
        ctx.set_materials(*mats)
        ctx.set_hardening(*crv)
        n = ctx.n_int
        assert n > 256 and n % 256 != 0
        assert ctx.kernel_names(0).startswith('p1_point_vmi_kernel' if t == 'P1' else f'point_vmi_kernel<{ctx.n_p}, {ctx.n_q}>')
        for accept in (False, True):
            ep_step = ep.copy()
            step = ctx.step(U, ep_step, e0=e0, apply_plastic_strain=accept, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
            free = vmi_dev_return_map(step['E'], 'C', ep, e0, mats, crv, accept)
            share = step['ind_p'].mean()
            print('vmi', t, c, accept, 'plastic share', share, step['n_smooth'])
            assert 0.2 <= share <= 0.8
            for k in ('s', 'ds', 'ind_p'):
                assert np.array_equal(free[k], step[k]), k
            assert (free['n_smooth'], free['n_apex']) == (step['n_smooth'], step['n_apex']) and step['n_apex'] == 0
            assert np.array_equal(free['ep'], ep_step)
            assert np.array_equal(ep_step, ep) == (not accept)
    finally:
        ctx.close()

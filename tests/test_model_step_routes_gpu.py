"""
The step of a von Mises, of a Mohr-Coulomb and of a 'vmi' context (von Mises with isotropic hardening on a piecewise-linear
curve; fep_api.hip: the staged plan of run_step, whose one point-stage launcher appends the curve where the model's ModelKernels says it has one) on every
route, against the element-by-element float64 reference (tests/elem_ref.py) and the models' restatements (tests/vm_ref.py,
tests/mc_ref.py, tests/vmi_ref.py), entry by entry.

Stage A of such a step is the model's own point kernel (p1_point_vm_kernel / p1_point_mc_kernel / p1_point_vmi_kernel,
point_vm_kernel<NP, NQ> / point_mc_kernel<NP, NQ> / point_vmi_kernel<NP, NQ>, asserted by name), stage B the context's
assembly from ds / s: p1_node_lds_kernel on the P1 node route, element_kernel<..., FROM_U = false> + fixup_kernel in the patch
form, element_kernel + csr_reduce + the force gather in the COO form.  The cases (tests/model_step_cases.py, checked on the
CPU by test_model_step_cases_host.py): the three models, every
element type, every route, the named meshes of test_element_route_gpu.py (one- and two-row strips, random numbering,
reversed elements, curved edges, 1 : 1000 cells, Delaunay) and three meshes of 256, 257 and 255 elements, at which n_int
modulo the point kernels' 256 lanes is 0, NQ and 256 - NQ.  A 'vmi' case runs on one of five curves, by its number: flat, one
linear segment, eight saturating segments, four with a softening one, or no set_hardening call at all (the context's default),
with kappa spread over the whole curve; from 1000 points on, every segment is the accepted one of three plastic points and more,
and as many cross a breakpoint.

The three decoupled stages of test_element_route_gpu.py, with its bounds as they are:
  1. E of the full-output step against ElemRef.strain(U):                        |dE| <= C_E u S_E
     and, where the kernels claim it (P2, Q1, Q2, P4 on both forms, P1 on the node route), E bit-equal to the E of a
     Drucker-Prager step of the same context (fep_kernels.hip.h: "dphi and E are bit-identical to theirs")
  2. s, ds, ind_p, both counters and the accepted ep against the restatement's return map applied to the KERNEL's E:
     DESIGN.md section 7, 1e-13 of the array maximum and 1e-12 per point.  Points within rounding of a branch boundary (von
     Mises: |crit| < 1e-9 Y; Mohr-Coulomb: under the floors of tests/mc_cases.py; 'vmi': |crit| < 1e-9 Y, or an accepted kappa
     within 1e-9 of a breakpoint, where the tangent jumps) are left out of the flag, ds and counter comparisons, at most 0.5 %
     of a case; their s and ep are compared like every point's.  'vmi', accepting: the strain rows of ep and kappa also each
     on their own (kappa is up to a thousand times the strains), kappa bit-equal to its input at the elastic points and
     larger at the plastic ones
  3. K and F against ElemRef.assemble of the KERNEL's ds and s:                  |dK_ij| <= C_K u S_ij, |dF_i| <= C_F u S_F,i
     (the P1 node route against the record form, and against the exact form on the widened scale with C + C_RECORD)
Every case also pins, bit for bit: the K,F-only, K-only and F-only steps (ds / s through the context's scratch) and
assemble(ds, s) to the full-output step, and the step without a plastic strain to the step with a zero one.

Measured worst ratios |delta| / (u S) (MI355X, both models, every case of this module), each beside the bound of
test_element_route_gpu.py it is held to (none fitted to these figures):
          E            K             F
    P1    3.41 (6)     3.98 (10)     3.32 (8)      node route; exact form, widened scale: K 3.86 (14), F 3.32 (12)
    P1    patch and COO forms: the same bounds, no figure recorded here
    P2    3.57 (8)     5.64 (16)     3.82 (12)
    Q1    3.20 (8)     4.53 (12)     3.79 (10)
    Q2    4.66 (8)     7.51 (16)     3.50 (10)
    P4    3.64 (8)    12.24 (24)     5.68 (12)
  von Mises alone: E 2.79 3.55 2.97 4.66 3.37, K 3.98 5.59 4.53 4.90 8.60, F 3.32 3.82 3.79 3.22 4.14; Mohr-Coulomb alone:
  E 3.41 3.57 3.20 3.63 3.64, K 3.88 5.64 4.03 7.51 12.24, F 3.12 3.79 3.76 3.50 5.68 (P1 node route, P2, Q1, Q2, P4).
  'vmi' alone, every case (P1 node route, P2, Q1, Q2, P4), beside the same bounds:
          E            K             F
    P1    3.13 (6)     4.19 (10)     3.77 (8)      node route; exact form, widened scale: K 4.12 (14), F 3.14 (12)
    P1    patch and COO forms: E 3.13, K 3.81, F 3.52
    P2    3.51 (8)     5.61 (16)     3.76 (12)
    Q1    4.06 (8)     5.01 (12)     3.68 (10)
    Q2    3.46 (8)     4.93 (16)     3.57 (10)
    P4    3.56 (8)     9.39 (24)     3.49 (12)
Stage 2, worst of the array maximum / per point: von Mises s 3.0e-16 / 8.9e-16, ds 4.7e-16 / 7.7e-16; Mohr-Coulomb s 5.2e-16 /
4.0e-15, ds 5.8e-16 / 7.3e-15; at most one point of a case left out.  'vmi' (bounds 1e-13 / 1e-12): s 4.0e-16 / 1.3e-15, ds
3.2e-16 / 5.7e-16, ep 2.7e-16 / 2.4e-15, its strain rows alone 4.0e-16 / 1.3e-14, kappa alone 2.5e-16 / 7.9e-15; no point left out.
E is bit-equal to the Drucker-Prager step's in every case that asserts it.

The P1 cases on FEP_ROUTE=patch | coo hold one thing more: the models' P1 point kernel takes the reference-element tables by
value (P1Tab), and a context that does not fill them on the element route returns NaN in E, s and F beside an elastic K;
p1_point_vmi_kernel takes them the same way.
"""
import numpy as np
import pytest

import model_step_cases as cases
from conftest import dp_materials, relerr, relerr_points
from elem_ref import ElemRef, ratio
from footprint import scrub
from routes import assert_route
from test_element_route_gpu import C_E, C_F, C_K, C_RECORD
from test_vmi_gpu import _expect_names

pytestmark = pytest.mark.gpu

TOL, TOL_PT = 1e-13, 1e-12
EVERY = ('E', 's', 'ds', 'ind_p', 'K', 'F')
WORST = {}                                                              # (model, t, route) -> worst (E, K, F) of the session


def _same(a, b, keys=('E', 's', 'ds', 'ind_p', 'F')):
    return all(np.array_equal(a[k], b[k]) for k in keys) and np.array_equal(a['K'].data, b['K'].data) \
        and (a['n_smooth'], a['n_apex']) == (b['n_smooth'], b['n_apex'])


@pytest.mark.parametrize('model,t,route,name', cases.cases())
def test_model_step_vs_reference_per_entry(fep, monkeypatch, model, t, route, name):
    c = cases.build(model, t, name)
    elem, coord, U, Ep, mats, e0, accept = (c[k] for k in ('elem', 'coord', 'U', 'ep', 'mats', 'e0', 'accept'))
    curve = c['curve']
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    ctx = fep.MeshContext(elem, coord)
    try:
        assert_route(ctx, 'patch' if route == 'default' else route)
        n_int = ctx.n_int
        # the strain of a Drucker-Prager step of this context, any valid materials
        ctx.set_materials(*dp_materials(n_int))
        E_dp = ctx.step(U, np.zeros((4, n_int)), want=EVERY)['E'].copy()
        ctx.set_model(model)
        ctx.set_materials(*mats)
        assert ctx.model == model and model + '_kernel' in ctx.kernel_names(0) and model + '_kernel' in ctx.kernel_names(1)
        if model == 'vmi':
            _expect_names(ctx, t, 'patch' if route == 'default' else route)
            if curve is None:                                           # the context's own curve: one segment of slope 0
                assert all(v.tolist() == [0.0] for v in ctx.hardening)
            else:
                ctx.set_hardening(*curve)
                assert all(np.array_equal(a, b) for a, b in zip(ctx.hardening, curve))
        kw = {} if e0 is None else {'e0': e0}
        ep = Ep.copy()                                                  # updated in place on accept
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
        scrub(ctx, U, Ep, kw)
        K2, F2 = ctx.assemble(full['ds'], full['s'])
        none = ctx.step(U, None, want=EVERY, **kw)
        zero = ctx.step(U, np.zeros((4, n_int)), want=EVERY, **kw)
        pattern = ctx.pattern()
    finally:
        ctx.close()
    # bitwise pins
    assert np.array_equal(kf['K'].data, full['K'].data) and np.array_equal(kf['F'], full['F'])
    assert np.array_equal(k_only['K'].data, full['K'].data) and np.array_equal(f_only['F'], full['F'])
    assert np.array_equal(K2.data, full['K'].data) and np.array_equal(F2, full['F'])
    assert _same(none, zero)
    for r in (kf, k_only, f_only):                                      # the counters do not depend on what is asked for
        assert (r['n_smooth'], r['n_apex']) == (full['n_smooth'], full['n_apex'])
    tab = fep.element_tables(t)
    ref = ElemRef(elem, coord, tab, pattern=pattern)
    # 1. strain
    E, S_E = ref.strain(U)
    r_E = ratio(full['E'], E, S_E)
    e_bits = np.array_equal(full['E'], E_dp)
    print(f'[E] {model} {t} {route} {name}: ratio {r_E:.2f}, bit-equal to the Drucker-Prager step: {e_bits}')
    assert r_E <= C_E[t], ('E', r_E)
    if t != 'P1' or route == 'node':
        assert e_bits
    # 2. return map on the kernel's strain
    o = cases.return_map(model, full['E'], Ep, mats, e0, accept, curve)
    excl = cases.excluded(model, o, mats, curve)
    keep = ~excl
    cases.check_conditions(model, o, excl, curve)
    assert np.array_equal(full['ind_p'][keep], o['ind_p'][keep])
    assert full['n_smooth'] + full['n_apex'] == int(full['ind_p'].sum())
    if keep.all():
        assert (full['n_smooth'], full['n_apex']) == (o['n_smooth'], o['n_apex'])
    else:                                                               # a left-out point may sit in either class
        n_out = int(excl.sum())
        assert int(full['ind_p'][keep].sum()) == int(o['ind_p'][keep].sum())
        assert abs(full['n_smooth'] - o['n_smooth']) <= n_out and abs(full['n_apex'] - o['n_apex']) <= n_out
    e_s = (relerr(full['s'], o['s']), relerr_points(full['s'], o['s']))
    e_ds = (relerr(full['ds'][:, keep], o['ds'][:, keep]), relerr_points(full['ds'][:, keep], o['ds'][:, keep]))
    print(f'[points] {model} {t} {route} {name}: left out {int(excl.sum())} of {n_int}, s {e_s[0]:.1e} / {e_s[1]:.1e}, '
          f'ds {e_ds[0]:.1e} / {e_ds[1]:.1e}')
    assert e_s[0] <= TOL and e_s[1] <= TOL_PT and e_ds[0] <= TOL and e_ds[1] <= TOL_PT
    if accept:
        e_p = (relerr(ep, o['ep']), relerr_points(ep, o['ep']))
        print(f'[points] ep {e_p[0]:.1e} / {e_p[1]:.1e}')
        assert e_p[0] <= TOL and e_p[1] <= TOL_PT
        assert not np.array_equal(ep, Ep)
        if model == 'vmi':
            # kappa is up to a thousand times the plastic strain beside it: the strain rows and kappa each on their own too
            for rows in (slice(0, 3), slice(3, 4)):
                e_r = (relerr(ep[rows], o['ep'][rows]), relerr_points(ep[rows], o['ep'][rows]))
                print(f'[points] ep rows {rows.start}:{rows.stop} {e_r[0]:.1e} / {e_r[1]:.1e}')
                assert e_r[0] <= TOL and e_r[1] <= TOL_PT
            # kappa, by the kernel's own flag: the input's bits at an elastic point, larger at a plastic one.  The multiplier
            # of a plastic point is positive on every curve here: its divisor Hj = 2G + a + slope_j is, the steepest softening
            # slope of the fixture's curves being -8000 against 2G >= 0.6 * 160 000, and at a kept point (|crit| >= 1e-9 Y)
            # it is at least 1e-12, a hundred thousand ulps of the largest kappa of a case
            P = full['ind_p'] & keep
            assert np.array_equal(ep[3][~full['ind_p'] & keep], Ep[3][~full['ind_p'] & keep])
            assert P.any() and (ep[3] > Ep[3])[P].all()
    else:
        assert np.array_equal(ep, Ep)
    # 3. assembly of the kernel's ds and s
    if route == 'node':
        rec = ElemRef(elem, coord, tab, pattern=pattern, record=True)
        K, S_K, F, S_F = rec.assemble(full['ds'], full['s'])
        r_K, r_F = ratio(full['K'].data, K, S_K), ratio(full['F'], F, S_F)
        Kx, W_K, Fx, W_F = ref.assemble(full['ds'], full['s'], widened=True)
        x_K, x_F = ratio(full['K'].data, Kx, W_K), ratio(full['F'], Fx, W_F)
        print(f'[ratios] {model} {t} {route} {name} E {r_E:.2f} K {r_K:.2f} F {r_F:.2f}; exact form, widened scale: '
              f'K {x_K:.2f} F {x_F:.2f}')
        assert x_K <= C_K[t] + C_RECORD, ('K, exact form', x_K)
        assert x_F <= C_F[t] + C_RECORD, ('F, exact form', x_F)
    else:
        K, S_K, F, S_F = ref.assemble(full['ds'], full['s'])
        r_K, r_F = ratio(full['K'].data, K, S_K), ratio(full['F'], F, S_F)
        print(f'[ratios] {model} {t} {route} {name} E {r_E:.2f} K {r_K:.2f} F {r_F:.2f}')
    w = WORST.get((model, t, route), (0.0, 0.0, 0.0))
    WORST[model, t, route] = (max(w[0], r_E), max(w[1], r_K), max(w[2], r_F))
    print('[worst] {} {} {}: E {:.2f} K {:.2f} F {:.2f}'.format(model, t, route, *WORST[model, t, route]))
    assert r_K <= C_K[t], ('K', r_K)
    assert r_F <= C_F[t], ('F', r_F)
    if name == 'mixed':
        assert (ref.det() < 0).mean() > 0.3

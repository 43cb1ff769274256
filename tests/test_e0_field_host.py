"""
The initial strain per point, on the CPU: what test_e0_field_gpu.py relies on is settled here, on the restatements alone.

  - every case of tests/e0_field_cases.py is the first draw of its generator that meets the conditions (plastic share /
    points per branch, at most 0.5 % of the points under the floors), with and without the previous plastic strain;
  - the per-point restatement (tests/e0_field_ref.py), called point by point, returns on a constant field the bits of the
    models' existing restatements called once with that (4, 1) strain: Drucker-Prager, von Mises, Mohr-Coulomb;
  - in_situ_strain is the strain whose elastic stress is s0, linear_in_situ the stated callable;
  - the K0 box's stress stays inside the yield surface of both layers at every load factor;
  - solve_tsx_tunnel with a uniform `in_situ` on the CPU context runs the load steps of the run without it (the driver's
    right-hand side, keywords and F0 with a field), and the body force reaches every residual;
  - the sharded TSX driver refuses `in_situ`.
"""
import numpy as np
import pytest

import e0_field_cases as fcases
import e0_field_ref as fref
from conftest import load_golden, relerr

POINT_CASES = sorted({(m, t, n) for m, t, _, n in fcases.grid()})


@pytest.mark.parametrize('model,t,name', POINT_CASES)
def test_case_meets_its_conditions(model, t, name):
    c = fcases.build(model, t, name)
    assert (c['curve'] is None) == (fcases.curve_id(model, t, name) is None)
    n = c['field'].shape[1]
    assert c['field'].shape == (4, n) == c['ep'].shape and c['draw'] < fcases.MAX_DRAWS
    assert (c['e0'] is None) == (c['scale'] == 1.0)
    nq = fcases.NQ[t]
    if name.startswith('block'):
        assert n % fcases.BLOCK == {'block255': fcases.BLOCK - nq, 'block256': 0, 'block257': nq}[name] % fcases.BLOCK
    # every row of the field differs from every other at every point: no stride or index error can cancel
    assert len(np.unique(c['field'])) == 4 * n


def test_every_type_meets_a_curve_of_several_segments_and_the_default():
    for t in fcases.TYPES:
        ids = [fcases.curve_id('vmi', t, n) for n in fcases.names(t)]
        assert len(set(ids)) == 4 and ({2, 3} & set(ids)), (t, ids)
    assert {fcases.curve_id('vmi', t, n) for t in fcases.TYPES for n in fcases.names(t)} == {0, 1, 2, 3, None}
    assert all(fcases.curve_id(m, t, n) is None for m, t, _, n in fcases.grid() if m != 'vmi')


def test_grid_covers_flags_for_every_model():
    for m in fcases.MODELS:
        seen = {fcases.flags(m, t, n) for mm, t, _, n in fcases.grid() if mm == m}
        assert len({f[1] for f in seen}) == 2 and len({f[0] for f in seen}) == 2 and len({f[2] for f in seen}) == 2


@pytest.mark.parametrize('model', fcases.MODELS)
@pytest.mark.parametrize('accept', [False, True])
def test_restatement_on_constant_field_is_the_existing_one_bit_for_bit(model, accept):
    E, ep, mats, e0, _ = fcases.mesh_free(model, 257, 0)
    z = np.repeat(e0, 257, axis=1)
    crv = fcases.cases.vmi_cases.curve(fcases.MESH_FREE_CURVE) if model == 'vmi' else None
    for p in (ep, None):
        got = fref.return_map(model, E, p, mats, z, accept, per_point=True, curve=crv)
        grouped = fref.return_map(model, E, p, mats, z, accept, curve=crv)
        ref = fref.plain_return_map(model, E, p, mats, e0, accept, crv)
        assert 0 < ref['ind_p'].sum() < 257
        for k in ('s', 'ds', 'ind_p', 'ep'):
            assert np.array_equal(got[k], ref[k]) and np.array_equal(grouped[k], ref[k]), k
        assert (got['n_smooth'], got['n_apex']) == (ref['n_smooth'], ref['n_apex'])
    # z = e0u + scale * field, the product rounded first
    f = np.random.default_rng(1).normal(size=(4, 5))
    assert np.array_equal(fref.z_of(e0, f, 0.37), e0 + np.float64(0.37) * f)
    assert np.array_equal(fref.z_of(None, f, 1.0), f)
    f[1, 2], f[3, 4] = np.inf, -np.inf                                  # an infinity counts as a NaN, and only where it stands
    z = fref.z_of(e0, f, 0.37)
    assert np.isnan(z[1, 2]) and np.isnan(z[3, 4]) and np.isnan(z).sum() == 2


def test_in_situ_strain_and_linear_in_situ(fep):
    rng = np.random.default_rng(2)
    n = 50
    s0 = rng.normal(0, 30.0, size=(4, n))
    G, K = rng.uniform(1e4, 3e4, n), rng.uniform(2e4, 5e4, n)
    e = fep.in_situ_strain(s0, G, K)
    tr = e[0] + e[1] + e[3]
    back = np.array([2 * G * (e[0] - tr / 3) + K * tr, 2 * G * (e[1] - tr / 3) + K * tr, G * e[2], 2 * G * (e[3] - tr / 3) + K * tr])
    assert relerr(back, s0) <= 1e-14
    assert np.array_equal(fep.in_situ_strain(s0, G[0], K[0]), fep.in_situ_strain(s0, G[0] * np.ones(n), K[0] * np.ones(n)))
    f = fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 2.0, (0.5, 1.0, 0.0, 0.25))
    x, y = rng.normal(size=n), rng.normal(size=n)
    got = f(x, y)
    assert got.shape == (4, n)
    for i, (a, g) in enumerate(zip((-45.0, -11.0, 0.0, -60.0), (0.5, 1.0, 0.0, 0.25))):
        assert np.array_equal(got[i], a + g * (y - 2.0))
    # the TSX demo's initial strain from its uniform stress (TSX:1675-1681)
    young, nu = 60000, 0.2
    s = np.array([-45.0, -11.0, 0.0, -60.0]).reshape(4, 1)
    tr0 = s[0] + s[1] + s[3]
    demo = np.array([-nu * tr0 + (1 + nu) * s[0], -nu * tr0 + (1 + nu) * s[1], [0.0], -nu * tr0 + (1 + nu) * s[3]]) / young
    assert relerr(fep.in_situ_strain(s, young / (2 * (1 + nu)), young / (3 * (1 - 2 * nu))), demo) <= 1e-15


def test_k0_types_have_exact_quadrature_tables():
    """Why the K0 box runs on P1 and Q1: their rules integrate what the identity needs to rounding, the P2 and P4 tables
    (13-digit points) do not."""
    d = {t: fcases.quadrature_defect(t, 1 if t == 'P1' else 3) for t in ('P1', 'P2', 'Q1', 'P4')}
    print(d)
    assert all(d[t] <= 8 * 2.0 ** -53 for t in fcases.K0_TYPES)
    assert d['P2'] > 1e-14 and d['P4'] > 1e-14


@pytest.mark.parametrize('t', fcases.K0_TYPES)
def test_k0_box_stays_inside_the_yield_surface(fep, t):
    b = fcases.k0_box(t)
    n = b['s0'].shape[1]
    assert (b['mats'][0] != b['mats'][0][0]).any()                      # two layers
    e = fep.in_situ_strain(b['s0'], b['mats'][0], b['mats'][1])
    for zeta in (1 / 17, 0.5, 1.0):
        r = fref.return_map('dp', np.zeros((3, n)), None, b['mats'], zeta * e, False)
        assert not r['ind_p'].any() and r['crit1'].max() < -1.0
        assert relerr(r['s'], zeta * b['s0']) <= 1e-14
    # equilibrium of the field with the body force: d s22 / dy = -f_y, s12 = 0, s11 constant in x
    assert b['body_force'] == (0.0, -fcases.GAMMA)


@pytest.fixture(scope='module')
def cpu_uniform_runs(fep):
    g = load_golden('tsx')
    plain = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', context_factory=fref.FieldContext)
    field = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', context_factory=fref.FieldContext,
                                 in_situ=fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 0.0, 0.0))
    return g, plain, field


def test_driver_with_uniform_field_on_cpu_context_is_the_plain_run(cpu_uniform_runs):
    g, plain, field = cpu_uniform_runs
    assert len(field['zeta']) == 17 == len(plain['zeta']) and field['n_plast'] == plain['n_plast'] == g['p1_nplast'].tolist()
    assert relerr(field['F0'], plain['F0']) <= 1e-14
    for a, b in zip(field['U'], plain['U']):
        assert relerr(a, b) <= 1e-10
    assert relerr(field['U'][-1], g['p1_U_final']) <= 1e-10
    assert len(field['s']) == 17 and field['s'][0].shape == (4, g['elem'].shape[1]) and 's' not in plain


def test_driver_body_force_reaches_f0_and_every_residual(fep):
    """One load step of the K0 box on the CPU context: with the body force the box stays at rest, without it the same
    field moves it (so F0 and the residuals carry f_V), and `body_force` alone is refused."""
    b = fcases.k0_box('P1')
    kw = dict(context_factory=fref.FieldContext, n_load_steps=2, materials=b['mats'], monitor=(0, 0))
    rest = fep.solve_tsx_tunnel(b['coord'], b['elem'], 'P1', in_situ=b['in_situ'], body_force=b['body_force'], **kw)
    moved = fep.solve_tsx_tunnel(b['coord'], b['elem'], 'P1', in_situ=b['in_situ'], **kw)
    assert len(rest['zeta']) == 2 == len(moved['zeta'])
    u_rest, u_moved = max(np.abs(u).max() for u in rest['U']), max(np.abs(u).max() for u in moved['U'])
    print('largest displacement at rest / without the body force:', u_rest, u_moved)
    assert u_moved > 1e-4 and u_rest <= 1e-9 * u_moved
    with pytest.raises(ValueError):
        fep.solve_tsx_tunnel(b['coord'], b['elem'], 'P1', body_force=(0.0, -1.0), **kw)


def test_sharded_tsx_driver_refuses_in_situ(fep):
    g = load_golden('tsx')
    with pytest.raises(ValueError):
        fep.solve_tsx_tunnel_sharded(g['coord'], g['elem'], 'P1', in_situ=fep.linear_in_situ((-45.0, -11.0, 0.0, -60.0), 0.0, 0.0))
    with pytest.raises(ValueError):
        fep.solve_tsx_tunnel_sharded(g['coord'], g['elem'], 'P1', body_force=(0.0, -1.0))

"""
Closed-form elasticity on the oracle (exact_cases.py): every element type must converge to the Lame solution at its
theoretical order, on straight and curved meshes, and reproduce a linear field exactly.  No GPU.

This file is the reference of tests/test_exact_solutions_gpu.py: it measures what that file's bounds are taken from
(exact_cases.MEASURED, exact_cases.PATCH) and asserts that it still finds those figures, and it holds every mesh to
exact_cases.check_mesh, the conditions the GPU file places on its inputs.

Meshes come from the host forms of refine_uniform(curves=) and create_midpoints(curves=), K from
oracle.fep_oracle.elastic_setup, the pressure from loads_ref.traction with the tables of loads_exact.edge_tables.
"""
import numpy as np
import pytest

import exact_cases as xc
import loads_ref
from conftest import relerr

ELASTIC_C = 1e12                                                             # cohesion of the patch test: no point yields


def oracle_K(elem, coord, tabs):
    from oracle import fep_oracle as orc
    n_int = elem.shape[1] * np.size(tabs[2])
    return orc.elastic_setup(elem, coord, xc.SHEAR * np.ones(n_int), xc.BULK * np.ones(n_int), *tabs)[0].tocsr()


def oracle_level(fep, name, level, m=None):
    """(mesh, K, U) of one level of a case on the oracle."""
    c = xc.CASES[name]
    if m is None:
        m = xc.mesh(fep, c['kind'], c['et'], level)
    xc.check_mesh(c, level, m)
    K = oracle_K(m['elem'], m['coord'], xc.tables(fep, c))
    f = None
    if c['load'] == 'pressure':
        edges, t, (hat, dhat, wf) = xc.wall_traction(m, c['et'])
        f = loads_ref.traction(edges, m['coord'], t, hat, dhat, wf)[0]
    return m, K, xc.solve(K, m, c['load'], f), f


@pytest.mark.parametrize('name', list(xc.CASES))
def test_convergence(fep, name):
    """Every level of the case: the order rule at the finest pair, and the figures of exact_cases.MEASURED.

    Q2 with the default tables is the one exception of the rule.  Its quadrature puts the 3 x 3 Gauss weights on the 2 x 2
    points +-1/sqrt(3) (tables.get_quadrature_volume keeps the reference's rule, the parity target).  The weights 25/81,
    40/81, 64/81 belong to the points +-sqrt(3/5) and 0: at +-1/sqrt(3) they give the integral of x^2 over the reference
    square as 180/243 instead of 4/3, so the element stiffness is not consistent, the element converges at first order in
    the energy norm and is less accurate than Q1 on the same mesh.  The kernels are not at fault.
    Only energy >= 0.8 and max >= 1.5 are asked (measured 0.96 and 1.80); with the true
    Gauss points passed as tables ('Q2 rect, Gauss') the rule holds with k = 2."""
    c = xc.CASES[name]
    errs = []
    for level in c['levels']:
        m, K, U, f = oracle_level(fep, name, level)
        errs.append(xc.errors(K, m, U))
    sens = relerr(xc.solve(xc.perturbed(K), m, c['load'], f), U)
    o_max, o_en = xc.orders(errs)[-1]
    print(f'{name!r}: (({o_max:.2f}, {o_en:.2f}), ({errs[-1][0]:.2e}, {errs[-1][1]:.2e}), {sens:.1e}),')
    least_max, least_en = xc.rule(name)
    assert o_max >= least_max and o_en >= least_en, (name, o_max, o_en)
    (r_max, r_en), (e_max, e_en), r_sens = xc.MEASURED[name]
    assert abs(o_max - r_max) <= 0.05 and abs(o_en - r_en) <= 0.05
    assert 0.5 <= errs[-1][0] / e_max <= 2 and 0.5 <= errs[-1][1] / e_en <= 2
    assert 0.5 <= sens / r_sens <= 2, sens
    assert xc.bound(name) <= 1e-9


def test_q2_default_is_less_accurate_than_q1(fep):
    """The consequence of the inherited Q2 rule, at n = 32: Q1's energy error is 6.4e-5, default Q2's 8.7e-3, and Q2 with the
    Gauss tables reaches a nodal error 5000 times smaller than default Q2."""
    e = {}
    for name in ('Q1 rect', 'Q2 rect', 'Q2 rect, Gauss'):
        m, K, U, _ = oracle_level(fep, name, 32)
        e[name] = xc.errors(K, m, U)
    assert e['Q2 rect'][1] > 100 * e['Q1 rect'][1]
    assert e['Q2 rect'][0] > 2000 * e['Q2 rect, Gauss'][0]


def test_unblended_curved_p4_misses_the_rule(fep):
    """What the rule is there to catch: the curved P4 ring with its interior nodes put back where the straight triangle has
    them (the enrichment before the blending rule) converges like P2, 3.1 / 2.7 between levels 2 and 3."""
    name = 'P4 ring, Dirichlet'
    errs = []
    for level in (2, 3):
        m = xc.mesh(fep, 'ring', 'P4', level)
        c1, e1 = fep.refine_uniform(*xc.ring_base(fep, range(6))[:2], levels=level, curves=xc.ring_base(fep, range(6))[2])
        straight = fep.create_midpoints_P4(c1, e1)
        assert np.array_equal(straight['elem_ext'], m['elem'])
        inner = m['elem'][12:15].ravel()
        moved = (m['coord'][:, inner] != straight['coord_ext'][:, inner]).any(axis=0)
        assert moved.sum() == 3 * 12 * 2 ** level                           # the elements of the two walls
        m['coord'] = m['coord'].copy()
        m['coord'][:, inner] = straight['coord_ext'][:, inner]
        m, K, U, _ = oracle_level(fep, name, level, m)
        errs.append(xc.errors(K, m, U))
    o_max, o_en = xc.orders(errs)[0]
    print('unblended P4, levels 2 -> 3:', o_max, o_en)
    assert o_max < 3.5 and o_en < 3.0


def oracle_patch(fep, elem, coord, tabs):
    """(E, F) of the linear field on the oracle: strain, elastic stress through the return map, internal force."""
    from oracle import fep_oracle as orc
    n_int = elem.shape[1] * np.size(tabs[2])
    one = np.ones(n_int)
    _, B, w, _, _, _ = orc.elastic_setup(elem, coord, xc.SHEAR * one, xc.BULK * one, *tabs)
    E = orc.strain(B, xc.linear(coord))
    cp = orc.return_map(E, np.zeros((4, n_int)), xc.SHEAR * one, xc.BULK * one, 0.1 * one, ELASTIC_C * one)
    assert cp['n_smooth'] == 0 and cp['n_apex'] == 0
    return E, orc.internal_force(B, w, cp['s'])


@pytest.mark.parametrize('name', xc.patch_names())
def test_patch(fep, name):
    """The linear field on every mesh: the strain at every point is the constant and the force at every interior DOF is zero,
    as ratios to ElemRef's u S_E and u S_F; the worst ratios are exact_cases.PATCH's."""
    elem, coord, inner = xc.patch_mesh(fep, name)
    assert inner.any() and not inner.all()
    tabs = xc.patch_tables(fep, name)
    E, F = oracle_patch(fep, elem, coord, tabs)
    r_e, r_f = xc.patch_ratios(elem, coord, tabs, inner, E, F)
    print(f'{name!r}: ({r_e:.2f}, {r_f:.2f}),')
    assert r_e <= 2 * xc.PATCH[name][0] and r_f <= 2 * xc.PATCH[name][1]
    # the boundary carries the reaction of the constant stress: the test would not pass on a field without stress
    assert np.abs(F[xc.dof_mask(~inner)]).max() > 1e-3 * max(np.abs(xc.linear_stress())) * np.ptp(coord[0]) / elem.shape[1]


def test_default_q2_fails_the_patch_test_on_distorted_elements(fep):
    """The other consequence of the inherited Q2 rule: on elements that are no parallelograms the integrand of the internal
    force is not constant, and the 3 x 3 weights at the 2 x 2 points leave a force of 8 % of its scale at interior nodes
    where the Gauss tables leave rounding.  The strain, which no quadrature enters, is exact with both."""
    elem, coord, inner = xc.patch_mesh(fep, 'Q2 curved')
    tabs = fep.element_tables('Q2')
    r_e, r_f = xc.patch_ratios(elem, coord, tabs, inner, *oracle_patch(fep, elem, coord, tabs))
    print('default Q2 on the curved mesh:', r_e, r_f * xc.U_RND)
    assert r_e <= 2 * xc.PATCH['Q2 curved'][0] and r_f * xc.U_RND > 0.01

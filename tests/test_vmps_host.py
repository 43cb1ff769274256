"""The plane-stress von Mises model on the CPU: the fixtures of the high-precision reference (tests/vmps_mp.py,
tests/golden/make_golden_return_map_mp_vmps.py) are reproduced by their generator, the float64 restatement's errors against
them are the table of DESIGN.md section 7 (vmps_cases.MEASURED and SURFACE_MEASURED, from which the bounds of the GPU tests
derive), the restatement reproduces the uniaxial closed form, and it equals the plane-strain law at the out-of-plane strain
that makes s33 vanish."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT  # noqa: F401
from vm_ref import vm_return_map
from vmps_cases import (BULK, FAMILIES, HARDENING, MAX_ITERATIONS, MEASURED, POISSON, SHEAR, SIGMA_Y, SURFACE_MEASURED, YIELD,
                        YOUNG, check, check_flags, check_surface, equivalence_points, errors, fixture, groups, merge, plane_strain_z3,
                        surface_errors, uniaxial)
from vmps_ref import MAX_ITER, elastic_matrix, vmps_return_map

sys.path.insert(0, GOLDEN)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def restatement(fix, idx, e0):
    mats = [fix[k][idx] for k in ('G', 'K', 'm3', 'm4')]
    r = vmps_return_map(fix['e'][:, idx], fix['p'][:, idx], *mats, apply_plastic_strain=True, e0=e0)
    return dict(r, n_smooth=r['n_plast'], n_apex=0)


def test_restatement_errors_are_the_recorded_tables():
    """Every figure of both tables is reproduced (within its rounding up to two digits), eight times each of them, capped by the
    standing bounds, holds for the restatement itself, and so does the recorded iteration count, well under the cap."""
    fix = fixture()
    errs, surf, its = {}, {}, 0
    for idx, e0 in groups(fix):
        r = restatement(fix, idx, e0)
        check_flags(fix, idx, r)
        errs = merge(errs, errors(fix, r, idx))
        for k, v in surface_errors(fix, r['s'], r['ep'], idx).items():
            surf[k] = max(surf.get(k, 0.0), v)
        its = max(its, int(r['its'].max()))
    for k, (wide, pt) in sorted(errs.items()):
        print(*k, f'{wide:.2e} {pt:.2e}', MEASURED[k])
        assert wide <= MEASURED[k][0] <= 2 * wide + 1e-17 and pt <= MEASURED[k][1] <= 2 * pt + 1e-17, k
    assert set(errs) == set(MEASURED)
    for k, v in sorted(surf.items()):
        print(k, f'{v:.2e}', SURFACE_MEASURED[k])
        assert v <= SURFACE_MEASURED[k] <= 2 * v + 1e-17, k
    assert set(surf) == set(SURFACE_MEASURED)
    check(errs)
    check_surface(surf)
    print('iterations', its)
    assert its == MAX_ITERATIONS and 2 * its <= MAX_ITER


def test_generator_reproduces_the_fixtures():
    """The inputs of every family but E entirely and two pairs per hardening modulus of E (the bisection runs on the
    reference), and the reference itself at 40 points spread over all families: bit for bit."""
    import make_golden_return_map_mp_vmps as gen
    fix = fixture()
    inp = gen.inputs(n_pairs=2)
    fam_new, fam_old = inp['family'], fix['family']
    for f in range(len(FAMILIES)):
        new, old = np.flatnonzero(fam_new == f), np.flatnonzero(fam_old == f)
        if FAMILIES[f] == 'E':
            old = old.reshape(2, -1)[:, :4].ravel()
        assert new.size == old.size
        for k in ('e', 'p', 'with_e0', 'G', 'K', 'm3', 'm4'):
            assert _bits(inp[k][..., new]) == _bits(fix[k][..., old]), (FAMILIES[f], k)
    assert np.array_equal(inp['e0'], fix['e0'])
    idx = np.unique(np.concatenate([np.flatnonzero(fam_old == f)[np.linspace(0, (fam_old == f).sum() - 1, 8).astype(int)]
                                    for f in np.unique(fam_old)]))
    out = gen.outputs(fix, idx)
    for k in gen.OUTPUT_KEYS:
        assert _bits(out[k]) == _bits(fix[k][..., idx]), k
    gen.check_conditions(fix)
    assert set(fix) == set(gen.INPUT_KEYS) | set(gen.OUTPUT_KEYS)


def test_uniaxial_closed_form():
    """sigma > sigma_y from a virgin state: eps11 = sigma / E + (sigma - sigma_y) / (1.5 a), eps22 = -nu sigma / E - half the
    plastic part give s = (sigma, 0, 0, 0), p = (ep, -ep / 2, 0, -ep / 2) and the uniaxial tangent E 1.5 a / (E + 1.5 a)."""
    for sigma in (451.0, 600.0, 2000.0):
        e, s, p, Et = uniaxial(sigma)
        r = vmps_return_map(e.reshape(3, 1), None, SHEAR, BULK, HARDENING, YIELD, True)
        d = r['ds'][:, 0].reshape(3, 3)
        print(sigma, r['s'][:, 0], r['ep'][:, 0], d[0, 0] - d[0, 1] ** 2 / d[1, 1], Et)
        assert r['ind_p'][0]
        assert np.abs(r['s'][:, 0] - s).max() <= 1e-13 * sigma and r['s'][3, 0] == 0
        assert np.abs(r['ep'][:, 0] - p).max() <= 1e-12 * np.abs(p).max()
        assert abs(d[0, 0] - d[0, 1] ** 2 / d[1, 1] - Et) <= 1e-12 * Et
        assert np.array_equal(d, d.T)


def test_yield_is_at_sigma_y_and_plane_strain_yields_later():
    """Elastic at sigma_y (1 - 1e-9), plastic at sigma_y (1 + 1e-9); the plane-strain model is elastic at both, and in it the
    strip yields at sigma_y / sqrt(1 - nu + nu^2)."""
    for f, plastic in ((1 - 1e-9, False), (1 + 1e-9, True)):
        sigma = SIGMA_Y * f
        e = np.array([sigma / YOUNG, -POISSON * sigma / YOUNG, 0.0]).reshape(3, 1)
        r = vmps_return_map(e, None, SHEAR, BULK, HARDENING, YIELD)
        assert bool(r['ind_p'][0]) == plastic
        assert not vm_return_map(e, None, SHEAR, BULK, HARDENING, YIELD)['ind_p'][0]
    # plane strain, eps22 free: sigma11 = s, sigma33 = nu s
    for f, plastic in ((1 - 1e-9, False), (1 + 1e-9, True)):
        s11 = SIGMA_Y / np.sqrt(1 - POISSON + POISSON ** 2) * f
        e = np.array([(1 - POISSON ** 2) * s11 / YOUNG, -POISSON * (1 + POISSON) * s11 / YOUNG, 0.0]).reshape(3, 1)
        assert bool(vm_return_map(e, None, SHEAR, BULK, HARDENING, YIELD)['ind_p'][0]) == plastic


def test_elastic_tangent_is_the_plane_stress_matrix():
    r = vmps_return_map(np.zeros((3, 1)), None, SHEAR, BULK, HARDENING, YIELD)
    C = np.array([[1, POISSON, 0], [POISSON, 1, 0], [0, 0, (1 - POISSON) / 2]]) * YOUNG / (1 - POISSON ** 2)
    assert np.abs(r['ds'][:, 0].reshape(3, 3) - C).max() <= 4e-16 * C.max()
    assert np.array_equal(r['ds'][:, 0].reshape(3, 3), elastic_matrix(SHEAR, BULK)[1])


@pytest.mark.parametrize('a', [0.0, HARDENING])
def test_equals_plane_strain_with_the_out_of_plane_strain_free(a):
    """The law is the plane-strain law at the z3 where its s33 vanishes, for traceless p: in-plane stress and new p."""
    e, p, mats = equivalence_points(a)
    r = vmps_return_map(e, p, *mats, True)
    assert r['ind_p'].sum() >= 20
    worst = [0.0, 0.0]
    for k, (z3, q) in enumerate(plane_strain_z3(e, p, mats)):
        assert abs(q['s'][3, 0]) <= 1e-12 * YIELD and bool(q['ind_p'][0]) == bool(r['ind_p'][k])
        worst[0] = max(worst[0], np.abs(q['s'][0:3, 0] - r['s'][0:3, k]).max() / np.abs(r['s'][:, k]).max())
        worst[1] = max(worst[1], np.abs(q['ep'][:, 0] - r['ep'][:, k]).max() / np.abs(r['ep'][:, k]).max())
    print(worst)
    assert worst[0] <= 1e-13 and worst[1] <= 1e-12

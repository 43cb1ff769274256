"""The NumPy restatement of the von Mises model (tests/vm_ref.py) against the pinned Drucker-Prager restatement, against its
own yield condition and against finite differences, and the cyclic driver on it.  No GPU."""
import numpy as np
import pytest

from conftest import relerr, relerr_points
from model_ref import traceless
from vm_cases import BULK, HARDENING, SHEAR, YIELD, cpu_cycle
from vm_ref import vm_return_map


def test_reduces_to_drucker_prager_without_friction():
    """a = 0, Y = sqrt(2) c, traceless p: the model is Drucker-Prager at eta = 0 (no pressure term, no apex)."""
    from oracle import fep_oracle as orc
    rng = np.random.default_rng(11)
    n = 4000
    sh = 3.4e6 * rng.uniform(0.7, 1.3, n)
    bu = 8.3e7 * rng.uniform(0.7, 1.3, n)
    c = 400.0 * rng.uniform(0.7, 1.3, n)
    e = rng.normal(0, 1.2e-4, size=(3, n))
    p = traceless(rng, n, 4e-5)
    ref = orc.return_map(e.copy(), p.copy(), sh, bu, np.zeros(n), c, apply_plastic_strain=True)
    got = vm_return_map(e, p, sh, bu, np.zeros(n), np.sqrt(2) * c, apply_plastic_strain=True)
    share = ref['ind_p'].mean()
    assert 0.2 < share < 0.9 and ref['n_apex'] == 0
    assert np.array_equal(got['ind_p'], ref['ind_p']) and got['n_plast'] == ref['n_smooth']
    for k in ('s', 'ds', 'ep'):
        print(k, relerr(got[k], ref[k]), relerr_points(got[k], ref[k]))
        assert relerr(got[k], ref[k]) <= 1e-13 and relerr_points(got[k], ref[k]) <= 1e-12


def _benchmark_points(rng, n):
    one = np.ones(n)
    e = rng.normal(0, 3e-3, size=(3, n))
    p = traceless(rng, n, 1e-3)
    return e, p, SHEAR * one, BULK * one, HARDENING * one, YIELD * one


def test_accepted_state_lies_on_the_yield_surface():
    rng = np.random.default_rng(12)
    n = 3000
    e, p, sh, bu, a, Y = _benchmark_points(rng, n)
    r = vm_return_map(e, p, sh, bu, a, Y, apply_plastic_strain=True)
    pl = r['ind_p']
    assert 0.2 < pl.mean() < 0.9
    s, pn = r['s'][:, pl], r['ep'][:, pl]
    tr = (s[0] + s[1] + s[3]) / 3
    xi = np.array([s[0] - tr, s[1] - tr, s[2], s[3] - tr]) - a[pl] * np.array([pn[0], pn[1], pn[2] / 2, pn[3]])
    nrm = np.sqrt(xi[0] ** 2 + xi[1] ** 2 + 2 * xi[2] ** 2 + xi[3] ** 2)
    print(np.abs(nrm / Y[pl] - 1).max())
    assert np.abs(nrm / Y[pl] - 1).max() <= 1e-13
    assert np.abs(pn[0] + pn[1] + pn[3]).max() <= 1e-13 * np.abs(pn).max()
    assert np.array_equal(r['ep'][:, ~pl], p[:, ~pl])                      # elastic points keep their plastic strain


def test_tangent_is_the_derivative_of_the_stress():
    """ds against central differences of s(e): second order, so halving h divides the error by four."""
    rng = np.random.default_rng(13)
    n = 2000
    e, p, sh, bu, a, Y = _benchmark_points(rng, n)
    r = vm_return_map(e, p, sh, bu, a, Y)
    keep = np.abs(r['crit']) > 0.05 * Y
    assert keep.mean() >= 0.9 and 0.2 < r['ind_p'][keep].mean() < 0.9
    ds = r['ds'].reshape(3, 3, n)
    err = []
    for h in (1e-6, 5e-7):
        fd = np.empty((3, 3, n))
        for j in range(3):
            d = np.zeros((3, 1))
            d[j] = h
            fd[:, j] = (vm_return_map(e + d, p, sh, bu, a, Y)['s'][0:3] - vm_return_map(e - d, p, sh, bu, a, Y)['s'][0:3]) / (2 * h)
        err.append(relerr(fd[:, :, keep], ds[:, :, keep]))
    print(err)
    assert 3.5 <= err[0] / err[1] <= 4.5


def test_elastic_cycle_is_linear_in_the_load_factor():
    r = cpu_cycle('P1', 20.0)
    assert r['failed_at'] is None and len(r['zeta']) == 16 and r['zeta'][-1] == 0.0
    assert max(r['n_plast']) == 0
    U1 = r['U'][0] / r['zeta'][0]
    for z, U in zip(r['zeta'], r['U']):
        assert np.abs(U - z * U1).max() <= 1e-10 * np.abs(U1).max()


def test_plastic_cycle_shows_hysteresis():
    r = cpu_cycle('P1', 200.0)
    z, n_plast = np.array(r['zeta']), r['n_plast']
    print(n_plast, r['newton_its'], r['work'])
    assert r['failed_at'] is None and len(z) == 16
    assert r['Ep'].shape == (4, 150)
    i_up, i_down = int(np.argmax(z)), int(np.argmin(z))
    assert z[i_up] == 1.0 and z[i_down] == -1.0
    assert n_plast[i_up] > 0 and n_plast[i_down] > 0
    assert n_plast[i_up + 1] == 0 and n_plast[i_down + 1] == 0              # the first step after each reversal is elastic
    i_zero = int(np.flatnonzero(z == 0.0)[0])
    assert i_up < i_zero < i_down and np.abs(r['U'][i_zero]).max() > 1e-8 * np.abs(r['U'][i_up]).max()
    assert r['work'] > 0
    assert max(r['newton_its']) <= 25

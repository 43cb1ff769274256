"""The NumPy restatement of the Mohr-Coulomb model (tests/mc_ref.py) against the conditions that define the closest-point
projection onto the yield surface, against finite differences, and the strip-footing driver on it.  No GPU."""
import functools

import numpy as np
import pytest
from scipy.optimize import nnls

from conftest import relerr_points
from mc_cases import (COHESION, DIST_FLOOR, EPS_Y, FOOTING, MIN_SHARE, P_BULK, P_SHEAR, PHI, R_FLOOR, cpu_footing, points,
                      shares, well_conditioned)
from mc_ref import mc_return_map

N = 2400


@functools.lru_cache(maxsize=None)
def _run(uniform, accept=False):
    e, p, e0, sh, bu, sp, c = points(N, uniform, 21)
    return mc_return_map(e, p, sh, bu, sp, c, apply_plastic_strain=accept, e0=e0)


def _principal(uniform):
    """Sorted principal trial strains and stresses, the plastic strain increment in that frame and the parameters."""
    _, _, _, sh, bu, sp, c = points(N, uniform, 21)
    r = _run(uniform)
    e = np.array(r['principal']['e'])
    sig = np.array(r['principal']['sig'])
    lam = bu - 2 * sh / 3
    th = sig.sum(axis=0) / (3 * bu)
    dep = e - (sig - lam * th) / (2 * sh)                                   # C^-1 (sig_tr - sig)
    return r, e, sig, dep, sh, bu, sp, c


@pytest.mark.parametrize('uniform', [True, False])
def test_inputs_reach_every_branch_and_keep_the_floors(uniform):
    r = _run(uniform)
    print(shares(r), r['r_rel'].min(), r['dist'].min())
    assert r['branch'].size >= 2000 and (shares(r) >= MIN_SHARE).all()
    assert well_conditioned(r) and R_FLOOR >= 1e-2 and DIST_FLOOR >= 1e-6


@pytest.mark.parametrize('uniform', [True, False])
def test_plastic_stress_is_ordered_and_on_the_yield_surface(uniform):
    r, _, sig, _, _, _, sp, c = _principal(uniform)
    pl = r['ind_p']
    scale = np.abs(sig).max(axis=0) + c
    assert ((sig[0] - sig[1] >= -1e-13 * scale) & (sig[1] - sig[2] >= -1e-13 * scale))[pl].all()
    F = (1 + sp) * sig[0] - (1 - sp) * sig[2] - 2 * c * np.sqrt(1 - sp * sp)
    print(np.abs(F / scale)[pl].max(), (F / scale)[~pl].max())
    assert np.abs(F / scale)[pl].max() <= 1e-13
    assert (F[~pl] < 0).all() and (r['f'][~pl] < 0).all()                  # elastic: the trial stress is admissible
    # edges and apex: the merged stresses are equal
    b = r['branch']
    assert np.abs(sig[0] - sig[1])[b == 2].max() <= 1e-13 * scale[b == 2].max()
    assert np.abs(sig[1] - sig[2])[b == 3].max() <= 1e-13 * scale[b == 3].max()
    assert np.array_equal(sig[0][b == 4], sig[2][b == 4])


def _plane(sp, i, j):
    n = np.zeros(3)
    n[i], n[j] = 1 + sp, -(1 - sp)
    return n


@pytest.mark.parametrize('uniform', [True, False])
def test_plastic_strain_increment_lies_in_the_normal_cone(uniform):
    """C^-1 (sig_tr - sig) is a non-negative combination of the normals of the planes active in the branch: the face's own
    normal, the two planes that meet in an edge, all six at the apex (non-negative least squares).  With ordering and the
    yield condition this is the closest-point projection in the energy norm."""
    r, e, _, dep, _, _, sp, _ = _principal(uniform)
    active = {1: ((0, 2),), 2: ((0, 2), (1, 2)), 3: ((0, 2), (0, 1)),
              4: ((0, 2), (1, 2), (0, 1), (2, 0), (2, 1), (1, 0))}
    worst = 0.0
    for k in np.flatnonzero(r['ind_p']):
        A = np.array([_plane(sp[k], i, j) for i, j in active[int(r['branch'][k])]]).T
        x, res = nnls(A, dep[:, k])
        worst = max(worst, res / np.abs(e[:, k]).max())
        assert (x >= 0).all() and x.max() > 0
    print(worst)
    assert worst <= 1e-13
    assert np.abs(dep[:, ~r['ind_p']]).max() <= 1e-15 * np.abs(e).max()     # elastic points: none


@pytest.mark.parametrize('uniform', [True, False])
def test_tangent_is_symmetric_and_the_derivative_of_the_stress(uniform):
    """ds against central differences of s(e) with step h where all three evaluations share a branch.  The third derivative
    of the eigen-decomposition is of the size (2G + K) / r^2, so the difference quotient is off by (2G + K) (h / r)^2 on top
    of its rounding eps max|s| / h: points with h / r <= 2e-5 are compared, to 1e-8 of 2G + K."""
    e, p, e0, sh, bu, sp, c = points(N, uniform, 21)
    r = _run(uniform)
    n = e.shape[1]
    ds = r['ds'].reshape(3, 3, n)
    scale = 2 * sh + bu
    assert np.abs(ds - ds.transpose(1, 0, 2)).max() <= 4e-16 * scale.max()
    h = 1e-5 * EPS_Y
    same = r['r'] >= h / 2e-5
    fd = np.empty((3, 3, n))
    for j in range(3):
        d = np.zeros((3, 1))
        d[j] = h
        up, dn = (mc_return_map(e + sgn * d, p, sh, bu, sp, c, e0=e0) for sgn in (1, -1))
        fd[:, j] = (up['s'][0:3] - dn['s'][0:3]) / (2 * h)
        same &= (up['branch'] == r['branch']) & (dn['branch'] == r['branch'])
    err = np.abs(fd - ds).max(axis=(0, 1)) / scale
    print(same.mean(), err[same].max(), np.bincount(r['branch'][same], minlength=5))
    assert same.mean() >= 0.8 and (np.bincount(r['branch'][same], minlength=5) >= 0.5 * MIN_SHARE * n).all()
    assert err[same].max() <= 1e-8


@pytest.mark.parametrize('uniform', [True, False])
def test_accepted_plastic_strain_reproduces_the_stress(uniform):
    """Step 7: the same strain with the accepted plastic strain is on the yield surface with the same stress."""
    e, p, e0, sh, bu, sp, c = points(N, uniform, 21)
    r = _run(uniform, accept=True)
    pl = r['ind_p']
    assert np.array_equal(r['ep'][:, ~pl], p[:, ~pl]) and np.abs(r['ep'] - p)[:, pl].min(axis=1).max() > 0
    again = mc_return_map(e, r['ep'], sh, bu, sp, c, e0=e0)
    scale = (np.abs(r['s']).max(axis=0) + c)
    print(relerr_points(again['s'], r['s']), np.abs(again['f'] / scale)[pl].max())
    assert np.abs(again['s'] - r['s']).max(axis=0)[pl].max() <= 1e-12 * scale[pl].max()
    assert (np.abs(again['s'] - r['s']).max(axis=0) <= 1e-12 * scale).all()
    assert np.abs(again['f'] / scale)[pl].max() <= 1e-12


def test_stress_is_continuous_across_every_branch_boundary():
    """Pairs of strains that straddle a boundary, found by bisection between points of different branches: the stresses of
    a pair differ by no more than the elastic stiffness allows for the pair's distance (the projection is a contraction)."""
    e, p, e0, sh, bu, sp, c = points(N, True, 21)
    rng = np.random.default_rng(5)
    lo, hi = e, e[:, rng.permutation(N)]

    def run(x):
        return mc_return_map(x, p, sh, bu, sp, c, e0=e0)
    b_lo, b_hi = run(lo)['branch'], run(hi)['branch']
    for _ in range(70):
        mid = (lo + hi) / 2
        b_mid = run(mid)['branch']
        go = b_mid == b_lo
        lo, hi = np.where(go, mid, lo), np.where(go, hi, mid)
        b_hi = np.where(go, b_hi, b_mid)
    r_lo, r_hi = run(lo), run(hi)
    assert np.array_equal(r_lo['branch'], b_lo) and np.array_equal(r_hi['branch'], b_hi)
    cross = b_lo != b_hi
    found = {tuple(sorted(q)) for q in zip(b_lo[cross].tolist(), b_hi[cross].tolist())}
    print(sorted(found))
    assert {(0, 1), (1, 2), (1, 3), (2, 4), (3, 4)} <= found
    gap = np.abs(hi - lo).max(axis=0)
    jump = np.abs(r_hi['s'] - r_lo['s']).max(axis=0)
    bound = 4 * (2 * sh + bu) * gap + 1e-13 * (np.abs(r_lo['s']).max(axis=0) + c)
    assert (gap[cross] <= 1e-14 * EPS_Y).all()
    print((jump / bound)[cross].max())
    assert (jump <= bound)[cross].all()


def test_apex_is_the_apex_of_the_matched_drucker_prager_cone():
    """newton._footing_setup's plane-strain match: c_dp / eta_dp = c / tan(phi) = c cos(phi) / sin(phi)."""
    eta_dp = 3 * np.tan(PHI) / np.sqrt(9 + 12 * np.tan(PHI) ** 2)
    c_dp = 3 * COHESION / np.sqrt(9 + 12 * np.tan(PHI) ** 2)
    e = EPS_Y * np.array([[3.0, 2.0], [2.5, 3.0], [0.4, -0.7]])
    r = mc_return_map(e, None, P_SHEAR, P_BULK, np.sin(PHI), COHESION, e0=EPS_Y * np.array([0, 0, 0, 2.8]))
    assert (r['branch'] == 4).all() and r['n_apex'] == 2 and r['n_smooth'] == 0
    assert np.abs(r['s'][[0, 1, 3]] - c_dp / eta_dp).max() <= 1e-14 * c_dp / eta_dp
    assert np.abs(r['s'][2]).max() <= 1e-14 * c_dp / eta_dp and not r['ds'].any()


@pytest.mark.parametrize('case', FOOTING)
def test_footing_driver_on_the_restatement_reaches_plastic_branches(case):
    """The footing meets the face, the right edge and the apex (never the left edge: sig1 = sig2 is triaxial compression)."""
    r = cpu_footing(*case)
    print(r['branches'], r['pressure'], r['prandtl_nc'])
    assert len(r['zeta']) == case[2]
    assert abs(r['prandtl_nc'] - 14.83) < 0.005
    met = r['branches'].sum(axis=0)
    assert met[1] > 0 and met[2] + met[3] > 0 and met[4] > 0               # face, an edge, the apex
    if case[2] > 1:                                                         # and one step less does not
        less = r['branches'][:-1].sum(axis=0)
        assert not (less[1] > 0 and less[2] + less[3] > 0 and less[4] > 0)
    assert r['branches'][-1][1:].sum() > 0                                  # the last step is plastic
    assert all(a == (int(b[1:4].sum()), int(b[4])) for a, b in zip(r['counts'], r['branches']))
    assert np.all(np.diff(r['pressure']) > 0)

#!/usr/bin/env python3
"""
Fixtures of the von Mises return map with isotropic hardening on a piecewise-linear curve (the fifth material model) against
its high-precision reference tests/vmi_mp.py: `return_map_mp_vmi.npz`.

    python tests/golden/make_golden_vmi_mp.py            (a few minutes; needs mpmath)

n points in columns, arrays only:
  e (3, n), p (4, n), e0 (4,), with_e0 (n,) bool, G, K, m3, m4 (n,)    the float64 inputs; m3, m4 are a, Y; the rows of p are
                                (p11, p22, gamma12, kappa)
  curve (n,) int8, kappa_c, slope_c (c = 0..3)    the hardening curve of a point.  The curve and the initial strain are one per
                                call of the kernels, so the points come in eight launches, (curve, without / with `e0`), each of
                                more than 256 points and no multiple of 256
  s (4, n), ds (9, n), ep (4, n)  the reference, rounded once to float64 (ds zero where `no_tangent`); ep = the new state rows
  label (n,) int8               0 elastic, 1 + j: plastic, the new kappa in segment j
  no_tangent (n,) bool          a difference point of the tangent, or a float64 neighbour of the strain, carries another label
  overshoot, dist (n,)          crit / Y of the trial state; distance of the new kappa to the nearest breakpoint (vmi_mp.point)
  family (n,) int8              index into FAMILIES = 'ABCDE'

Curves: 0 one flat segment; 1 one linear segment; 2 eight concave saturating segments ending flat (a Voce curve, 450 -> 700,
b = 60); 3 four segments, the second softening.
Families:
  A  the interior of a segment: steel +-40 % per point, a = 0 or up to 20 000, every segment of the curve in turn as the one
     the return ends in, the start in it or in the one before; a quarter of the points elastic
  B  breakpoints (curves 2, 3): starts with kappa exactly on one, and returns that end 2 and 3 ulps of e[0] to either side of one
     (found by bisection on the reference's label)
  C  long steps: one return across at least three segments (curves 2, 3), and starts beyond the last breakpoint
  D  overshoot crit / Y = 1e-12 ... 1e4, log-uniform
  E  pairs one ulp apart in e[0] that straddle the yield surface or (curves 2, 3) a breakpoint
Conditions asserted here, on the reference alone: the sizes of the launches, `no_tangent` nowhere in A and at every point of E,
every family present, every segment of curve 2 the end of at least 20 returns.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vmi_mp                                                           # noqa: E402
from vmi_ref import radius_growth                                       # noqa: E402

FAMILIES = 'ABCDE'
YOUNG, POISSON, SIGMA_Y = 206900.0, 0.29, 450.0                         # tests/vm_cases.py
SHEAR, BULK, YIELD = YOUNG / (2 * (1 + POISSON)), YOUNG / (3 * (1 - 2 * POISSON)), np.sqrt(2 / 3) * SIGMA_Y
PER_LAUNCH = 260
N_B, N_C, N_D, N_PAIRS = 40, 40, 52, 14


def voce(sigma_0, sigma_inf, b, n_seg):
    """The sampling of hardening.voce_curve, restated (the fixture does not depend on the product's host code)."""
    frac = np.arange(n_seg) / (n_seg - 1) * (1 - np.exp(-b * (np.log(100.0) / b)))
    eps = -np.log1p(-frac) / b
    eps[-1] = np.log(100.0) / b
    kappa, R = np.sqrt(1.5) * eps, np.sqrt(2 / 3) * (sigma_inf - sigma_0) * frac
    return kappa, np.append(np.diff(R) / np.diff(kappa), 0.0)


def curves():
    return [(np.zeros(1), np.zeros(1)), (np.zeros(1), np.array([2 * 20000.0 / 3])), voce(450.0, 700.0, 60.0, 8),
            (np.array([0.0, 2e-3, 6e-3, 1.5e-2]), np.array([30000.0, -8000.0, 5000.0, 0.0]))]


def widths(kappa):
    """Length of every segment, the last (infinite) one counted as long as the curve before it (0.02 for a single segment)."""
    return np.append(np.diff(kappa), kappa[-1] if kappa.size > 1 else 0.02)


def materials(rng):
    f = rng.uniform(0.6, 1.4)
    return SHEAR * f, BULK * rng.uniform(0.6, 1.4), (0.0 if rng.random() < 0.4 else 10000.0 * rng.uniform(0, 2)), \
        YIELD * rng.uniform(0.6, 1.4)


def strain_for(rng, mats, z, k0, nrm):
    """(e (3,), p (4,)) whose relative trial stress has the norm `nrm` (up to rounding) in a random direction."""
    G, K, a, Y = mats
    p = np.append(rng.normal(0, 1e-3, 3), k0)
    pt = np.array([p[0], p[1], p[2] / 2, -(p[0] + p[1])])
    d = rng.normal(0, 1, 4)
    d[[0, 1, 3]] -= d[[0, 1, 3]].mean()
    d /= np.sqrt(d[0] ** 2 + d[1] ** 2 + 2 * d[2] ** 2 + d[3] ** 2)
    dev = (nrm * d + a * pt) / (2 * G)
    v = 3 * (z[3] - pt[3] - dev[3])                                     # the trace that the prescribed component 33 asks for
    Et = np.array([dev[0] + v / 3, dev[1] + v / 3, 2 * dev[2]])
    return Et - z[:3] + p[:3], p


def landing(mats, curve, k0, k_new):
    """The norm of the relative trial stress whose return from k0 ends at k_new."""
    G, K, a, Y = mats
    return Y + radius_growth(*curve, k_new) + (2 * G + a) * (k_new - k0)


def straddle(e, p, z, mats, curve, labels):
    """Two values of e[0] one ulp apart, the reference's label in labels[0] at the first and in labels[1] at the second (None
    when e[0] * (1 -+ 1e-6 ... 1e-2) does not bracket the change)."""
    mc = vmi_mp.Curve(*curve)
    lab = lambda x: vmi_mp.label_of((x, e[1], e[2]), p, z, *mats, mc)                    # noqa: E731
    side = lambda x: 0 if lab(x) in labels[0] else (1 if lab(x) in labels[1] else None)    # noqa: E731
    for rel in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2):
        lo, hi = e[0] * (1 - rel), e[0] * (1 + rel)
        s_lo, s_hi = side(lo), side(hi)
        if s_lo is not None and s_hi is not None and s_lo != s_hi:
            break
    else:
        return None
    while True:
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            break
        s = side(mid)
        if s is None:
            return None
        lo, hi = (mid, hi) if s == s_lo else (lo, mid)
    return (lo, hi) if s_lo == 0 else (hi, lo)


def launch(c, curve, with_e0, z, rng):
    """The points of one launch -> list of (e, p, mats, family)."""
    kappa, slope = curve
    n_seg, w = kappa.size, widths(kappa)
    rows = []
    multi = n_seg > 1
    n_A = PER_LAUNCH - (N_B if multi else 0) - N_C - N_D - 2 * N_PAIRS

    def interior(j, lo=0.1, hi=0.9):
        return kappa[j] + w[j] * rng.uniform(lo, hi)

    for i in range(n_A):                                               # A
        mats, j = materials(rng), i % n_seg
        k_new = interior(j)
        if i % 4 == 3:
            k0 = k_new
            nrm = rng.uniform(0.3, 0.95) * (mats[3] + radius_growth(*curve, k0))
        else:
            k0 = kappa[j] + (k_new - kappa[j]) * rng.uniform(0.05, 0.8) if (j == 0 or i % 2) else interior(j - 1)
            nrm = landing(mats, curve, k0, k_new)
        rows.append((*strain_for(rng, mats, z, k0, nrm), mats, 'A'))
    n_pairs_bp = N_PAIRS // 2 if multi else 0
    if multi:                                                          # B
        for i in range(N_B // 2):
            mats, j = materials(rng), 1 + i % (n_seg - 1)
            rows.append((*strain_for(rng, mats, z, kappa[j], landing(mats, curve, kappa[j], interior(j + i % 2 if j + 1 < n_seg else j))),
                         mats, 'B'))
        done = 0
        while done < N_B // 8:
            mats, j = materials(rng), 1 + done % (n_seg - 1)
            k0 = interior(j - 1, 0.1, 0.5)
            e, p = strain_for(rng, mats, z, k0, landing(mats, curve, k0, kappa[j]))
            pair = straddle(e, p, z, mats, curve, ((j,), (j + 1,)))
            if pair is None:
                continue
            for x, to in zip(pair, (-np.inf, np.inf) if pair[0] < pair[1] else (np.inf, -np.inf)):
                for ulps in (2, 3):
                    y = x
                    for _ in range(ulps):
                        y = np.nextafter(y, to)
                    rows.append((np.array([y, e[1], e[2]]), p, mats, 'B'))
            done += 1
    for i in range(N_C):                                               # C
        mats = materials(rng)
        if multi and i % 2 == 0:
            j = rng.integers(0, n_seg - 3)
            k0, k_new = interior(j), interior(rng.integers(j + 3, n_seg))
        else:
            k0 = kappa[-1] * rng.uniform(1.2, 5) if multi else rng.uniform(0.01, 0.5)
            k_new = k0 * rng.uniform(1.05, 3)
        rows.append((*strain_for(rng, mats, z, k0, landing(mats, curve, k0, k_new)), mats, 'C'))
    for i in range(N_D):                                               # D
        mats = materials(rng)
        k0 = rng.uniform(0, 1.5) * (kappa[-1] if multi else 0.02)
        over = 10.0 ** (-12 + 16 * (i + rng.random()) / N_D)
        rows.append((*strain_for(rng, mats, z, k0, mats[3] + radius_growth(*curve, k0) + over * mats[3]), mats, 'D'))
    done = 0
    while done < N_PAIRS:                                              # E
        mats = materials(rng)
        if done < n_pairs_bp:
            j = 1 + done % (n_seg - 1)
            k0 = interior(j - 1, 0.1, 0.5)
            e, p = strain_for(rng, mats, z, k0, landing(mats, curve, k0, kappa[j]))
            labels = ((j,), (j + 1,))
        else:
            k0 = rng.uniform(0, 1.2) * (kappa[-1] if multi else 0.02)
            e, p = strain_for(rng, mats, z, k0, mats[3] + radius_growth(*curve, k0))
            labels = ((0,), tuple(range(1, n_seg + 1)))
        pair = straddle(e, p, z, mats, curve, labels)
        if pair is None:
            continue
        for x in pair:
            rows.append((np.array([x, e[1], e[2]]), p, mats, 'E'))
        done += 1
    assert len(rows) == PER_LAUNCH, len(rows)
    return rows


def inputs():
    rng = np.random.default_rng(20260105)
    e0 = rng.normal(0, 1e-3, 4)
    cs = curves()
    cols = {k: [] for k in ('e', 'p', 'G', 'K', 'm3', 'm4', 'family', 'curve', 'with_e0')}
    for c, curve in enumerate(cs):
        for with_e0 in (False, True):
            for e, p, mats, fam in launch(c, curve, with_e0, e0 if with_e0 else np.zeros(4), rng):
                cols['e'].append(e); cols['p'].append(p)
                for k, v in zip(('G', 'K', 'm3', 'm4'), mats):
                    cols[k].append(v)
                cols['family'].append(FAMILIES.index(fam)); cols['curve'].append(c); cols['with_e0'].append(with_e0)
    inp = {'e': np.array(cols['e']).T.copy(), 'p': np.array(cols['p']).T.copy(), 'e0': e0,
           'with_e0': np.array(cols['with_e0'], dtype=bool), 'family': np.array(cols['family'], dtype=np.int8),
           'curve': np.array(cols['curve'], dtype=np.int8), **{k: np.array(cols[k], dtype=float) for k in ('G', 'K', 'm3', 'm4')}}
    for c, (kappa, slope) in enumerate(cs):
        inp[f'kappa_{c}'], inp[f'slope_{c}'] = kappa, slope
    return inp


def outputs(inp, idx=None):
    """The reference at the points `idx` (all of them by default) of the inputs."""
    idx = np.arange(inp['G'].size) if idx is None else np.asarray(idx)
    out = None
    for c in np.unique(inp['curve'][idx]):
        at = np.flatnonzero(inp['curve'][idx] == c)
        sub = idx[at]
        z = inp['e0'].reshape(4, 1) * inp['with_e0'][sub]
        r = vmi_mp.reference(inp['e'][:, sub], inp['p'][:, sub], z, *(inp[k][sub] for k in ('G', 'K', 'm3', 'm4')),
                             inp[f'kappa_{c}'], inp[f'slope_{c}'])
        if out is None:
            out = {k: np.zeros(v.shape[:-1] + (idx.size,), dtype=v.dtype) for k, v in r.items()}
        for k, v in r.items():
            out[k][..., at] = v
    return out


def check_conditions(fix):
    fam, nt, lab = fix['family'], fix['no_tangent'], fix['label']
    for c in range(4):
        for with_e0 in (False, True):
            n = int(((fix['curve'] == c) & (fix['with_e0'] == with_e0)).sum())
            assert n > 256 and n % 256 != 0, (c, with_e0, n)
    for f in FAMILIES:
        assert (fam == FAMILIES.index(f)).any(), f
    assert not nt[fam == FAMILIES.index('A')].any()
    sel = fam == FAMILIES.index('A')
    assert (lab[sel] == 0).any() and (lab[sel] > 0).any()
    for f in 'BCD':
        assert (lab[fam == FAMILIES.index(f)] > 0).all(), f
    sel = fam == FAMILIES.index('E')
    pairs = lab[sel].reshape(-1, 2)
    assert nt[sel].all() and (pairs[:, 0] != pairs[:, 1]).all()
    ends = np.bincount(lab[(fix['curve'] == 2) & (lab > 0)] - 1, minlength=8)
    assert (ends >= 20).all(), ends
    # one return of family C crosses at least three segments
    sel = np.flatnonzero((fam == FAMILIES.index('C')) & (fix['curve'] >= 2))
    start = np.array([np.searchsorted(fix[f'kappa_{fix["curve"][k]}'], fix['p'][3, k], side='right') - 1 for k in sel])
    assert ((lab[sel] - 1 - start) >= 3).sum() >= 20


def path():
    return os.path.join(HERE, 'return_map_mp_vmi.npz')


def main():
    inp = inputs()
    fix = dict(inp, **outputs(inp))
    check_conditions(fix)
    np.savez_compressed(path(), **fix)
    print(fix['G'].size, 'points,', os.path.getsize(path()), 'bytes; per family', np.bincount(fix['family'], minlength=5),
          'labels', np.bincount(fix['label']))


if __name__ == '__main__':
    main()

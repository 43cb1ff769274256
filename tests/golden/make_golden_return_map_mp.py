#!/usr/bin/env python3
"""
Fixtures of the three return maps against the high-precision reference tests/return_map_mp.py:
`return_map_mp_mc.npz`, `return_map_mp_vm.npz`, `return_map_mp_dp.npz`.

    python tests/golden/make_golden_return_map_mp.py            (a few minutes; needs mpmath)

Per file, n points in columns:
  e (3, n), p (4, n), e0 (4,), with_e0 (n,) bool, G, K, m3, m4 (n,)    the float64 inputs; m3, m4 are sin_phi, c (Mohr-Coulomb),
                                a, Y (von Mises), eta, c (Drucker-Prager).  The initial strain is one vector per call of the
                                kernels, so the points come in two groups, without it and with `e0`, each of more than 256
                                points and no multiple of 256.
  s (4, n), ds (9, n), ep (4, n)  the reference, rounded once to float64 (ds zero where `no_tangent`)
  label (n,) int8               return_map_mp.LABELS[model]
  no_tangent (n,) bool          a difference point of the tangent, or a float64 neighbour of the strain (one ulp in one
                                component), carries another label than the point
  r_rel, dist (n,)              the conditioning (return_map_mp)
  family (n,) int8              index into FAMILIES = 'ABCDE';  names_C: the names of family C's points in their order

Families (Mohr-Coulomb; the other two models have A, C, D, E):
  A  generic: the footing's material (E = 1e7, nu = 0.48, phi = pi/9, c = 450), a quarter each without p and e0, with p, with
     e0, with both; the floors of tests/mc_cases.py kept twice over (on tests/mc_ref.py), every branch >= MIN_SHARE
  B  nearly isotropic in-plane strain: r / max|Et| = 1e-3, 1e-6, 1e-9, 1e-12 at nu = 0.2 and 0.48; elastic, both edges, apex
     in equal parts (a face point does not keep DIST_FLOOR there: e1 - e2 or e2 - e3 is r-sized)
  C  exact ties and special values, by name
  D  wide parameters: G 1e2..1e9, nu up to 0.499, sin(phi) 0.01..0.99, c 1e-2..1e5, strains around each point's yield strain
  E  pairs of points one ulp apart in e[0] that straddle a branch boundary, found by bisection on the reference
Conditions asserted here, on the reference alone: `no_tangent` nowhere in A, B, D; in C exactly at NO_TANGENT_C[model]; at
every point of E.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import return_map_mp as rmp                                            # noqa: E402
from mc_ref import mc_return_map                                        # noqa: E402
from vm_ref import vm_return_map                                        # noqa: E402

FAMILIES = 'ABCDE'
R_FLOOR, DIST_FLOOR, MIN_SHARE = 1e-2, 1e-6, 0.02                       # tests/mc_cases.py
YOUNG, COHESION, PHI = 1e7, 450.0, np.pi / 9                           # the strip footing
SIN_PHI = float(np.sin(PHI))
VM_YOUNG, VM_POISSON, VM_SIGMA_Y = 206900.0, 0.29, 450.0               # tests/vm_cases.py
DECADES = tuple(range(-7, 8))
# family C's points that sit on a branch boundary exactly, per model (none: every tie below lies inside its branch)
NO_TANGENT_C = {'mc': (), 'vm': (), 'dp': ()}
N_PAIRS = 15                                                            # per boundary of family E


def lame(young, poisson):
    return young / (2 * (1 + poisson)), young / (3 * (1 - 2 * poisson))


class Cols:
    """Points collected column by column."""

    def __init__(self):
        self.rows = []
        self.names = []

    def add(self, family, e, p, with_e0, G, K, m3, m4, name=None):
        e, p = np.asarray(e, dtype=float), np.asarray(p, dtype=float)
        n = e.shape[1] if e.ndim == 2 else 1
        one = np.ones(n)
        self.rows.append(dict(e=e.reshape(3, n), p=(p.reshape(4, n) if p.size > 1 else np.zeros((4, n))),
                              with_e0=np.full(n, bool(with_e0)), G=G * one, K=K * one, m3=m3 * one, m4=m4 * one,
                              family=np.full(n, FAMILIES.index(family), dtype=np.int8)))
        if family == 'C':
            self.names.append(name)

    def arrays(self, e0):
        out = {k: np.concatenate([r[k] for r in self.rows], axis=-1) for k in self.rows[0]}
        order = np.argsort(out['with_e0'], kind='stable')              # the group without e0 first
        out = {k: np.ascontiguousarray(v[..., order]) for k, v in out.items()}
        out['e0'] = np.asarray(e0, dtype=float)
        out['names_C'] = np.array(self.names)
        return out


def traceless(p):
    p[3] = -(p[0] + p[1])
    return p


def rotate(pa, pb, ang):
    q, m = (pa - pb) / 2, (pa + pb) / 2
    return np.array([m + q * np.cos(ang), m - q * np.cos(ang), 2 * q * np.sin(ang)])


def pick(labels, ok, quota, n_labels, n):
    """Indices of n points among those `ok`: `quota` of every label first (as far as there are), then in their order."""
    idx = []
    for l in range(n_labels):
        idx += list(np.flatnonzero(ok & (labels == l))[:quota])
    rest = [k for k in np.flatnonzero(ok) if k not in set(idx)]
    idx = (idx + rest)[:n]
    assert len(idx) == n, (len(idx), n)
    return np.sort(np.array(idx))


# ---------------------------------------------------------------------------------------
# Mohr-Coulomb
# ---------------------------------------------------------------------------------------
def _mc_ok(e, p, e0, G, K, s, c):
    r = mc_return_map(e, p, G, K, s, c, e0=e0)
    return r['branch'], (r['r_rel'] >= 2 * R_FLOOR) & (r['dist'] >= 2 * DIST_FLOOR)


def mc_inputs(n_pairs=N_PAIRS):
    cols = Cols()
    G48, K48 = lame(YOUNG, 0.48)
    G20, K20 = lame(YOUNG, 0.2)
    ey = {0.48: COHESION / (2 * G48), 0.2: COHESION / (2 * G20)}
    mats = {0.48: (G48, K48), 0.2: (G20, K20)}
    e0 = ey[0.48] * np.array([-0.30, -0.28, 0.02, -0.31])              # a nearly hydrostatic in-situ state
    # A: the volume change decides nearly alone at nu = 0.48 (lam = 24 G), so the trace is drawn a tenth of the deviator
    rng = np.random.default_rng(4801)
    for with_p in (False, True):
        for with_e0 in (False, True):
            m = 6000
            dev = ey[0.48] * rng.normal(0, 3.0, size=(2, m))
            tr = ey[0.48] * rng.normal(0.1, 0.3, size=m)
            e = rotate(tr / 2 + dev[0] / 2, tr / 2 - dev[0] / 2, rng.uniform(0, 2 * np.pi, m))
            p = ey[0.48] * rng.normal(0, 1.5, size=(4, m)) * with_p
            p[[0, 1, 3]] -= (p[0] + p[1] + p[3]) / 3 * rng.uniform(0.8, 1.0, m)
            z = e0.reshape(4, 1) if with_e0 else None
            lab, ok = _mc_ok(e, p, z, G48, K48, SIN_PHI, COHESION)
            k = pick(lab, ok, 15, 5, 75)
            cols.add('A', e[:, k], p[:, k], with_e0, G48, K48, SIN_PHI, COHESION)
    # B: Et = (m + r cos, m - r cos, 2 r sin, ez); e = Et - e0 + p in float64 moves Et by roundings far below r
    rng = np.random.default_rng(4802)
    for nu in (0.2, 0.48):
        G, K = mats[nu]
        for r_rel in (1e-3, 1e-6, 1e-9, 1e-12):
            for with_e0 in (False, True):
                m = 4000
                spread = 3.0 if nu == 0.2 else 0.4
                mean = ey[nu] * rng.normal(0, spread, m)
                ez = mean + ey[nu] * rng.normal(0, 3.0, m) * (rng.uniform(size=m) < 0.8)
                big = np.maximum(np.abs(mean), np.abs(ez))
                ang = rng.uniform(0, 2 * np.pi, m)
                Et = np.array([mean + r_rel * big * np.cos(ang), mean - r_rel * big * np.cos(ang),
                               2 * r_rel * big * np.sin(ang), ez])
                p = traceless(ey[nu] * rng.normal(0, 0.2, size=(4, m))) * (rng.uniform(size=m) < 0.5)
                z = e0.reshape(4, 1) * with_e0
                e = (Et + p - z)[0:3]
                p[3] = -(Et[3] - z[3])                                     # the out-of-plane strain is e0[3] - p[3]
                r = mc_return_map(e, p, G, K, SIN_PHI, COHESION, e0=z)
                ok = (r['dist'] >= 2 * DIST_FLOOR) & (r['branch'] != 1) & (r['r_rel'] < 3 * r_rel) & (r['r_rel'] > r_rel / 3)
                k = pick(np.searchsorted([0, 2, 3, 4], r['branch']), ok, 4, 4, 16)
                assert min(np.bincount(r['branch'][k], minlength=5)[[0, 2, 3, 4]]) >= 3
                cols.add('B', e[:, k], p[:, k], with_e0, G, K, SIN_PHI, COHESION)
    # C
    for nu in (0.2, 0.48):
        G, K = mats[nu]
        y = ey[nu]
        tag = f' nu={nu}'
        special = [('zero strain', (0.0, 0.0, 0.0))]
        special += [(f'r = 0, compression x{f}', (-f * y, -f * y, 0.0)) for f in (0.5, 2.0, 50.0)]
        special += [(f'r = 0, tension x{f}', (f * y, f * y, 0.0)) for f in (0.5, 2.0, 10.0, 100.0)]
        special += [(f'uniaxial tension x{f}', (f * y, 0.0, 0.0)) for f in (0.5, 2.0, 5.0, 40.0)]
        special += [(f'uniaxial compression x{f}', (-f * y, 0.0, 0.0)) for f in (0.5, 2.0, 5.0, 40.0)]
        special += [(f'uniaxial tension in 22 x{f}', (0.0, f * y, 0.0)) for f in (2.0, 5.0)]
        special += [(f'pure shear x{f}', (0.0, 0.0, f * y)) for f in (0.5, 2.0, 6.0, 60.0)]
        special += [('denormal products 1e-300', (1e-300, -1e-300, 1e-300)), ('denormal products 1e-170', (3e-170, 1e-170, -2e-170)),
                    ('denormal products 1e-160', (-1.5e-160, 0.5e-160, 1e-160)), ('denormal strain', (3e-310, -1e-310, 2e-310))]
        for name, e in special:
            cols.add('C', np.array(e).reshape(3, 1), 0.0, False, G, K, SIN_PHI, COHESION, name + tag)
        for d in DECADES:                                            # the law is homogeneous of degree one in (strain, c)
            sc = 10.0 ** d
            cols.add('C', (np.array([-1.1, -0.7, 0.2]) * y * sc).reshape(3, 1), 0.0, False, G, K, SIN_PHI, COHESION * sc,
                     f'elastic state x1e{d}' + tag)
            cols.add('C', (np.array([1.3, -0.4, 0.9]) * 3 * y * sc).reshape(3, 1), 0.0, False, G, K, SIN_PHI, COHESION * sc,
                     f'plastic state x1e{d}' + tag)
    # D
    rng = np.random.default_rng(4804)
    m = 8000
    G = 10 ** rng.uniform(2, 9, m)
    nu = rng.uniform(0.0, 0.499, m)
    K = 2 * G * (1 + nu) / (3 * (1 - 2 * nu))
    s = rng.uniform(0.01, 0.99, m)
    c = 10 ** rng.uniform(-2, 5, m)
    scale = c / (2 * G) * 10 ** rng.uniform(-1, 1, m)
    pr = rng.normal(0, 1.0, size=(2, m)) * scale
    e = rotate(pr[0], pr[1], rng.uniform(0, 2 * np.pi, m))
    p = rng.normal(0, 0.3, size=(4, m)) * scale * (rng.uniform(size=m) < 0.7)
    lab, ok = _mc_ok(e, p, None, G, K, s, c)
    k = pick(lab, ok, 40, 5, 200)
    cols.add('D', e[:, k], p[:, k], False, G[k], K[k], s[k], c[k])
    # E: from well-conditioned points at nu = 0.2 (every branch is met in the plane), e[0] moved until the label changes
    rng = np.random.default_rng(4805)
    m = 3000
    pr = ey[0.2] * rng.normal(0, 3.0, size=(2, m))
    e = rotate(pr[0], pr[1], rng.uniform(0, 2 * np.pi, m))
    p = ey[0.2] * rng.normal(0, 0.25, size=(4, m))
    p[[0, 1, 3]] -= (p[0] + p[1] + p[3]) / 3 * rng.uniform(0.8, 1.0, m)
    for la, lb in ((0, 1), (1, 2), (1, 3), (2, 4), (3, 4)):
        _pairs(cols, 'mc', e, p, (G20, K20, SIN_PHI, COHESION), la, lb, n_pairs, ey[0.2],
               lambda x, q: mc_return_map(x, q, G20, K20, SIN_PHI, COHESION)['branch'])
    return cols.arrays(e0)


def _pairs(cols, model, e, p, mats, la, lb, n_pairs, step, labels):
    """n_pairs pairs (x, nextafter(x)) in e[0] with the reference's labels (la, lb) or (lb, la): candidates from the float64
    restatement's labels along e[0], the bisection itself on the reference."""
    found = 0
    lab = labels(e, p)
    for k in np.flatnonzero(lab == la):
        if found == n_pairs:
            break
        for dx in (step * f for f in (0.25, -0.25, 1.0, -1.0, 4.0, -4.0)):
            x = e[:, k:k + 1].copy()
            x[0] += dx
            if labels(x, p[:, k:k + 1])[0] == lb:
                break
        else:
            continue
        zero = np.zeros(4)
        f = lambda v: rmp.label_of(model, (v, e[1, k], e[2, k]), p[:, k], zero, *mats)      # noqa: E731
        lo, hi = float(e[0, k]), float(x[0, 0])
        if f(lo) != la or f(hi) != lb:
            continue
        while np.nextafter(lo, hi) != hi:
            mid = lo + (hi - lo) / 2
            if mid == lo or mid == hi:
                mid = np.nextafter(lo, hi)
            if f(mid) == la:
                lo = mid
            else:
                hi = mid
        if f(hi) != lb:                                              # a third branch lies between the two
            continue
        pair = np.array([[lo, hi], [e[1, k]] * 2, [e[2, k]] * 2])
        cols.add('E', pair, np.repeat(p[:, k:k + 1], 2, axis=1), False, *mats)
        found += 1
    assert found == n_pairs, (la, lb, found)


# ---------------------------------------------------------------------------------------
# von Mises
# ---------------------------------------------------------------------------------------
def vm_inputs(n_pairs=N_PAIRS):
    cols = Cols()
    G, K = lame(VM_YOUNG, VM_POISSON)
    Y = np.sqrt(2 / 3) * VM_SIGMA_Y
    y = Y / (2 * G)
    e0 = y * np.array([0.3, -0.2, 0.25, -0.1])
    hardenings = (0.0, G / 100, 10 * G)
    rng = np.random.default_rng(2901)
    for a in hardenings:
        for with_p in (False, True):
            for with_e0 in (False, True):
                m = 40
                e = rng.normal(0, 1.2 * y, size=(3, m))
                p = traceless(rng.normal(0, 0.3 * y, size=(4, m))) * with_p
                cols.add('A', e, p, with_e0, G, K, a, Y)
    # states where a p dominates 2G dev(eps - p): an in-plane plastic strain of four yield strains at a = 10 G (back stress 20 Y),
    # the strain within a fifth of a yield strain of it.  (At a = G / 100 such a state needs a plastic strain of 400 yield
    # strains, and (e + e0) - p loses the digits of that ratio before the law begins.)
    m = 40
    q, g = rng.normal(0, 4 * y, size=(2, m))
    p = np.array([q, -q, g, 0 * q])
    e = p[0:3] - e0[0:3].reshape(3, 1) + rng.normal(0, 0.2 * y, size=(3, m))
    cols.add('A', e, p, True, G, K, hardenings[2], Y)
    for a in hardenings:
        tag = f' a={a:.3g}'
        special = [('zero strain', (0.0, 0.0, 0.0))]
        special += [(f'volumetric x{f}', (f * y, f * y, 0.0)) for f in (-50.0, 0.5, 50.0)]
        special += [(f'uniaxial x{f}', (f * y, 0.0, 0.0)) for f in (-5.0, 0.5, 5.0)]
        special += [(f'pure deviatoric x{f}', (f * y, -f * y, 0.0)) for f in (0.3, 3.0)]
        special += [(f'pure shear x{f}', (0.0, 0.0, f * y)) for f in (0.5, 6.0)]
        special += [('denormal products 1e-300', (1e-300, -1e-300, 1e-300)), ('denormal products 1e-160', (-1.5e-160, 0.5e-160, 1e-160)),
                    ('denormal strain', (3e-310, -1e-310, 2e-310))]
        for name, e in special:
            cols.add('C', np.array(e).reshape(3, 1), 0.0, False, G, K, a, Y, name + tag)
        for d in DECADES:
            sc = 10.0 ** d
            cols.add('C', (np.array([-0.4, 0.3, 0.2]) * y * sc).reshape(3, 1), 0.0, False, G, K, a, Y * sc, f'elastic state x1e{d}' + tag)
            cols.add('C', (np.array([1.3, -0.4, 0.9]) * 2 * y * sc).reshape(3, 1), 0.0, False, G, K, a, Y * sc, f'plastic state x1e{d}' + tag)
    rng = np.random.default_rng(2904)
    m = 200
    Gd = 10 ** rng.uniform(2, 9, m)
    nu = rng.uniform(0.0, 0.499, m)
    Kd = 2 * Gd * (1 + nu) / (3 * (1 - 2 * nu))
    ad = Gd * 10 ** rng.uniform(-3, 1.5, m) * (rng.uniform(size=m) < 0.8)
    Yd = 10 ** rng.uniform(-2, 5, m)
    scale = Yd / (2 * Gd) * 10 ** rng.uniform(-1, 1, m)
    e = rng.normal(0, 1.0, size=(3, m)) * scale
    p = traceless(rng.normal(0, 0.3, size=(4, m)) * scale)
    cols.add('D', e, p, False, Gd, Kd, ad, Yd)
    rng = np.random.default_rng(2905)
    m = 400
    e = rng.normal(0, 0.9 * y, size=(3, m))
    p = traceless(rng.normal(0, 0.3 * y, size=(4, m)))
    for a in hardenings[:2]:                                            # the one boundary, at two hardening moduli
        _pairs(cols, 'vm', e, p, (G, K, a, Y), 0, 1, n_pairs, y, lambda x, q: vm_return_map(x, q, G, K, a, Y)['ind_p'].astype(int))
    return cols.arrays(e0)


# ---------------------------------------------------------------------------------------
# Drucker-Prager
# ---------------------------------------------------------------------------------------
def _dp_labels(x, q, G, K, eta, c):
    from oracle import fep_oracle as orc
    n = x.shape[1]
    one = np.ones(n)
    r = orc.return_map(x.copy(), q.copy(), G * one, K * one, eta * one, c * one)
    return np.where(r['ind_p'], np.where(np.abs(r['ds']).max(axis=0) > 0, 1, 2), 0)


def dp_inputs(n_pairs=N_PAIRS):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    cols = Cols()
    G, K = lame(YOUNG, 0.48)
    t = np.tan(PHI)
    eta, c = 3 * t / np.sqrt(9 + 12 * t * t), 3 * COHESION / np.sqrt(9 + 12 * t * t)
    e0 = np.array([-1e-5, -0.9e-5, 0.1e-5, -1.1e-5])
    rng = np.random.default_rng(4811)
    for with_p in (False, True):
        for with_e0 in (False, True):
            m = 140
            e = rng.normal(0, 3e-4, size=(3, m))
            e[0:2] += rng.normal(1e-4, 2e-4, size=(1, m))
            p = rng.normal(0, 2e-5, size=(4, m)) * with_p
            cols.add('A', e, p, with_e0, G, K, eta, c)
    special = [('zero strain', (0.0, 0.0, 0.0)), ('denormal products 1e-300', (1e-300, -1e-300, 1e-300)),
               ('volumetric compression', (-5e-4, -5e-4, 0.0)), ('pure deviatoric', (3e-4, -3e-4, 0.0)), ('pure shear', (0.0, 0.0, 7e-4))]
    for name, e in special:
        cols.add('C', np.array(e).reshape(3, 1), 0.0, False, G, K, eta, c, name)
    for d in DECADES:
        sc = 10.0 ** d
        cols.add('C', (np.array([-1.1, -0.7, 0.2]) * 1e-4 * sc).reshape(3, 1), 0.0, False, G, K, eta, c * sc, f'elastic state x1e{d}')
        cols.add('C', (np.array([1.3, -0.4, 0.9]) * 1e-4 * sc).reshape(3, 1), 0.0, False, G, K, eta, c * sc, f'plastic state x1e{d}')
    rng = np.random.default_rng(4814)                                   # as test_return_map_random_materials_wide_ranges
    m = 200
    Gd = 10 ** rng.uniform(2, 9, m)
    Kd = Gd * 10 ** rng.uniform(-1, 2, m)
    ed = rng.uniform(0.01, 0.9, m)
    cd = 10 ** rng.uniform(-2, 5, m)
    scale = cd / Gd
    e = rng.normal(0, 1, size=(3, m)) * scale * 10 ** rng.uniform(-2, 1.5, m)
    p = rng.normal(0, 0.1, size=(4, m)) * scale
    cols.add('D', e, p, False, Gd, Kd, ed, cd)
    rng = np.random.default_rng(4815)
    m = 400
    e = rng.normal(0, 3e-4, size=(3, m))
    e[0:2] += rng.normal(1e-4, 2e-4, size=(1, m))
    p = rng.normal(0, 2e-5, size=(4, m))
    for la, lb in ((0, 1), (1, 2)):
        _pairs(cols, 'dp', e, p, (G, K, eta, c), la, lb, n_pairs, 1e-4, lambda x, q: _dp_labels(x, q, G, K, eta, c))
    return cols.arrays(e0)


INPUTS = {'mc': mc_inputs, 'vm': vm_inputs, 'dp': dp_inputs}
INPUT_KEYS = ('e', 'p', 'e0', 'with_e0', 'G', 'K', 'm3', 'm4', 'family', 'names_C')
OUTPUT_KEYS = ('s', 'ds', 'ep', 'label', 'no_tangent', 'r_rel', 'dist')


def outputs(model, inp, idx=None):
    """The reference at the points `idx` (all of them by default) of the inputs."""
    idx = np.arange(inp['G'].size) if idx is None else np.asarray(idx)
    z = inp['e0'].reshape(4, 1) * inp['with_e0'][idx]
    return rmp.reference(model, inp['e'][:, idx], inp['p'][:, idx], z, *(inp[k][idx] for k in ('G', 'K', 'm3', 'm4')))


def check_conditions(model, fix):
    fam, nt = fix['family'], fix['no_tangent']
    for f in 'ABD':
        assert not nt[fam == FAMILIES.index(f)].any(), (model, f)
    assert nt[fam == FAMILIES.index('E')].all(), model
    listed = set(NO_TANGENT_C[model])
    got = {str(n) for n, t in zip(fix['names_C'], nt[fam == FAMILIES.index('C')]) if t}
    assert got == listed, (model, got ^ listed)
    for with_e0 in (False, True):
        n = int((fix['with_e0'] == with_e0).sum())
        assert n > 256 and n % 256 != 0, (model, with_e0, n)
    if model == 'mc':
        share = np.bincount(fix['label'][fam == 0], minlength=5) / (fam == 0).sum()
        assert (share >= MIN_SHARE).all(), share


def path(model):
    return os.path.join(HERE, f'return_map_mp_{model}.npz')


def main():
    for model in sys.argv[1:] or list(INPUTS):
        inp = INPUTS[model]()
        fix = dict(inp, **outputs(model, inp))
        check_conditions(model, fix)
        np.savez_compressed(path(model), **fix)
        print(model, fix['G'].size, 'points,', os.path.getsize(path(model)), 'bytes; per family',
              np.bincount(fix['family'], minlength=5), 'labels', np.bincount(fix['label']))


if __name__ == '__main__':
    main()

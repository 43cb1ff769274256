#!/usr/bin/env python3
"""
Fixtures of the plane-stress von Mises return map against its high-precision reference tests/vmps_mp.py:
`return_map_mp_vmps.npz`.

    python tests/golden/make_golden_return_map_mp_vmps.py            (under a minute; needs mpmath)

n points in columns, arrays only:
  e (3, n), p (4, n), e0 (4,), with_e0 (n,) bool, G, K, m3, m4 (n,)    the float64 inputs; m3, m4 are a, Y.  Every p is traceless
                                (p[3] = -(p[0] + p[1])).  The initial strain is one vector per call of the kernels, so the points
                                come in two groups, without it and with `e0`, each of more than 256 points and no multiple of 256.
  s (4, n), ds (9, n), ep (4, n)  the reference, rounded once to float64 (ds zero where `no_tangent`)
  label (n,) int8               0 elastic, 1 plastic
  no_tangent (n,) bool          a difference point of the tangent, or a float64 neighbour of the strain, carries another label
  dist (n,)                     |sqrt(eta^T P eta) / Y - 1| of the trial state
  family (n,) int8              index into FAMILIES = 'ACDEF'

Families:
  A  generic: steel (E = 206 900, nu = 0.29, sigma_y = 450), a = 0, G / 100, 10 G, with and without p, with and without e0,
     strains of 1.5 yield strains
  C  next to the yield surface: sqrt(eta^T P eta) / Y - 1 = 1e-12 ... 1e-3, a decade each, random directions, with p (the new
     plastic strain of a point with p = 0 would be the increment alone, which carries no more digits than the overshoot leaves)
  D  wide: G 1e2..1e9, nu up to 0.499, a up to 30 G or 0, Y 1e-2..1e5, overshoot 1e-2 ... 1e8
  E  pairs of points one ulp apart in e[0] that straddle the yield surface, found by bisection on the reference's label
  F  the degenerate directions, exactly: equibiaxial (hd = h12 = 0: only the cs term of phi is alive and the start of the
     iteration is furthest from the root), hs = 0 (e11 = -e22), pure shear, uniaxial stress; overshoots 1.001, 1.5, 10, 1e3
Conditions asserted here, on the reference alone: `no_tangent` nowhere in A, C, D, F and at every point of E; every family but
E holds plastic points, A and D elastic ones too.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vmps_mp                                                          # noqa: E402
from vmps_ref import elastic_matrix                                     # noqa: E402

FAMILIES = 'ACDEF'
YOUNG, POISSON, SIGMA_Y = 206900.0, 0.29, 450.0                         # tests/vm_cases.py
N_PAIRS = 15
P = np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 6.0]]) / 3


def lame(young, poisson):
    return young / (2 * (1 + poisson)), young / (3 * (1 - 2 * poisson))


def traceless(p):
    p[3] = -(p[0] + p[1])
    return p


class Cols:
    """Points collected column by column."""

    def __init__(self):
        self.rows = []

    def add(self, family, e, p, with_e0, G, K, m3, m4):
        e, p = np.asarray(e, dtype=float), np.asarray(p, dtype=float)
        n = e.shape[1]
        one = np.ones(n)
        self.rows.append(dict(e=e, p=p.reshape(4, n), with_e0=np.full(n, bool(with_e0)), G=G * one, K=K * one, m3=m3 * one,
                              m4=m4 * one, family=np.full(n, FAMILIES.index(family), dtype=np.int8)))

    def arrays(self, e0):
        out = {k: np.concatenate([r[k] for r in self.rows], axis=-1) for k in self.rows[0]}
        order = np.argsort(out['with_e0'], kind='stable')              # the group without e0 first
        out = {k: np.ascontiguousarray(v[..., order]) for k, v in out.items()}
        out['e0'] = np.asarray(e0, dtype=float)
        return out


def at_overshoot(d, over, p, z, G, K, a, Y):
    """The strains e (3, m) whose relative trial stress is along d (3, m) with sqrt(eta^T P eta) = Y (1 + over)."""
    m = d.shape[1]
    e = np.zeros((3, m))
    for k in range(m):
        g, kk, aa, yy = (np.broadcast_to(v, (m,))[k] for v in (G, K, a, Y))
        C = elastic_matrix(g, kk)[1]
        eta = d[:, k] * yy * (1 + np.broadcast_to(over, (m,))[k]) / np.sqrt(d[:, k] @ P @ d[:, k])
        q = p[:, k]
        st = eta + aa * np.array([2 * q[0] + q[1], 2 * q[1] + q[0], q[2] / 2])
        e[:, k] = np.linalg.solve(C, st) + q[0:3] - z[0:3]
    return e


def pairs(cols, e, p, mats, n_pairs, step):
    """n_pairs pairs (x, nextafter(x)) in e[0] with the reference's labels (0, 1) or (1, 0), by bisection on the reference."""
    found = 0
    zero = np.zeros(4)
    for k in range(e.shape[1]):
        if found == n_pairs:
            break
        f = lambda v: vmps_mp.label_of((v, e[1, k], e[2, k]), p[:, k], zero, *mats)      # noqa: E731
        lo = float(e[0, k])
        la = f(lo)
        for dx in (step * f_ for f_ in (0.25, -0.25, 1.0, -1.0, 4.0, -4.0)):
            if f(lo + dx) != la:
                break
        else:
            continue
        hi = lo + dx
        while np.nextafter(lo, hi) != hi:
            mid = lo + (hi - lo) / 2
            if mid == lo or mid == hi:
                mid = np.nextafter(lo, hi)
            if f(mid) == la:
                lo = mid
            else:
                hi = mid
        pair = np.array([[lo, hi], [e[1, k]] * 2, [e[2, k]] * 2])
        cols.add('E', pair, np.repeat(p[:, k:k + 1], 2, axis=1), False, *mats)
        found += 1
    assert found == n_pairs, found


def inputs(n_pairs=N_PAIRS):
    cols = Cols()
    G, K = lame(YOUNG, POISSON)
    Y = np.sqrt(2 / 3) * SIGMA_Y
    y = Y / (2 * G)
    e0 = y * np.array([0.3, -0.2, 0.25, -0.1])
    none = np.zeros(4)
    hardenings = (0.0, G / 100, 10 * G)
    rng = np.random.default_rng(2911)
    for a in hardenings:
        for with_p in (False, True):
            for with_e0 in (False, True):
                m = 30
                e = rng.normal(0, 1.5 * y, size=(3, m))
                p = traceless(rng.normal(0, 0.3 * y, size=(4, m))) * with_p
                cols.add('A', e, p, with_e0, G, K, a, Y)
    rng = np.random.default_rng(2913)
    for a in hardenings:
        for with_e0 in (False, True):
            over = np.repeat(10.0 ** np.arange(-12, -2), 3)
            m = over.size
            p = traceless(rng.normal(0, 0.3 * y, size=(4, m)))
            e = at_overshoot(rng.normal(size=(3, m)), over, p, e0 if with_e0 else none, G, K, a, Y)
            cols.add('C', e, p, with_e0, G, K, a, Y)
    rng = np.random.default_rng(2914)
    m = 100
    Gd = 10 ** rng.uniform(2, 9, m)
    nu = rng.uniform(0.0, 0.499, m)
    Kd = 2 * Gd * (1 + nu) / (3 * (1 - 2 * nu))
    ad = Gd * 10 ** rng.uniform(-3, 1.5, m) * (rng.uniform(size=m) < 0.7)
    Yd = 10 ** rng.uniform(-2, 5, m)
    over = np.where(np.arange(m) % 5 == 0, -rng.uniform(0.05, 0.9, m), 10 ** rng.uniform(-2, 8, m))      # a fifth elastic
    p = traceless(rng.normal(0, 0.3, size=(4, m)) * Yd / (2 * Gd))
    cols.add('D', at_overshoot(rng.normal(size=(3, m)), over, p, none, Gd, Kd, ad, Yd), p, False, Gd, Kd, ad, Yd)
    rng = np.random.default_rng(2915)
    m = 200
    e = rng.normal(0, 0.9 * y, size=(3, m))
    p = traceless(rng.normal(0, 0.3 * y, size=(4, m)))
    for a in hardenings[:2]:
        pairs(cols, e, p, (G, K, a, Y), n_pairs, y)
    # F: directions in the strain itself, so that hd = h12 = 0 or hs = 0 hold bit for bit; p, where there is one, lies along the
    # direction's own plastic flow, so that its back stress is parallel to the trial stress and the overshoot is the named one
    nu_ps = POISSON
    dirs = {'equibiaxial': (1.0, 1.0, 0.0), 'hs = 0': (1.0, -1.0, 0.0), 'pure shear': (0.0, 0.0, 1.0), 'uniaxial': (1.0, -nu_ps, 0.0)}
    pdir = {'equibiaxial': (1.0, 1.0, 0.0, -2.0), 'hs = 0': (1.0, -1.0, 0.0, 0.0), 'pure shear': (0.0, 0.0, 1.0, 0.0),
            'uniaxial': (1.0, -0.5, 0.0, -0.5)}
    for a in hardenings:
        for name, d in dirs.items():
            for with_p in (False, True):
                for over in (1e-3, 0.5, 9.0, 999.0):
                    d3 = np.array(d).reshape(3, 1)
                    p = np.array(pdir[name]).reshape(4, 1) * 0.25 * y * with_p
                    Cd = elastic_matrix(G, K)[1] @ d3[:, 0]
                    ab = a * np.array([2 * p[0, 0] + p[1, 0], 2 * p[1, 0] + p[0, 0], p[2, 0] / 2])     # along C d, by pdir
                    size = (Y * (1 + over) + np.sqrt(ab @ P @ ab)) / np.sqrt(Cd @ P @ Cd)
                    cols.add('F', d3 * size + p[0:3], p, False, G, K, a, Y)
    return cols.arrays(e0)


INPUT_KEYS = ('e', 'p', 'e0', 'with_e0', 'G', 'K', 'm3', 'm4', 'family')
OUTPUT_KEYS = ('s', 'ds', 'ep', 'label', 'no_tangent', 'dist')


def outputs(inp, idx=None):
    """The reference at the points `idx` (all of them by default) of the inputs."""
    idx = np.arange(inp['G'].size) if idx is None else np.asarray(idx)
    z = inp['e0'].reshape(4, 1) * inp['with_e0'][idx]
    return vmps_mp.reference(inp['e'][:, idx], inp['p'][:, idx], z, *(inp[k][idx] for k in ('G', 'K', 'm3', 'm4')))


def check_conditions(fix):
    fam, nt, lab = fix['family'], fix['no_tangent'], fix['label']
    assert np.array_equal(fix['p'][3], -(fix['p'][0] + fix['p'][1]))
    for f in 'ACDF':
        sel = fam == FAMILIES.index(f)
        assert not nt[sel].any(), f
        assert (lab[sel] == 1).any(), f
    for f in 'AD':
        assert (lab[fam == FAMILIES.index(f)] == 0).any(), f
    for f in 'CF':
        assert (lab[fam == FAMILIES.index(f)] == 1).all(), f
    sel = fam == FAMILIES.index('E')
    assert nt[sel].all() and (np.sort(lab[sel].reshape(-1, 2), axis=1) == (0, 1)).all()
    for a_zero in (True, False):
        assert ((fix['m3'] == 0) == a_zero).sum() >= 50
    for with_e0 in (False, True):
        n = int((fix['with_e0'] == with_e0).sum())
        assert n > 256 and n % 256 != 0, (with_e0, n)


def path():
    return os.path.join(HERE, 'return_map_mp_vmps.npz')


def main():
    inp = inputs()
    fix = dict(inp, **outputs(inp))
    check_conditions(fix)
    np.savez_compressed(path(), **fix)
    print(fix['G'].size, 'points,', os.path.getsize(path()), 'bytes; per family', np.bincount(fix['family'], minlength=5),
          'labels', np.bincount(fix['label']))


if __name__ == '__main__':
    main()

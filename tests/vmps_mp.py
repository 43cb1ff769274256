"""High-precision reference of the plane-stress von Mises return map (test infrastructure, CPU only; mpmath at 80 digits).
It shares no formula with the kernel or with tests/vmps_ref.py: it takes the 3-D von Mises law as tests/return_map_mp.py
states it (vm_stress: backward Euler in the new relative stress) and makes the out-of-plane trial strain an unknown,

    find Et3 such that vm_stress((Et0, Et1, Et2, Et3), p, ...)[3] = 0,

by mpmath.findroot to 65 digits.  The map is the kernel's law whenever p is traceless (the 3-D law reads p[3]).

  label     0 elastic, 1 plastic.  The point is plastic exactly when the ELASTIC plane-stress state, Et3 = -lam (Et0 + Et1) /
            (lam + 2G), violates the 3-D yield condition (the stress is then not admissible, and the solution is unique).
  stress    (s11, s22, s12, 0) of the 3-D law at the root.
  tangent   central differences of that stress map in the three in-plane strains, step 1e-25 of the strain scale, the root
            solved anew at every difference point.  As in return_map_mp.point: both difference points of all three directions
            and the six float64 neighbours of the strain (one ulp in one component) must carry the centre's label; otherwise
            `no_tangent` is set and ds is zero.
  ep        p + Et - C^-1 sig with the 3-D compliance at the root, for plastic points; p itself for elastic ones.
  cond      |sqrt(eta^T P eta) - Y| / Y of the elastic plane-stress trial state: the distance to the yield surface."""
import mpmath as mp
import numpy as np

import return_map_mp as rmp
from return_map_mp import STEP, _compliance, _m

ROOT_TOL = mp.mpf(10) ** -65
LABELS = ('elastic', 'plastic')


def _elastic_et3(Et, G, K):
    G, K = _m(G), _m(K)
    lam = K - 2 * G / 3
    return -lam * (Et[0] + Et[1]) / (lam + 2 * G)


def vmps_stress(Et, p, G, K, a, Y):
    """Et: the three in-plane trial strains -> (S (4), label, cond, Et3 at the root)."""
    x0 = _elastic_et3(Et, G, K)
    S, label, cond = rmp.vm_stress([Et[0], Et[1], Et[2], x0], p, G, K, a, Y)
    if label == 0:
        return [S[0], S[1], S[2], mp.mpf(0)], 0, cond, x0
    scale = _m(Y) / (2 * _m(G))
    f = lambda x: rmp.vm_stress([Et[0], Et[1], Et[2], x], p, G, K, a, Y)[0][3] / _m(Y)      # noqa: E731
    x = mp.findroot(f, (x0, x0 + scale * mp.mpf('0.01')), solver='secant', tol=ROOT_TOL, maxsteps=200, verify=False)
    S, label, _ = rmp.vm_stress([Et[0], Et[1], Et[2], x], p, G, K, a, Y)
    if label != 1 or abs(S[3]) > mp.mpf(10) ** -60 * _m(Y):
        raise ArithmeticError('the root of s33 was not found')
    return [S[0], S[1], S[2], mp.mpf(0)], 1, cond, x


def _trial(e, p, e0):
    e, p, e0 = [_m(v) for v in e], [_m(v) for v in p], [_m(v) for v in e0]
    return [e[0] + e0[0] - p[0], e[1] + e0[1] - p[1], e[2] + e0[2] - p[2]], p


def label_of(e, p, e0, G, K, a, Y):
    """The label alone (for bisections): no root is solved."""
    Et, p = _trial(e, p, e0)
    return rmp.vm_stress(Et + [_elastic_et3(Et, G, K)], p, G, K, a, Y)[1]


def point(e, p, e0, G, K, a, Y):
    """One point -> dict of mpf lists s (4), ds (9, row-major 3x3; zeros with no_tangent), ep (4), and label, no_tangent, dist."""
    Et, p = _trial(e, p, e0)
    S, label, cond, x = vmps_stress(Et, p, G, K, a, Y)
    big = max(abs(v) for v in Et)
    h = STEP * (big if big > 0 else _m(Y) / (2 * _m(G)))
    ds = [mp.mpf(0)] * 9
    no_tangent = False
    for j in range(3):
        up, dn = list(Et), list(Et)
        up[j] += h
        dn[j] -= h
        Su, lu, _, _ = vmps_stress(up, p, G, K, a, Y)
        Sd, ld, _, _ = vmps_stress(dn, p, G, K, a, Y)
        if lu != label or ld != label:
            no_tangent = True
            break
        for i in range(3):
            ds[3 * i + j] = (Su[i] - Sd[i]) / (2 * h)
    if not no_tangent:
        ef = [float(v) for v in e]
        for j in range(3):
            for to in (-np.inf, np.inf):
                nb = list(ef)
                nb[j] = float(np.nextafter(ef[j], to))
                if label_of(nb, p, e0, G, K, a, Y) != label:
                    no_tangent = True
    floor = mp.mpf(10) ** -40 * (2 * _m(G) + _m(K))
    ds = [mp.mpf(0) if no_tangent or abs(v) < floor else v for v in ds]
    if label == 0:
        ep = list(p)
    else:
        el = _compliance(S, G, K)
        Et4 = Et + [x]
        ep = [p[i] + Et4[i] - el[i] for i in range(4)]
    return {'s': S, 'ds': ds, 'ep': ep, 'label': label, 'no_tangent': no_tangent, 'dist': cond}


def reference(e, p, e0, G, K, a, Y):
    """Arrays e (3, n), p (4, n), e0 (4, n) per point, parameters (n,) -> dict of float64 arrays s (4, n), ds (9, n), ep (4, n),
    dist (n,), label (n,) int8 and no_tangent (n,) bool, each rounded once from the high-precision value."""
    n = e.shape[1]
    out = {'s': np.zeros((4, n)), 'ds': np.zeros((9, n)), 'ep': np.zeros((4, n)), 'dist': np.zeros(n),
           'label': np.zeros(n, dtype=np.int8), 'no_tangent': np.zeros(n, dtype=bool)}
    for k in range(n):
        r = point(e[:, k], p[:, k], e0[:, k], G[k], K[k], a[k], Y[k])
        for key in ('s', 'ds', 'ep'):
            out[key][:, k] = [float(v) for v in r[key]]
        out['dist'][k] = float(r['dist'])
        out['label'][k], out['no_tangent'][k] = r['label'], r['no_tangent']
    return out

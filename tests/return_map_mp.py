"""High-precision reference of the three return maps (test infrastructure, CPU only; mpmath at 80 digits).  It states each
law as the closest-point projection it is and shares no branch formula with the kernels or with tests/mc_ref.py,
tests/vm_ref.py and the Drucker-Prager oracle:

  stress    The float64 inputs are converted exactly, Et = (e, 0) + e0 - p.
            Mohr-Coulomb: principal values and directions of the 3x3 strain tensor (mpmath.eigsy), trial principal stress
            C e, then the projection in the energy norm of C^-1 onto the six half-spaces
            (1+s) sig_i - (1-s) sig_j <= 2 c cos(phi), i != j: every active set of 0 to 3 planes has its KKT system solved, the
            first (smallest) one that is feasible with non-negative multipliers is taken.  Nothing is sorted.  The label is
            read off the active set: 0 planes elastic, 1 the face, 2 an edge (left when the planes share their minor stress, so
            that the two major ones are equal; right when they share the major one), 3 the apex.
            Von Mises (the law of include/fep.h, which is the radial return for a traceless plastic strain): backward Euler
            in the new relative stress, xi_new (1 + (2G+a) gamma / Y) = xi_trial, |xi_new| = Y.
            Drucker-Prager: projection onto {rho/sqrt2 + eta p <= c, rho >= 0} in the (p, rho) half-plane, by the same
            enumeration of active sets.  The Drucker-Prager kernels have passed against the reference implementation for
            long; this module is anchored on them.
  tangent   central differences of that stress map, step 1e-25 of the strain scale (truncation: (step / r)^2 and below).
            Both difference points of all three directions must carry the centre's label, and so must the six float64
            neighbours of the strain (one ulp in one component); otherwise `no_tangent` is set and ds is zero.
  ep        p + Et - C^-1 sig for plastic points (the Drucker-Prager apex: Et - C^-1 sig, as the reference writes it), p
            itself for elastic ones.
  cond      r_rel = r / max|Et| (r half the distance of the in-plane principal strains); dist = the distance of the multipliers
            to the nearest change of the active set over the multiplier scale, in the units of mc_ref's 'dist' (an active
            multiplier going to zero, an inactive plane's slack over its n.Cn, at the apex the violation of the best edge
            candidate; the scale is the largest trial multiplier or principal strain difference)."""
import functools
import itertools

import mpmath as mp
import numpy as np

mp.mp.dps = 80
STEP = mp.mpf(10) ** -25
TOL = mp.mpf(10) ** -60
LABELS = {'mc': ('elastic', 'smooth', 'left', 'right', 'apex'), 'vm': ('elastic', 'plastic'), 'dp': ('elastic', 'smooth', 'apex')}


def _m(x):
    return mp.mpf(float(x))                                # exact: every float64 is an mpf


def _dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------
# a small convex projection: minimise (x - xt)^T C^-1 (x - xt) / 2  subject to  n_k . x <= b_k
# ---------------------------------------------------------------------------------------
def _inverse(M):
    """Inverse of a 1x1 .. 3x3 Gram matrix (nested lists), None when it is singular to working precision."""
    k = len(M)
    A = mp.matrix(M)
    scale = mp.mpf(1)
    for i in range(k):
        scale *= A[i, i]
    if abs(mp.det(A)) <= mp.mpf(10) ** -40 * abs(scale):
        return None
    return (A ** -1).tolist()


class _Planes:
    """Half-spaces n_k . x <= b_k and the metric C; the inverse Gram matrix of every active set of at most `most` planes."""

    def __init__(self, normals, rhs, C_apply, most):
        self.N, self.b = normals, rhs
        self.CN = [C_apply(n) for n in normals]
        self.den = [_dot(n, cn) for n, cn in zip(self.N, self.CN)]
        self.sets = [()]
        self.inv = {(): None}
        for size in range(1, most + 1):
            for A in itertools.combinations(range(len(normals)), size):
                inv = _inverse([[_dot(self.N[k], self.CN[l]) for l in A] for k in A])
                if inv is not None:
                    self.sets.append(A)
                    self.inv[A] = inv

    def values(self, x):
        return [_dot(n, x) - b for n, b in zip(self.N, self.b)]

    def candidate(self, A, xt, gt):
        """-> (x, mu) of the KKT system of the active set A."""
        if not A:
            return list(xt), []
        mu = [_dot(row, [gt[k] for k in A]) for row in self.inv[A]]
        x = [xt[i] - mp.fsum(m * self.CN[k][i] for m, k in zip(mu, A)) for i in range(len(xt))]
        return x, mu

    def project(self, xt):
        """-> (x, active set, dist): the first active set, by size, that is feasible with non-negative multipliers."""
        gt = self.values(xt)
        big = max([abs(v) for v in xt] + [abs(b) for b in self.b])
        tol_g = TOL * big
        tol_mu = tol_g / min(self.den)
        for A in self.sets:
            x, mu = self.candidate(A, xt, gt)
            if any(m < -tol_mu for m in mu):
                continue
            g = self.values(x)
            if any(v > tol_g for v in g):
                continue
            slack = [-g[k] / self.den[k] for k in range(len(self.N)) if k not in A]
            return x, A, mu, slack, gt
        raise ArithmeticError('no active set is feasible')


# ---------------------------------------------------------------------------------------
# Mohr-Coulomb
# ---------------------------------------------------------------------------------------
PAIRS = [(i, j) for i in range(3) for j in range(3) if i != j]


@functools.lru_cache(maxsize=4096)
def _mc_planes(G, K, s, c):
    G, K, s, c = _m(G), _m(K), _m(s), _m(c)
    lam = K - 2 * G / 3
    normals = []
    for i, j in PAIRS:
        n = [mp.mpf(0)] * 3
        n[i], n[j] = 1 + s, -(1 - s)
        normals.append(n)
    b = 2 * c * mp.sqrt(1 - s * s)
    return _Planes(normals, [b] * 6, lambda n: [2 * G * v + lam * mp.fsum(n) for v in n], 3), lam, G


def _mc_label(A):
    if len(A) < 2:
        return len(A)
    if len(A) == 3:
        return 4
    (i, j), (k, l) = PAIRS[A[0]], PAIRS[A[1]]
    if j == l and i != k:
        return 2                                          # the two major stresses are equal
    if i == k and j != l:
        return 3                                          # the two minor stresses are equal
    raise ArithmeticError(f'two active planes {PAIRS[A[0]]}, {PAIRS[A[1]]} that are no edge')


def mc_stress(Et, p, G, K, s, c, want_cond=False):
    pl, lam, Gm = _mc_planes(float(G), float(K), float(s), float(c))
    T = mp.matrix([[Et[0], Et[2] / 2, 0], [Et[2] / 2, Et[1], 0], [0, 0, Et[3]]])
    ev, Q = mp.eigsy(T)
    e = [ev[i] for i in range(3)]
    tr = mp.fsum(e)
    sigt = [lam * tr + 2 * Gm * v for v in e]
    sig, A, mu, slack, gt = pl.project(sigt)
    S = [mp.fsum(sig[k] * Q[i, k] * Q[j, k] for k in range(3)) for i, j in ((0, 0), (1, 1), (0, 1), (2, 2))]
    label = _mc_label(A)
    if not want_cond:
        return S, label, None
    scale = max([abs(g) / d for g, d in zip(gt, pl.den)] + [abs(e[i] - e[j]) for i, j in PAIRS])
    if label < 4:
        d = min(list(mu) + slack)
    else:
        d = None
        for B in pl.sets:
            if len(B) != 2:
                continue
            x, m2 = pl.candidate(B, sigt, gt)
            if any(m < 0 for m in m2):
                continue
            worst = max(v / dn for v, dn in zip(pl.values(x), pl.den))
            d = worst if d is None else min(d, worst)
        d = mp.mpf(0) if d is None else max(d, mp.mpf(0))
    return S, label, d / scale


# ---------------------------------------------------------------------------------------
# von Mises with linear kinematic hardening (include/fep.h)
# ---------------------------------------------------------------------------------------
def _dev4(Et):
    tr = Et[0] + Et[1] + Et[3]
    return [Et[0] - tr / 3, Et[1] - tr / 3, Et[2] / 2, Et[3] - tr / 3], tr


def _norm4(x):
    return mp.sqrt(x[0] ** 2 + x[1] ** 2 + 2 * x[2] ** 2 + x[3] ** 2)


def vm_stress(Et, p, G, K, a, Y, want_cond=False):
    G, K, a, Y = _m(G), _m(K), _m(a), _m(Y)
    dv, tr = _dev4(Et)
    iota = (1, 1, 0, 1)
    st = [2 * G * dv[i] + K * tr * iota[i] for i in range(4)]
    pt = [p[0], p[1], p[2] / 2, p[3]]
    xi = [2 * G * dv[i] - a * pt[i] for i in range(4)]
    nrm = _norm4(xi)
    cond = (nrm - Y) / Y
    if nrm <= Y:
        return st, 0, abs(cond)
    gamma = (nrm / Y - 1) * Y / (2 * G + a)               # from |xi_new| (1 + (2G+a) gamma / Y) = |xi_trial|
    xi_new = [x / (1 + (2 * G + a) * gamma / Y) for x in xi]
    S = [st[i] - 2 * G * gamma * xi_new[i] / Y for i in range(4)]
    return S, 1, abs(cond)


# ---------------------------------------------------------------------------------------
# Drucker-Prager: projection in the (p, rho) half-plane
# ---------------------------------------------------------------------------------------
def dp_stress(Et, p, G, K, eta, c, want_cond=False):
    G, K, eta, c = _m(G), _m(K), _m(eta), _m(c)
    dv, tr = _dev4(Et)
    nd = _norm4(dv)
    xt = [K * tr, 2 * G * nd]
    pl = _Planes([[eta, 1 / mp.sqrt(2)], [mp.mpf(0), mp.mpf(-1)]], [c, mp.mpf(0)], lambda n: [K * n[0], 2 * G * n[1]], 2)
    x, A, mu, slack, gt = pl.project(xt)
    iota = (1, 1, 0, 1)
    if nd == 0:
        if x[1] != 0:
            raise ArithmeticError('a deviator without a direction')
        S = [x[0] * i for i in iota]
    else:
        S = [x[0] * iota[i] + x[1] * dv[i] / nd for i in range(4)]
    d = min([abs(m) for m in mu] + [abs(v) for v in slack]) / max(abs(gt[0]) / pl.den[0], abs(xt[1]) / pl.den[1])
    return S, len(A), d


STRESS = {'mc': mc_stress, 'vm': vm_stress, 'dp': dp_stress}


def _compliance(S, G, K):
    """C^-1 sig as (11, 22, engineering 12, 33)."""
    G, K = _m(G), _m(K)
    mean = (S[0] + S[1] + S[3]) / 3
    vol = mean / (3 * K)
    return [(S[0] - mean) / (2 * G) + vol, (S[1] - mean) / (2 * G) + vol, S[2] / G, (S[3] - mean) / (2 * G) + vol]


def point(model, e, p, e0, G, K, m3, m4):
    """One point -> dict of mpf lists s (4), ds (9, row-major 3x3; zeros with no_tangent), ep (4), and label, no_tangent,
    r_rel, dist."""
    f = STRESS[model]
    e, p, e0 = [_m(v) for v in e], [_m(v) for v in p], [_m(v) for v in e0]
    Et = [e[0] + e0[0] - p[0], e[1] + e0[1] - p[1], e[2] + e0[2] - p[2], e0[3] - p[3]]
    S, label, dist = f(Et, p, G, K, m3, m4, want_cond=True)
    big = max(abs(v) for v in Et)
    yield_strain = _m(m4) / (2 * _m(G))
    h = STEP * (big if big > 0 else yield_strain)
    ds = [mp.mpf(0)] * 9
    no_tangent = False
    for j in range(3):
        up, dn = list(Et), list(Et)
        up[j] += h
        dn[j] -= h
        Su, lu, _ = f(up, p, G, K, m3, m4)
        Sd, ld, _ = f(dn, p, G, K, m3, m4)
        if lu != label or ld != label:
            no_tangent = True
            break
        for i in range(3):
            ds[3 * i + j] = (Su[i] - Sd[i]) / (2 * h)
    if not no_tangent:                                    # a float64 neighbour of the strain on another branch
        ef = [float(v) for v in e]
        for j in range(3):
            for to in (-np.inf, np.inf):
                nb = list(ef)
                nb[j] = float(np.nextafter(ef[j], to))
                if label_of(model, nb, p, e0, G, K, m3, m4) != label:
                    no_tangent = True
    floor = mp.mpf(10) ** -40 * (2 * _m(G) + _m(K))         # the differences' own noise is 1e-55 of the moduli: an exact zero stays one
    ds = [mp.mpf(0) if no_tangent or abs(v) < floor else v for v in ds]
    if label == 0:
        ep = list(p)
    else:
        el = _compliance(S, G, K)
        apex_dp = model == 'dp' and label == 2
        ep = [(0 if apex_dp else p[i]) + Et[i] - el[i] for i in range(4)]
    r = mp.sqrt(((Et[0] - Et[1]) / 2) ** 2 + (Et[2] / 2) ** 2)
    return {'s': S, 'ds': ds, 'ep': ep, 'label': label, 'no_tangent': no_tangent, 'r_rel': r / big if big > 0 else mp.mpf(1),
            'dist': dist}


def label_of(model, e, p, e0, G, K, m3, m4):
    """The label alone (for bisections)."""
    e, p, e0 = [_m(v) for v in e], [_m(v) for v in p], [_m(v) for v in e0]
    Et = [e[0] + e0[0] - p[0], e[1] + e0[1] - p[1], e[2] + e0[2] - p[2], e0[3] - p[3]]
    return STRESS[model](Et, p, G, K, m3, m4)[1]


def reference(model, e, p, e0, G, K, m3, m4):
    """Arrays e (3, n), p (4, n), e0 (4, n) per point, parameters (n,) -> dict of float64 arrays s (4, n), ds (9, n), ep (4, n),
    r_rel, dist (n,), label (n,) int8 and no_tangent (n,) bool, each rounded once from the high-precision value."""
    n = e.shape[1]
    out = {'s': np.zeros((4, n)), 'ds': np.zeros((9, n)), 'ep': np.zeros((4, n)), 'r_rel': np.zeros(n), 'dist': np.zeros(n),
           'label': np.zeros(n, dtype=np.int8), 'no_tangent': np.zeros(n, dtype=bool)}
    for k in range(n):
        r = point(model, e[:, k], p[:, k], e0[:, k], G[k], K[k], m3[k], m4[k])
        for key in ('s', 'ds', 'ep'):
            out[key][:, k] = [float(v) for v in r[key]]
        out['r_rel'][k], out['dist'][k] = float(r['r_rel']), float(r['dist'])
        out['label'][k], out['no_tangent'][k] = r['label'], r['no_tangent']
    return out

"""High-precision reference of the fifth material model (test infrastructure, CPU only; mpmath at 80 digits), in the manner of
tests/return_map_mp.py.  It shares no formula with the kernel or with tests/vmi_ref.py beyond the definition of the law:

  curve     R(k) by plain interpolation of the exact polygon through (kappa[j], sum of slope * length), the last segment
            extended, the first one extended to the left; no table of rounded R, no start segment.
  stress    backward Euler in the new relative stress: xi_new = xi_trial * r / |xi_trial| on the grown surface
            r = Y + R(k0 + lam), the multiplier lam being the root of the monotone scalar residual
            g(lam) = |xi_trial| - (2G + a) lam - (Y + R(k0 + lam)),
            bracketed by g(0) > 0 and g(0) / min(2G + a + slope) and bisected to 1e-70 of the bracket: no walk over segments.
  tangent   central differences of that stress map, step 1e-25 of the strain scale.  Both difference points of all three
            directions must carry the centre's label (0 elastic, 1 + the segment the new kappa lies in), and so must the six
            float64 neighbours of the strain; otherwise `no_tangent` is set and ds is zero.
  ep        rows 0..2 of p + Et - C^-1 sig, and kappa = k0 + the norm of that increment (tensor norm: half the engineering
            shear, twice); p and k0 themselves for an elastic point.
  cond      overshoot = g(0) / Y;  dist = the distance of the new kappa to the nearest breakpoint over max(kappa_new, the
            first breakpoint's scale), 1 for a curve of one segment."""
import mpmath as mp
import numpy as np

mp.mp.dps = 80
STEP = mp.mpf(10) ** -25
TOL = mp.mpf(10) ** -70


def _m(x):
    return mp.mpf(float(x))                                # exact: every float64 is an mpf


class Curve:
    def __init__(self, kappa, slope):
        self.k = [_m(v) for v in kappa]
        self.h = [_m(v) for v in slope]
        self.R = [mp.mpf(0)]
        for j in range(1, len(self.k)):
            self.R.append(self.R[-1] + self.h[j - 1] * (self.k[j] - self.k[j - 1]))

    def segment(self, k):
        """The segment whose half-open interval [kappa[j], kappa[j+1]) holds k (0 to the left of the curve)."""
        j = 0
        while j + 1 < len(self.k) and self.k[j + 1] <= k:
            j += 1
        return j

    def radius_growth(self, k):
        j = self.segment(k)
        return self.R[j] + self.h[j] * (k - self.k[j])


def _dev4(Et):
    tr = Et[0] + Et[1] + Et[3]
    return [Et[0] - tr / 3, Et[1] - tr / 3, Et[2] / 2, Et[3] - tr / 3], tr


def _norm4(x):
    return mp.sqrt(x[0] ** 2 + x[1] ** 2 + 2 * x[2] ** 2 + x[3] ** 2)


def vmi_stress(Et, p4, k0, G, K, a, Y, curve):
    """Et, p4 (the full plastic strain, p33 included, engineering shear) -> (stress, label, lam, overshoot)."""
    G, K, a, Y = _m(G), _m(K), _m(a), _m(Y)
    dv, tr = _dev4(Et)
    iota = (1, 1, 0, 1)
    st = [2 * G * dv[i] + K * tr * iota[i] for i in range(4)]
    pt = [p4[0], p4[1], p4[2] / 2, p4[3]]
    xi = [2 * G * dv[i] - a * pt[i] for i in range(4)]
    nrm = _norm4(xi)
    H0 = 2 * G + a

    def g(lam):
        return nrm - H0 * lam - (Y + curve.radius_growth(k0 + lam))

    g0 = g(mp.mpf(0))
    if g0 <= 0:
        return st, 0, mp.mpf(0), g0 / Y
    lo, hi = mp.mpf(0), g0 / (H0 + min(curve.h))           # g' <= -(2G + a + min slope) < 0
    width = hi
    while hi - lo > TOL * width:
        mid = (lo + hi) / 2
        if g(mid) > 0:
            lo = mid
        else:
            hi = mid
    lam = (lo + hi) / 2
    r = Y + curve.radius_growth(k0 + lam)
    xi_new = [x * r / nrm for x in xi]
    S = [st[i] - 2 * G * lam * xi_new[i] / r for i in range(4)]
    return S, 1 + curve.segment(k0 + lam), lam, g0 / Y


def _compliance(S, G, K):
    """C^-1 sig as (11, 22, engineering 12, 33)."""
    G, K = _m(G), _m(K)
    mean = (S[0] + S[1] + S[3]) / 3
    vol = mean / (3 * K)
    return [(S[0] - mean) / (2 * G) + vol, (S[1] - mean) / (2 * G) + vol, S[2] / G, (S[3] - mean) / (2 * G) + vol]


def _trial(e, p, e0):
    e, p, e0 = [_m(v) for v in e], [_m(v) for v in p], [_m(v) for v in e0]
    p4 = [p[0], p[1], p[2], -(p[0] + p[1])]
    Et = [e[0] + e0[0] - p4[0], e[1] + e0[1] - p4[1], e[2] + e0[2] - p4[2], e0[3] - p4[3]]
    return e, p4, p[3], Et


def label_of(e, p, e0, G, K, a, Y, curve):
    """The label alone (for bisections)."""
    _, p4, k0, Et = _trial(e, p, e0)
    return vmi_stress(Et, p4, k0, G, K, a, Y, curve)[1]


def point(e, p, e0, G, K, a, Y, curve):
    """One point, `p` = (p11, p22, gamma12, kappa) -> dict of mpf lists s (4), ds (9; zeros with no_tangent), ep (4: the new
    state rows), and label, no_tangent, overshoot, dist."""
    e, p4, k0, Et = _trial(e, p, e0)
    S, label, lam, over = vmi_stress(Et, p4, k0, G, K, a, Y, curve)
    big = max(abs(v) for v in Et)
    h = STEP * (big if big > 0 else _m(Y) / (2 * _m(G)))
    ds = [mp.mpf(0)] * 9
    no_tangent = False
    for j in range(3):
        up, dn = list(Et), list(Et)
        up[j] += h
        dn[j] -= h
        Su, lu, _, _ = vmi_stress(up, p4, k0, G, K, a, Y, curve)
        Sd, ld, _, _ = vmi_stress(dn, p4, k0, G, K, a, Y, curve)
        if lu != label or ld != label:
            no_tangent = True
            break
        for i in range(3):
            ds[3 * i + j] = (Su[i] - Sd[i]) / (2 * h)
    if not no_tangent:                                    # a float64 neighbour of the strain with another label
        ef = [float(v) for v in e]
        for j in range(3):
            for to in (-np.inf, np.inf):
                nb = list(ef)
                nb[j] = float(np.nextafter(ef[j], to))
                if label_of(nb, p, e0, G, K, a, Y, curve) != label:
                    no_tangent = True
    floor = mp.mpf(10) ** -40 * (2 * _m(G) + _m(K))
    ds = [mp.mpf(0) if no_tangent or abs(v) < floor else v for v in ds]
    if label == 0:
        ep = [p4[0], p4[1], p4[2], k0]
        k_new = k0
    else:
        el = _compliance(S, G, K)
        d = [Et[i] - el[i] for i in range(4)]
        k_new = k0 + _norm4([d[0], d[1], d[2] / 2, d[3]])
        ep = [p4[0] + d[0], p4[1] + d[1], p4[2] + d[2], k_new]
    if len(curve.k) == 1:
        dist = mp.mpf(1)
    else:
        dist = min(abs(k_new - b) for b in curve.k[1:]) / max(abs(k_new), curve.k[1])
    return {'s': S, 'ds': ds, 'ep': ep, 'label': label, 'no_tangent': no_tangent, 'overshoot': over, 'dist': dist}


def reference(e, p, e0, G, K, a, Y, kappa, slope):
    """Arrays e (3, n), p (4, n), e0 (4, n) per point, parameters (n,), one curve -> dict of float64 arrays s (4, n), ds (9, n),
    ep (4, n), overshoot, dist (n,), label (n,) int8 and no_tangent (n,) bool, each rounded once from the high-precision value."""
    curve = Curve(kappa, slope)
    n = e.shape[1]
    out = {'s': np.zeros((4, n)), 'ds': np.zeros((9, n)), 'ep': np.zeros((4, n)), 'overshoot': np.zeros(n), 'dist': np.zeros(n),
           'label': np.zeros(n, dtype=np.int8), 'no_tangent': np.zeros(n, dtype=bool)}
    for k in range(n):
        r = point(e[:, k], p[:, k], e0[:, k], G[k], K[k], a[k], Y[k], curve)
        for key in ('s', 'ds', 'ep'):
            out[key][:, k] = [float(v) for v in r[key]]
        out['overshoot'][k], out['dist'][k] = float(r['overshoot']), float(r['dist'])
        out['label'][k], out['no_tangent'][k] = r['label'], r['no_tangent']
    return out

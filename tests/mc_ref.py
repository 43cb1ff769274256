"""NumPy restatement of the third material model (test infrastructure): associative, perfectly plastic Mohr-Coulomb in
plane strain, the closest-point return map in principal stresses (elastic, smooth face, two edges, apex) with its
spectral tangent, and a MeshContext look-alike built on the pinned CPU restatement of geometry, B and the assembly
(oracle.fep_oracle).

Layout as for the other models: strain e (3, n) = (eps11, eps22, gamma12); 4-vectors (11, 22, 12, 33); the plastic strain
`p` holds the engineering shear in row 2.  Parameters per point: shear G, bulk K, sin_phi in (0, 1), cohesion c > 0.
Yield function, tension positive, sig1 >= sig2 >= sig3:  (1+s) sig1 - (1-s) sig3 - 2 c cos(phi) <= 0.

Every plastic branch is one formula on its own normal n (in the sorted principal frame):
    smooth  n = (1+s, 0, -(1-s))                    strains as they are
    left    n = ((1+s)/2, (1+s)/2, -(1-s))          e1, e2 replaced by their mean     (sig1 = sig2)
    right   n = (1+s, -(1-s)/2, -(1-s)/2)           e2, e3 replaced by their mean     (sig2 = sig3)
with A = 2G I + lam 11^T:  A n = 2G n + 2 lam s,  den = n . A n = 2G |n|^2 + 4 lam s^2,
    f = 2G n . e + 2 lam s tr - 2 c cos(phi),  L = f / den,  sig = (lam tr + 2G e~) - L A n,
    dsig/deps = lam + G M - (A n)(A n)^T / den      (M = 2I with the merged pair's 2x2 block replaced by ones).
The computation runs in the dtype asked for (np.longdouble measures the float64 run's own error)."""
import numpy as np

from model_ref import RefContext

BRANCHES = ('elastic', 'smooth', 'left', 'right', 'apex')


def _pick(pz, v0, v1, v2):
    return np.where(pz == 0, v0, np.where(pz == 1, v1, v2))


def mc_return_map(e, ep_prev, shear, bulk, sin_phi, c, apply_plastic_strain=False, e0=None, dtype=np.float64):
    """-> dict s (4,n), ds (9,n) row-major 3x3, ind_p, branch (0 elastic, 1 smooth, 2 left edge, 3 right edge, 4 apex),
    ep (4,n) (the updated COPY of ep_prev when `apply_plastic_strain`, else zeros), n_smooth (faces and edges), n_apex,
    and the conditioning of every point: 'f' the trial yield value, 'r', 'r_rel' = r / max|Et|, 'dist' the distance of the
    multipliers to the nearest branch boundary relative to the multiplier scale, 'margins' the signed differences it is the
    smallest of (L_s, L_s - min(g_sl, g_sr), L_edge - g_la or g_ra, g_sl - g_sr).  No argument is modified."""
    T = dtype
    e = np.asarray(e, dtype=T)
    n = e.shape[1]
    one = np.ones(n, dtype=T)
    G, K, s, c = (np.asarray(v, dtype=T) * one for v in (shear, bulk, sin_phi, c))
    p = np.zeros((4, n), dtype=T) if ep_prev is None else np.array(ep_prev, dtype=T)
    Et = np.concatenate([e, np.zeros((1, n), dtype=T)])
    if e0 is not None:
        Et = Et + np.asarray(e0, dtype=T).reshape(4, 1)
    Et = Et - p
    lam = K - 2 * G / 3
    G2 = 2 * G
    tr = Et[0] + Et[1] + Et[3]
    # 2: in-plane eigen-decomposition
    m, dd, h = (Et[0] + Et[1]) / 2, (Et[0] - Et[1]) / 2, Et[2] / 2
    tiny = np.maximum(np.abs(dd), np.abs(h)) < T(2.0) ** -500       # the squares kept out of the denormal range (exact scaling)
    with np.errstate(over='ignore'):
        dds, hs = np.where(tiny, dd * T(2.0) ** 600, dd), np.where(tiny, h * T(2.0) ** 600, h)
    rsc = np.sqrt(dds * dds + hs * hs)
    r = np.where(tiny, rsc * T(2.0) ** -600, rsc)
    ea, eb, ez = m + r, m - r, Et[3]
    rpos = rsc > 0
    rs = np.where(rpos, rsc, one)
    ca, sa = np.where(rpos, dds / rs, one), np.where(rpos, hs / rs, 0 * one)
    Pa = np.array([(1 + ca) / 2, (1 - ca) / 2, sa / 2])
    Pb = np.array([(1 - ca) / 2, (1 + ca) / 2, -sa / 2])
    # 3: stable descending sort; ea >= eb always, so only the place pz of ez varies
    pz = np.where(ez > ea, 0, np.where(ez > eb, 1, 2))
    e1, e2, e3 = _pick(pz, ez, ea, ea), _pick(pz, ea, ez, eb), _pick(pz, eb, eb, ez)
    # 4, 5: trial values and the branch
    cphi = np.sqrt(1 - s * s)
    ltr = lam * tr
    k0 = 2 * lam * s * tr - 2 * c * cphi
    f = G2 * ((1 + s) * e1 - (1 - s) * e3) + k0
    g_sl, g_sr = (e1 - e2) / (1 + s), (e2 - e3) / (1 - s)
    g_la, g_ra = (e1 + e2 - 2 * e3) / (3 - s), (2 * e1 - e2 - e3) / (3 + s)
    ls2 = 4 * lam * s * s
    den_s = ls2 + 4 * G * (1 + s * s)
    L_s = f / den_s
    left = g_sl < g_sr
    f_e = np.where(left, G * ((1 + s) * (e1 + e2) - 2 * (1 - s) * e3), G * (2 * (1 + s) * e1 - (1 - s) * (e2 + e3))) + k0
    den_e = ls2 + np.where(left, G * (1 + s) ** 2 + G2 * (1 - s) ** 2, G2 * (1 + s) ** 2 + G * (1 - s) ** 2)
    L_e = f_e / den_e
    g_lo, g_hi = np.where(left, g_sl, g_sr), np.where(left, g_la, g_ra)
    smooth = L_s <= g_lo
    edge = L_e <= g_hi                    # (g_lo <= L_e holds exactly when L_s >= g_lo: den_e (L_e - g_lo) = den_s (L_s - g_lo))
    # ~(f > 0), not f <= 0: a NaN f is elastic, and its stress NaN; it must not fall through every comparison to the apex
    branch = np.where(~(f > 0), 0, np.where(smooth, 1, np.where(edge, np.where(left, 2, 3), 4)))
    ml, mr = branch == 2, branch == 3
    # the branch's normal, strains and multiplier
    n1 = np.where(ml, (1 + s) / 2, 1 + s)
    n2 = np.where(ml, (1 + s) / 2, np.where(mr, -(1 - s) / 2, 0 * one))
    n3 = np.where(mr, -(1 - s) / 2, -(1 - s))
    m12, m23 = (e1 + e2) / 2, (e2 + e3) / 2
    t1, t2, t3 = np.where(ml, m12, e1), np.where(ml, m12, np.where(mr, m23, e2)), np.where(mr, m23, e3)
    L = np.where(branch == 0, 0 * one, np.where(branch == 1, L_s, L_e))
    ls = 2 * lam * s
    a1, a2, a3 = G2 * n1 + ls, G2 * n2 + ls, G2 * n3 + ls
    sig1, sig2, sig3 = (ltr + G2 * t1) - L * a1, (ltr + G2 * t2) - L * a2, (ltr + G2 * t3) - L * a3
    iden = np.where(branch == 0, 0 * one, 1 / np.where(branch == 1, den_s, den_e))
    two = 2 * one
    D11 = lam + G * np.where(ml, one, two) - a1 * a1 * iden
    D12 = lam + G * np.where(ml, one, 0 * one) - a1 * a2 * iden
    D13 = lam - a1 * a3 * iden
    D22 = lam + G * np.where(ml | mr, one, two) - a2 * a2 * iden
    D23 = lam + G * np.where(mr, one, 0 * one) - a2 * a3 * iden
    D33 = lam + G * np.where(mr, one, two) - a3 * a3 * iden
    apex = branch == 4
    sx = c * cphi / s
    sig1, sig2, sig3 = (np.where(apex, sx, v) for v in (sig1, sig2, sig3))
    D11, D12, D13, D22, D23, D33 = (np.where(apex, 0 * one, v) for v in (D11, D12, D13, D22, D23, D33))
    # 6: back to (a, b, z) and to the Cartesian frame
    sig_a, sig_b, sig_z = _pick(pz, sig2, sig1, sig1), _pick(pz, sig3, sig3, sig2), _pick(pz, sig1, sig2, sig3)
    Daa, Dbb, Dab = _pick(pz, D22, D11, D11), _pick(pz, D33, D33, D22), _pick(pz, D23, D13, D12)
    S = np.empty((4, n), dtype=T)
    S[0:3] = sig_a * Pa + sig_b * Pb
    S[3] = sig_z
    # theta from the difference itself: sig_a - sig_b = 2G [(t_a - t_b) - L (n_a - n_b)], and t_a - t_b = 2r where no edge merges
    ta, tb, na, nb = _pick(pz, t2, t1, t1), _pick(pz, t3, t3, t2), _pick(pz, n2, n1, n1), _pick(pz, n3, n3, n2)
    dt = np.where(ml | mr, ta - tb, 2 * r)
    theta = np.where(apex, 0 * one, np.where(rpos, G * ((dt - L * (na - nb)) / np.where(rpos, r, one)), Daa - Dab))
    I3 = (one, one, one / 2)
    idx = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    d = {}
    for i, j in idx:
        d[i, j] = d[j, i] = (Daa * (Pa[i] * Pa[j]) + Dab * (Pa[i] * Pb[j] + Pb[i] * Pa[j]) + Dbb * (Pb[i] * Pb[j])
                             + theta * ((I3[i] if i == j else 0 * one) - Pa[i] * Pa[j] - Pb[i] * Pb[j]))
    ds = np.array([d[i, j] for i in range(3) for j in range(3)])
    ind = branch != 0
    ep = np.zeros((4, n), dtype=T)
    if apply_plastic_strain:
        # 7: the plastic strain takes what the elastic strain of the new stress leaves of the trial strain
        th = (sig_a + sig_b + sig_z) / (3 * K)
        dpa, dpb, dpz = (ei - (si - lam * th) / G2 for ei, si in ((ea, sig_a), (eb, sig_b), (ez, sig_z)))
        inc = np.array([dpa * Pa[0] + dpb * Pb[0], dpa * Pa[1] + dpb * Pb[1], 2 * (dpa * Pa[2] + dpb * Pb[2]), dpz])
        ep = p + np.where(ind, inc, 0 * one)
    # conditioning: distances to the branch boundaries in multiplier units
    scale = np.maximum.reduce([np.abs(L_s), np.abs(g_sl), np.abs(g_sr), np.abs(g_la), np.abs(g_ra)])
    plastic_dist = np.where(smooth, np.abs(L_s - g_lo),
                            np.minimum.reduce([np.abs(L_s - g_lo), np.abs(L_e - g_hi), np.abs(g_sl - g_sr)]))
    et_max = np.abs(Et).max(axis=0)
    with np.errstate(invalid='ignore'):                     # a point without strain is exact: r == 0, f = -2 c cos(phi)
        dist = np.where(scale > 0, np.minimum(np.abs(L_s), np.where(f <= 0, np.abs(L_s), plastic_dist)) / scale, one)
        r_rel = np.where(et_max > 0, r / et_max, one)
    return {'s': S, 'ds': ds, 'ind_p': ind, 'branch': branch, 'ep': ep, 'f': f, 'r': r, 'r_rel': r_rel, 'dist': dist,
            'margins': dict(L_s=L_s, face=L_s - g_lo, apex=L_e - g_hi, side=g_sl - g_sr),
            'n_smooth': int(((branch >= 1) & (branch <= 3)).sum()), 'n_apex': int(apex.sum()),
            'principal': dict(e=(e1, e2, e3), sig=(sig1, sig2, sig3), pz=pz, Pa=Pa, Pb=Pb, abz=(sig_a, sig_b, sig_z))}


class MCRefContext(RefContext):
    """The Mohr-Coulomb look-alike; `branches` holds, per accepting call, the number of points per branch."""
    model, return_map, passed = 'mc', staticmethod(mc_return_map), ('branch', 'f', 'r_rel', 'dist')

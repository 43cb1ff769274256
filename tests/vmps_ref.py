"""NumPy float64 restatement of the fourth material model (test infrastructure): von Mises plasticity with linear
kinematic hardening in PLANE STRESS (include/fep.h, fep_return_map_vmps_*), and its MeshContext look-alike.

Layout as tests/vm_ref.py: strain e (3, n) = (eps11, eps22, gamma12); 4-vectors (11, 22, 12, 33); the plastic strain `p`
holds the engineering shear in row 2.  Parameters per point: shear G, bulk K, hardening modulus a >= 0 and yield radius
Y = sqrt(2/3) sigma_y > 0.  s[3] = 0; row 3 of e0 and p enters only through the propagation of non-finite values."""
import numpy as np

from model_ref import RefContext

MAX_ITER = 16                                                           # kVmpsMaxIter
TOL = 2.0 ** -51                                                        # kVmpsTol


def elastic_matrix(G, K):
    """(lb, C) of plane stress from the shear and bulk moduli: lb = 2G lam / (lam + 2G), C (3, 3) for scalars."""
    lam = K - 2 * G / 3
    lb = 2 * G * lam / (lam + 2 * G)
    return lb, np.array([[lb + 2 * G, lb, 0 * G], [lb, lb + 2 * G, 0 * G], [0 * G, 0 * G, G]])


def vmps_return_map(e, ep_prev, shear, bulk, a, Y, apply_plastic_strain=False, e0=None):
    """-> dict s (4,n), ds (9,n) row-major 3x3, ind_p (n,), crit (n,) = sqrt(eta^T P eta) - Y, gamma (n,), its (n,) the Newton
    iterations a point took, surface (n,) = sqrt(eta'^T P eta') - Y of the returned state (0 for elastic points), ep (4,n)
    (the updated COPY of ep_prev when `apply_plastic_strain`, else zeros), n_plast.  No argument is modified."""
    e = np.asarray(e, dtype=float)
    n = e.shape[1]
    one = np.ones(n)
    G, K, a, Y = (np.asarray(v, dtype=float) * one for v in (shear, bulk, a, Y))
    p = np.zeros((4, n)) if ep_prev is None else np.array(ep_prev, dtype=float)
    z = np.zeros((4, 1)) if e0 is None else np.asarray(e0, dtype=float).reshape(4, -1)          # (4, 1), or (4, n) per point
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        ee = (e + z[0:3]) - p[0:3]
        Et3 = (0.0 + z[3]) - p[3]
        G2 = 2 * G
        lam = K - G2 / 3
        lb = G2 * lam / (lam + G2)
        c00 = lb + G2
        st = np.array([c00 * ee[0] + lb * ee[1], lb * ee[0] + c00 * ee[1], G * ee[2]])
        ab = np.array([a * (2 * p[0] + p[1]), a * (2 * p[1] + p[0]), a * (0.5 * p[2])])
        h0, h1, h12 = st - ab
        hs, hd = h0 + h1, h0 - h1
        cs, cd = (2 * lb + G2) / 3 + a, G2 + a
        qs, qd = hs * hs / 6, 0.5 * (hd * hd) + 2 * (h12 * h12)
        poison = -np.abs(0.0 * (((np.abs(ee[0]) + np.abs(ee[1])) + np.abs(ee[2])) + np.abs(Et3)))     # -0.0, or NaN for a non-finite trial strain
        n2 = (qs + qd) + poison
        Y2 = Y * Y
        ind = n2 - Y2 > 0                                               # a NaN is elastic
        g = np.where(ind, (np.sqrt(n2) / Y - 1) / np.maximum(cs, cd), 0.0)
        its = np.zeros(n, dtype=np.int64)
        live = ind.copy()
        for _ in range(MAX_ITER):
            if not live.any():
                break
            us, ud = 1 + cs * g, 1 + cd * g
            fs, fd = qs / (us * us), qd / (ud * ud)
            dg = ((fs + fd) - Y2) / (2 * (cs * (fs / us) + cd * (fd / ud)))
            g = np.where(live, g + dg, g)
            its += live
            live = live & (np.abs(dg) * cd > TOL * (1 + cd * g))
        us, ud = 1 + cs * g, 1 + cd * g
        hs1, hd1, h121 = hs / us, hd / ud, h12 / ud
        n0, n1 = 0.5 * (hs1 + hd1), 0.5 * (hs1 - hd1)
        Pn = np.array([(2 * n0 - n1) / 3, (2 * n1 - n0) / 3, 2 * h121])
        dp = g * Pn
        ag = 1 + a * g
        # st - C dp without its cancellation: (1 + a g) eta' + ab (include/fep.h); elastic points keep the trial stress
        s = np.concatenate([np.where(ind, ag * np.array([n0, n1, h121]) + ab, st), (0.0 + poison).reshape(1, n)])
        th = g / ag
        xs, xd, xh = 1 / (1 / (2 * lb + G2) + th / 3), 1 / (1 / G2 + th), 1 / (1 / G + 2 * th)
        ns, nd, nh = xs * (hs1 / 3), xd * hd1, xh * Pn[2]
        v = np.array([0.5 * (ns + nd), 0.5 * (ns - nd), nh])
        w = 1 / ((Pn * v).sum(axis=0) + a * Y2 * ag)
        Xi = np.array([0.5 * (xs + xd), 0.5 * (xs - xd), 0 * xs, 0.5 * (xs - xd), 0.5 * (xs + xd), 0 * xs, 0 * xs, 0 * xs, xh])
        zero = 0 * G
        C = np.array([c00, lb, zero, lb, c00, zero, zero, zero, G])
        vv = np.array([v[i] * v[j] for i in range(3) for j in range(3)])
        ds = np.where(ind, Xi - w * vv, C)
        surface = np.where(ind, np.sqrt(hs1 * hs1 / 6 + 0.5 * (hd1 * hd1) + 2 * (h121 * h121)) - Y, 0.0)
    ep = np.zeros((4, n))
    if apply_plastic_strain:
        ep = p.copy()
        ep[:, ind] += np.array([dp[0], dp[1], dp[2], -(dp[0] + dp[1])])[:, ind]
    return {'s': s, 'ds': ds, 'ind_p': ind, 'crit': np.sqrt(np.where(n2 > 0, n2, 0.0)) - Y, 'gamma': g, 'its': its,
            'surface': surface, 'ep': ep, 'n_plast': int(ind.sum())}


def surface_residual(s, p, a, Y):
    """sqrt(eta^T P eta) - Y of a returned state: eta = s[0:3] - a (2 p0 + p1, 2 p1 + p0, p2 / 2) from the stress and the
    NEW plastic strain (the check that an iteration stopped by its cap cannot pass)."""
    h0, h1, h12 = s[0] - a * (2 * p[0] + p[1]), s[1] - a * (2 * p[1] + p[0]), s[2] - a * (0.5 * p[2])
    hs, hd = h0 + h1, h0 - h1
    return np.sqrt(hs * hs / 6 + 0.5 * (hd * hd) + 2 * (h12 * h12)) - Y


def _vmps_step_map(*a, **k):
    """vmps_return_map with the counters as a context's step reports them: the plastic count and no apex."""
    r = vmps_return_map(*a, **k)
    return dict(r, n_smooth=r['n_plast'], n_apex=0)


class VMPSRefContext(RefContext):
    """The plane-stress von Mises look-alike."""
    model, return_map, passed = 'vmps', staticmethod(_vmps_step_map), ('crit',)

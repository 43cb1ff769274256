"""NumPy float64 restatement of the fifth material model (test infrastructure): von Mises plasticity in plane strain with
isotropic hardening on a piecewise-linear curve next to the linear kinematic one (include/fep.h, fep_return_map_vmi_*), and
its MeshContext look-alike.  It follows the law of the header statement by statement: the trial state in the expressions of
tests/vm_ref.py (so one flat segment gives that restatement's bits), the start segment, the walk over the segments and the
update in the operations and the order of the kernel (vmi_return_map in csrc/fep_kernels.hip.h, which fuses no product into
a sum).

Layout as for von Mises, except the state: `p` (4, n) holds (p11, p22, gamma12 (engineering), kappa); p33 = -(p11 + p22) is
implied.  The curve is `kappa` (n_seg,), kappa[0] = 0 and increasing, with one slope per segment; the last segment runs to
infinity."""
import numpy as np

from model_ref import RefContext

IOTA = np.array([1.0, 1.0, 0.0, 1.0])
MAX_SEGMENTS = 8                                            # FEP_MAX_HARDENING_SEGMENTS


def curve_tables(kappa, slope):
    """(kappa, R, slope) as the library hands them to its kernels: R[0] = 0, R[j+1] = R[j] + slope[j] (kappa[j+1] - kappa[j])
    in this order."""
    kappa = np.array(kappa, dtype=float).ravel()
    slope = np.array(slope, dtype=float).ravel()
    assert kappa.size == slope.size and 1 <= kappa.size <= MAX_SEGMENTS and kappa[0] == 0 and (np.diff(kappa) > 0).all()
    R = np.zeros(kappa.size)
    for j in range(1, kappa.size):
        R[j] = R[j - 1] + slope[j - 1] * (kappa[j] - kappa[j - 1])
    return kappa, R, slope


def radius_growth(kappa, slope, k):
    """R(k) by the formula of the start segment (the yield test's): for diagnostics and hand formulas."""
    kap, R, slo = curve_tables(kappa, slope)
    k = np.asarray(k, dtype=float)
    j = np.clip(np.searchsorted(kap, k, side='right') - 1, 0, kap.size - 1)
    return R[j] + slo[j] * (k - kap[j])


def vmi_return_map(e, ep_prev, shear, bulk, a, Y, curve, apply_plastic_strain=False, e0=None):
    """-> dict s (4,n), ds (9,n) row-major 3x3, ind_p (n,), crit (n,), ep (4,n) (the updated COPY of ep_prev when
    `apply_plastic_strain`, else zeros), n_plast, seg (n,) the accepted segment of a plastic point (-1: elastic), lam (n,).
    No argument is modified."""
    kap, R, slo = curve_tables(*curve)
    n_seg = kap.size
    e = np.asarray(e, dtype=float)
    n = e.shape[1]
    one = np.ones(n)
    G, K, a, Y = (np.asarray(v, dtype=float) * one for v in (shear, bulk, a, Y))
    p = np.zeros((4, n)) if ep_prev is None else np.array(ep_prev, dtype=float)
    k0 = p[3].copy()
    p3 = -(p[0] + p[1])
    pt = np.array([p[0], p[1], p[2], p3])
    Et = np.concatenate([e, np.zeros((1, n))])
    if e0 is not None:
        Et = Et + np.asarray(e0, dtype=float).reshape(4, -1)                # one for all points, or one per point
    Et = Et - pt
    with np.errstate(invalid='ignore', over='ignore'):
        tr = Et[0] + Et[1] + Et[3]
        dv = np.array([Et[0] - tr / 3, Et[1] - tr / 3, Et[2] / 2, Et[3] - tr / 3])
        poison = -np.abs(0.0 * k0)                          # -0.0, or NaN for a NaN / infinite kappa
        s = 2 * G * dv + (K * tr + poison) * IOTA.reshape(4, 1)
        xi = 2 * G * dv - a * np.array([pt[0], pt[1], pt[2] / 2, pt[3]])
        nrm = np.sqrt(xi[0] ** 2 + xi[1] ** 2 + 2 * xi[2] ** 2 + xi[3] ** 2) + poison
        # start segment: the last comparison kappa[j] <= k0 that holds
        crit = nrm - (Y + (R[0] + slo[0] * (k0 - kap[0])))
        j0 = np.zeros(n, dtype=int)
        for j in range(1, n_seg):
            at = kap[j] <= k0
            crit = np.where(at, nrm - (Y + (R[j] + slo[j] * (k0 - kap[j]))), crit)
            j0[at] = j
        ind = crit > 0
        iota3 = np.array([1.0, 1.0, 0.0])
        Vol = np.outer(iota3, iota3)
        Dev = np.diag([1.0, 1.0, 0.5]) - Vol / 3
        ds = 2 * Dev.reshape(-1, 1) * G + Vol.reshape(-1, 1) * K
        ep = np.zeros((4, n))
        if apply_plastic_strain:
            ep = p.copy()
        seg = np.full(n, -1)
        lam_all = np.zeros(n)
        if ind.any():
            Gp, ap, Yp, kp, nr = G[ind], a[ind], Y[ind], k0[ind], nrm[ind]
            lam, H = np.zeros(kp.size), np.ones(kp.size)
            open_ = np.ones(kp.size, dtype=bool)
            sg = np.full(kp.size, -1)
            for j in range(n_seg):
                Hj = (2 * Gp + ap) + slo[j]
                lj = (nr - (Yp + (R[j] + slo[j] * (kp - kap[j])))) / Hj
                take = open_ & (j >= j0[ind])
                if j + 1 < n_seg:
                    take = take & (kp + lj <= kap[j + 1])
                lam, H = np.where(take, lj, lam), np.where(take, Hj, H)
                sg[take] = j
                open_ = open_ & ~take
            N = xi[:, ind] / nr
            s[:, ind] = s[:, ind] - 2 * Gp * lam * N
            NN = np.tile(N[0:3], (3, 1)) * np.repeat(N[0:3], 3, axis=0)
            ID = np.outer(Dev.flatten(), np.ones(int(ind.sum())))
            ds[:, ind] = ds[:, ind] - (2 * Gp) ** 2 / H * NN - (2 * Gp) ** 2 * lam / nr * (ID - NN)
            seg[ind], lam_all[ind] = sg, lam
            if apply_plastic_strain:
                ep[0:3, ind] += lam * np.array([N[0], N[1], 2 * N[2]])
                ep[3, ind] = kp + lam
    return {'s': s, 'ds': ds, 'ind_p': ind, 'crit': crit, 'ep': ep, 'n_plast': int(ind.sum()), 'seg': seg, 'lam': lam_all}


class VMIRefContext(RefContext):
    """The look-alike of a 'vmi' context: `set_hardening(kappa, slope)` as MeshContext's, one flat segment without it."""
    model, passed = 'vmi', ('crit',)

    def __init__(self, *a):
        super().__init__(*a)
        self.hardening = (np.zeros(1), np.zeros(1))

    def set_hardening(self, kappa, slope):
        curve_tables(kappa, slope)
        self.hardening = (np.array(kappa, dtype=float).ravel(), np.array(slope, dtype=float).ravel())

    def return_map(self, e, ep_prev, *mats, apply_plastic_strain=False, e0=None):
        r = vmi_return_map(e, ep_prev, *mats, self.hardening, apply_plastic_strain=apply_plastic_strain, e0=e0)
        return dict(r, n_smooth=r['n_plast'], n_apex=0)

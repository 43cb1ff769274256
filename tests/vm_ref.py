"""NumPy float64 restatement of the second material model (test infrastructure): von Mises plasticity with linear
kinematic hardening in plane strain, radial return with the symmetric consistent tangent, and a MeshContext
look-alike built on the pinned CPU restatement of geometry, B and the assembly (oracle.fep_oracle).

Layout as for Drucker-Prager: strain e (3, n) = (eps11, eps22, gamma12); 4-vectors (11, 22, 12, 33); the plastic strain
`p` holds the engineering shear in row 2.  Parameters per point: shear G, bulk K, hardening modulus a >= 0 and yield
radius Y = sqrt(2/3) sigma_y > 0.  The back stress is a * p: the plastic strain is the only state."""
import numpy as np

from model_ref import RefContext

IOTA = np.array([1.0, 1.0, 0.0, 1.0])


def vm_return_map(e, ep_prev, shear, bulk, a, Y, apply_plastic_strain=False, e0=None):
    """-> dict s (4,n), ds (9,n) row-major 3x3, ind_p (n,), crit (n,), ep (4,n) (the updated COPY of ep_prev when
    `apply_plastic_strain`, else zeros), n_plast.  No argument is modified."""
    e = np.asarray(e, dtype=float)
    n = e.shape[1]
    one = np.ones(n)
    G, K, a, Y = (np.asarray(v, dtype=float) * one for v in (shear, bulk, a, Y))
    p = np.zeros((4, n)) if ep_prev is None else np.array(ep_prev, dtype=float)
    Et = np.concatenate([e, np.zeros((1, n))])
    if e0 is not None:
        Et = Et + np.asarray(e0, dtype=float).reshape(4, 1)
    Et = Et - p
    tr = Et[0] + Et[1] + Et[3]
    dv = np.array([Et[0] - tr / 3, Et[1] - tr / 3, Et[2] / 2, Et[3] - tr / 3])
    s = 2 * G * dv + K * tr * IOTA.reshape(4, 1)
    xi = 2 * G * dv - a * np.array([p[0], p[1], p[2] / 2, p[3]])
    nrm = np.sqrt(xi[0] ** 2 + xi[1] ** 2 + 2 * xi[2] ** 2 + xi[3] ** 2)
    crit = nrm - Y
    ind = crit > 0
    iota3 = np.array([1.0, 1.0, 0.0])
    Vol = np.outer(iota3, iota3)
    Dev = np.diag([1.0, 1.0, 0.5]) - Vol / 3
    ds = 2 * Dev.reshape(-1, 1) * G + Vol.reshape(-1, 1) * K
    ep = np.zeros((4, n))
    if apply_plastic_strain:
        ep = p.copy()
    if ind.any():
        Gp, ap = G[ind], a[ind]
        lam = crit[ind] / (2 * Gp + ap)
        N = xi[:, ind] / nrm[ind]
        s[:, ind] = s[:, ind] - 2 * Gp * lam * N
        NN = np.tile(N[0:3], (3, 1)) * np.repeat(N[0:3], 3, axis=0)
        ID = np.outer(Dev.flatten(), np.ones(int(ind.sum())))
        ds[:, ind] = (ds[:, ind] - (2 * Gp) ** 2 / (2 * Gp + ap) * NN
                      - (2 * Gp) ** 2 * lam / nrm[ind] * (ID - NN))
        if apply_plastic_strain:
            ep[:, ind] += lam * np.array([N[0], N[1], 2 * N[2], N[3]])
    return {'s': s, 'ds': ds, 'ind_p': ind, 'crit': crit, 'ep': ep, 'n_plast': int(ind.sum())}


def _vm_step_map(*a, **k):
    """vm_return_map with the counters as a context's step reports them: the plastic count and no apex."""
    r = vm_return_map(*a, **k)
    return dict(r, n_smooth=r['n_plast'], n_apex=0)


class VMRefContext(RefContext):
    """The von Mises look-alike ('dp' is refused: the Drucker-Prager look-alike is OracleContext)."""
    model, return_map, passed = 'vm', staticmethod(_vm_step_map), ('crit',)

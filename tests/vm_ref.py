"""NumPy float64 restatement of the second material model (test infrastructure): von Mises plasticity with linear
kinematic hardening in plane strain, radial return with the symmetric consistent tangent, and a MeshContext
look-alike built on the pinned CPU restatement of geometry, B and the assembly (oracle.fep_oracle).

Layout as for Drucker-Prager: strain e (3, n) = (eps11, eps22, gamma12); 4-vectors (11, 22, 12, 33); the plastic strain
`p` holds the engineering shear in row 2.  Parameters per point: shear G, bulk K, hardening modulus a >= 0 and yield
radius Y = sqrt(2/3) sigma_y > 0.  The back stress is a * p: the plastic strain is the only state."""
import numpy as np

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


class VMRefContext:
    """Shaped like tests/oracle_context.OracleContext; the model is von Mises whatever `set_model` is told last, except
    that 'dp' is refused (the Drucker-Prager look-alike is OracleContext)."""

    def __init__(self, elem, coord, d1, d2, wf):
        from oracle import fep_oracle as orc
        self.orc, self.elem, self.coord, self.tab = orc, np.asarray(elem), np.asarray(coord, dtype=float), (d1, d2, wf)
        self.n_int = self.elem.shape[1] * np.size(wf)
        self.n_n = self.coord.shape[1]
        self.model = 'vm'

    def set_model(self, model):
        if model != 'vm':
            raise ValueError('VMRefContext restates the von Mises model only')

    def set_materials(self, sh, bu, a, Y):
        one = np.ones(self.n_int)
        self.m = tuple(np.asarray(v, dtype=float).ravel() * one for v in (sh, bu, a, Y))
        K, B, w, iD, jD, D = self.orc.elastic_setup(self.elem, self.coord, self.m[0], self.m[1], *self.tab)
        self.c = dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD)

    def geometry(self):
        return None, None, self.c['weight'], None

    def step(self, U, ep_prev=None, e0=None, apply_plastic_strain=False, want=()):
        """As MeshContext.step on a von Mises context: `ep_prev` is updated in place on accept; every output is returned
        whatever `want` names ('n_smooth' carries the plastic count, 'n_apex' is 0)."""
        c = self.c
        U2 = np.asarray(U, dtype=float).reshape((2, -1), order='F') if np.ndim(U) == 1 else np.asarray(U, dtype=float)
        E = self.orc.strain(c['B'], U2)
        accept = bool(apply_plastic_strain) and ep_prev is not None
        r = vm_return_map(E, ep_prev, *self.m, apply_plastic_strain=accept, e0=e0)
        if accept:
            ep_prev[...] = r['ep']
        K_t = self.orc.tangent(c['K_elast'], c['B'], c['D_elast'], c['weight'], r['ds'], c['iD'], c['jD'])
        F = self.orc.internal_force(c['B'], c['weight'], r['s'])
        return {'E': np.asarray(E), 'K': K_t.tocsr(), 'F': F, 's': r['s'], 'ds': r['ds'], 'ind_p': r['ind_p'],
                'crit': r['crit'], 'n_smooth': r['n_plast'], 'n_apex': 0}

    def close(self):
        pass

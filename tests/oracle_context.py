"""MeshContext look-alike backed by the CPU oracle (test infrastructure): the drivers' `context_factory` takes it, so the
same load-step / Newton loop runs with another hot path, and without a GPU."""
import numpy as np


class OracleContext:

    def __init__(self, elem, coord, d1, d2, wf):
        from oracle import fep_oracle as orc
        self.orc, self.elem, self.coord, self.tab = orc, elem, coord, (d1, d2, wf)
        self.n_int = elem.shape[1] * wf.size

    def set_materials(self, sh, bu, eta, c):
        one = np.ones(self.n_int)
        self.m = (sh * one, bu * one, eta * one, c * one)
        K, B, w, iD, jD, D = self.orc.elastic_setup(self.elem, self.coord, self.m[0], self.m[1], *self.tab)
        self.c = dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=self.m[0], bulk=self.m[1],
                      eta=self.m[2], c=self.m[3])

    def geometry(self):
        return None, None, self.c['weight'], None

    def step(self, U, ep_prev=None, e0=None, apply_plastic_strain=False, want=()):
        """`e0` (4,1) selects the TSX flavour of the return map (TSX:1052), as it does in MeshContext.step."""
        U2 = np.asarray(U).reshape((2, -1), order='F') if np.ndim(U) == 1 else U
        E, cp, K_t, F = self.orc.hot_path(U2, ep_prev, self.c, apply_plastic_strain=apply_plastic_strain,
                                          e0=e0, tsx=e0 is not None)
        return {'K': K_t.tocsr(), 'F': F, 's': cp['s'], 'ds': cp['ds'], 'ind_p': cp['ind_p'],
                'n_smooth': cp['n_smooth'], 'n_apex': cp['n_apex']}

    def assemble(self, ds=None, s=None):
        """F from given point stresses (TSX:1737); the drivers ask for no K here."""
        assert ds is None
        return None, self.orc.internal_force(self.c['B'], self.c['weight'], np.asarray(s, dtype=float))

    def close(self):
        pass

"""Shared by the tests of the material models (test infrastructure): the MeshContext look-alike on a model's NumPy
restatement, the caller of the mesh-free device entry points, and the comparisons the model tests have in common."""
import ctypes

import numpy as np

from conftest import relerr, relerr_points

DEV_ENTRY = {'dp': 'fep_return_map_dev', 'vm': 'fep_return_map_vm_dev', 'mc': 'fep_return_map_mc_dev'}


def traceless(rng, n, scale):
    p = rng.normal(0, scale, size=(4, n))
    p[[0, 1, 3]] -= (p[0] + p[1] + p[3]) / 3
    return p


def check_points(got, ref, keys, tol, tol_pt):
    """Every array of `keys`: `tol` of the array maximum and `tol_pt` per point."""
    for k in keys:
        print(k, relerr(got[k], ref[k]), relerr_points(got[k], ref[k]))
        assert relerr(got[k], ref[k]) <= tol and relerr_points(got[k], ref[k]) <= tol_pt, k


def bytes_equal(a, b, keys=('s', 'ds', 'ind_p', 'F')):
    return all(np.array_equal(a[k], b[k]) for k in keys) and np.array_equal(a['K'].data, b['K'].data) \
        and (a['n_smooth'], a['n_apex']) == (b['n_smooth'], b['n_apex'])


def dev_return_map(fep, model, e, order, p, e0, mats, accept):
    """The model's mesh-free device entry point on torch tensors; the strain (3, n) is handed over in `order`, `p` may be
    None.  -> s, ds, ind_p, the two counters as n_smooth / n_apex, 'ep' the device copy of p afterwards."""
    import torch
    dev = torch.device('cuda', 0)
    n = mats[0].size
    up = lambda v: torch.from_numpy(np.array(v, dtype=np.float64, order='C')).to(dev)     # noqa: E731  (a writable copy)
    ed = up(e.T if order == 'F' else e)
    ps, cs = (3, 1) if order == 'F' else (1, n)
    pd = None if p is None else up(p)
    md = [up(m) for m in mats]
    f64 = dict(dtype=torch.float64, device=dev)
    S, DS = torch.zeros((4, n), **f64), torch.zeros((9, n), **f64)
    ind, cnt = torch.zeros(n, dtype=torch.uint8, device=dev), torch.full((2,), -1, dtype=torch.int64, device=dev)
    e0v = None if e0 is None else np.ascontiguousarray(e0, dtype=np.float64).ravel()
    rc = getattr(fep.lib(), DEV_ENTRY[model])(0, torch.cuda.current_stream().cuda_stream, n, ed.data_ptr(), ps, cs,
                                              None if e0v is None else e0v.ctypes.data_as(ctypes.c_void_p),
                                              None if pd is None else pd.data_ptr(), *(m.data_ptr() for m in md),
                                              int(accept), S.data_ptr(), DS.data_ptr(), ind.data_ptr(), cnt.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    k = cnt.cpu().numpy()
    return {'s': S.cpu().numpy(), 'ds': DS.cpu().numpy(), 'ind_p': ind.cpu().numpy().astype(bool), 'n_smooth': int(k[0]),
            'n_apex': int(k[1]), 'ep': None if pd is None else pd.cpu().numpy()}


class RefContext:
    """Shaped like tests/oracle_context.OracleContext, on the pinned CPU restatement of geometry, B and the assembly
    (oracle.fep_oracle) and a model's restated return map.  A subclass names its `model`, `return_map(e, ep_prev, four
    materials, apply_plastic_strain=, e0=)` -> dict with s, ds, ind_p, ep, n_smooth, n_apex, and the further keys of that
    dict which `step` passes through.  The model is the subclass's whatever `set_model` is told last, except that any other
    is refused."""
    model, return_map, passed = None, None, ()

    def __init__(self, elem, coord, d1, d2, wf):
        from oracle import fep_oracle as orc
        self.orc, self.elem, self.coord, self.tab = orc, np.asarray(elem), np.asarray(coord, dtype=float), (d1, d2, wf)
        self.n_int = self.elem.shape[1] * np.size(wf)
        self.n_n = self.coord.shape[1]
        self.branches = []                                  # per accepting call: the number of points per branch, if told

    def set_model(self, model):
        if model != self.model:
            raise ValueError(f'{type(self).__name__} restates the {self.model} model only')

    def set_materials(self, *mats):
        one = np.ones(self.n_int)
        self.m = tuple(np.asarray(v, dtype=float).ravel() * one for v in mats)
        K, B, w, iD, jD, D = self.orc.elastic_setup(self.elem, self.coord, self.m[0], self.m[1], *self.tab)
        self.c = dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD)

    def geometry(self):
        return None, None, self.c['weight'], None

    def step(self, U, ep_prev=None, e0=None, apply_plastic_strain=False, want=()):
        """As MeshContext.step on a context of the model: `ep_prev` is updated in place on accept; every output is returned
        whatever `want` names."""
        c = self.c
        U2 = np.asarray(U, dtype=float).reshape((2, -1), order='F') if np.ndim(U) == 1 else np.asarray(U, dtype=float)
        E = self.orc.strain(c['B'], U2)
        accept = bool(apply_plastic_strain) and ep_prev is not None
        r = self.return_map(E, ep_prev, *self.m, apply_plastic_strain=accept, e0=e0)
        if accept:
            ep_prev[...] = r['ep']
            if 'branch' in r:
                self.branches.append(np.bincount(r['branch'], minlength=5))
        K_t = self.orc.tangent(c['K_elast'], c['B'], c['D_elast'], c['weight'], r['ds'], c['iD'], c['jD'])
        F = self.orc.internal_force(c['B'], c['weight'], r['s'])
        return {'E': np.asarray(E), 'K': K_t.tocsr(), 'F': F,
                **{k: r[k] for k in ('s', 'ds', 'ind_p', 'n_smooth', 'n_apex') + self.passed}}

    def close(self):
        pass

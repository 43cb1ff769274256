"""
Host-side mirror of the reference's interface for the hot path, on top of the
C ABI (include/fep.h -> csrc/libfep_hip.so).  All arithmetic of the path runs in the HIP
kernels; this module only normalises NumPy layouts, keeps the reference's return
conventions (shapes, aliasing quirks) and wraps CSR values into SciPy matrices.

Reference interface mirrored here (DP = Plasticity2D_DP/pythonFEM.py, TSX = tsx-tunnel/pythonFEM.py):
  construct_constitutive_problem   DP:604-757 / TSX:990-1157
  get_elastic_stiffness_matrix     DP:491-601 / TSX:432-542 / EL:368-477
  (inline) tangent + residual      DP:1047-1058 / TSX:1773-1778  ->  assemble_tangent / MeshContext.step
"""
import ctypes as C
import os
import weakref

import numpy as np
import scipy.sparse as ssp

from . import _lib
from .hardening import check_curve
from .tables import (ELEMENT_SHAPE, LagrangeElementType, _coerce, element_tables, get_local_basis_volume,
                     get_quadrature_volume)

_NP_TO_TYPE = {3: LagrangeElementType.P1, 6: LagrangeElementType.P2, 4: LagrangeElementType.Q1,
               8: LagrangeElementType.Q2, 15: LagrangeElementType.P4}


def default_device():
    for var in ('FEP_DEVICE', 'LOCAL_RANK'):
        if os.environ.get(var, '') != '':
            return int(os.environ[var])
    return 0


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        a = np.ascontiguousarray(a.reshape(shape))
    return a


def _strain_view(e, n_int):
    """(array kept alive, point stride, component stride) of a (3,n_int) strain in either
    memory order: the driver hands over an F-ordered array (DP:1043), tests C-ordered ones."""
    e = np.asarray(e, dtype=np.float64)
    if e.shape != (3, n_int):
        raise ValueError(f'strain must be (3,{n_int}), got {e.shape}')
    if not (e.flags.c_contiguous or e.flags.f_contiguous):
        e = np.ascontiguousarray(e)
    if n_int == 1 or e.flags.f_contiguous and not e.flags.c_contiguous:
        return np.asfortranarray(e), 3, 1
    return e, 1, n_int


# ---------------------------------------------------------------------------------------
# a2  construct_constitutive_problem
# ---------------------------------------------------------------------------------------
def _return_map(e, e0, ep_prev, shear, bulk, eta, c, apply_plastic_strain, tsx, device=None, entry='fep_return_map_host',
                field=None, curve=None):
    l = _lib.lib()
    dev = default_device() if device is None else device
    shear = _f64(shear).ravel()
    n_int = shear.size
    bulk, eta, c = _f64(bulk).ravel(), _f64(eta).ravel(), _f64(c).ravel()
    ev, ps, cs = _strain_view(e, n_int)
    e0v = None if e0 is None else _f64(e0).ravel()
    if e0v is not None and e0v.size != 4:
        raise ValueError('e0 must hold 4 values (broadcast (4,1) initial strain, TSX:1052)')
    ep_dev = None
    if ep_prev is not None:
        if ep_prev.shape != (4, n_int):
            raise ValueError(f'ep_prev must be (4,{n_int})')
        # the kernel writes the plastic strain only on accepting calls: otherwise the caller's array is read in place
        direct = (isinstance(ep_prev, np.ndarray) and ep_prev.dtype == np.float64 and ep_prev.flags.c_contiguous
                  and (ep_prev.flags.writeable or not apply_plastic_strain))
        ep_dev = ep_prev if direct else _f64(ep_prev).copy()
    s = _lib.pinned_empty((4, n_int))                  # outputs in page-locked memory: DMA-ed straight into them
    ds = _lib.pinned_empty((9, n_int))
    ind = _lib.pinned_empty(n_int, np.uint8)
    counts = np.zeros(2, dtype=np.int64)
    accept = bool(apply_plastic_strain) and ep_prev is not None
    if field is not None:                              # (model, e0_field, e0_scale): the one entry point of every model
        model, fld, scale = field
        fld = _f64(fld)
        if fld.shape != (4, n_int):
            raise ValueError(f'e0_field must be (4,{n_int}), got {fld.shape}')
        _lib.check(l.fep_return_map_field_host(MODELS[model], dev, n_int, _lib.ptr(ev), ps, cs, _lib.ptr(e0v), _lib.ptr(fld),
                                               float(scale), _lib.ptr(ep_dev), _lib.ptr(shear), _lib.ptr(bulk), _lib.ptr(eta),
                                               _lib.ptr(c), int(accept), _lib.ptr(s), _lib.ptr(ds), _lib.ptr(ind),
                                               _lib.ptr(counts)), 'fep_return_map_field_host')
    elif curve is not None:                            # (kappa, slope): the model with a hardening curve
        kap, slo = curve
        _lib.check(getattr(l, entry)(dev, n_int, _lib.ptr(ev), ps, cs, _lib.ptr(e0v), _lib.ptr(ep_dev),
                                     _lib.ptr(shear), _lib.ptr(bulk), _lib.ptr(eta), _lib.ptr(c), kap.size, _lib.ptr(kap),
                                     _lib.ptr(slo), int(accept), _lib.ptr(s), _lib.ptr(ds), _lib.ptr(ind), _lib.ptr(counts)),
                   entry)
    else:
        _lib.check(getattr(l, entry)(dev, n_int, _lib.ptr(ev), ps, cs, _lib.ptr(e0v), _lib.ptr(ep_dev),
                                     _lib.ptr(shear), _lib.ptr(bulk), _lib.ptr(eta), _lib.ptr(c), int(accept),
                                     _lib.ptr(s), _lib.ptr(ds), _lib.ptr(ind), _lib.ptr(counts)), entry)
    n_smooth, n_apex = int(counts[0]), int(counts[1])
    out = _Result({'s': s, 'ds': ds, 'ind_p': ind.view(np.bool_), 'n_smooth': n_smooth, 'n_apex': n_apex})
    early_out = tsx and n_smooth == 0 and n_apex == 0                  # TSX:1103
    # C2: lambda_final is None in DP always, in TSX whenever a point is plastic
    out['lambda_final'] = np.zeros((1, n_int)) if early_out else None
    if apply_plastic_strain and not early_out:
        if ep_prev is None:
            raise TypeError('apply_plastic_strain needs ep_prev (the reference fails at DP:752 too)')
        if ep_dev is not ep_prev:
            ep_prev[...] = ep_dev                                      # C4: caller's array is mutated
        out['ep'] = ep_prev                                            # and returned as 'ep' (DP:751)
    else:
        out.lazy_zeros('ep', (4, n_int))                               # DP:749: zeros nobody reads on a Newton iterate
    return out


class _Result(dict):
    """The reference's result dict.  A non-accepting call returns 'ep' = zeros((4, n_int)) (DP:749) that the Newton
    iterates never look at; the 32 MB array is created when the key is first touched (any read access to the dict
    that could see it materialises it first), so that the per-iterate call does not pay for it."""
    __slots__ = ('_lazy',)

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._lazy = {}

    def lazy_zeros(self, key, shape):
        self._lazy[key] = shape

    def _fill(self):
        if self._lazy:
            for k, shape in self._lazy.items():
                super().__setitem__(k, np.zeros(shape))
            self._lazy = {}

    def __missing__(self, key):
        if key in self._lazy:
            self._fill()
            return super().__getitem__(key)
        raise KeyError(key)

    def __setitem__(self, key, value):
        self._lazy.pop(key, None)
        super().__setitem__(key, value)

    def __contains__(self, key):
        return key in self._lazy or super().__contains__(key)

    def get(self, key, default=None):
        self._fill()
        return super().get(key, default)

    def keys(self):
        self._fill()
        return super().keys()

    def items(self):
        self._fill()
        return super().items()

    def values(self):
        self._fill()
        return super().values()

    def __iter__(self):
        self._fill()
        return super().__iter__()

    def __len__(self):
        self._fill()
        return super().__len__()

    def __repr__(self):
        self._fill()
        return super().__repr__()

    def copy(self):
        self._fill()
        return dict(self)


def construct_constitutive_problem(e, ep_prev, shear, bulk, eta, c, apply_plastic_strain=False, device=None):
    """Drop-in for Plasticity2D_DP/pythonFEM.py:604-757 (same positional signature).

    Returns the reference's dict {'s','ds','ind_p','lambda_final','ep'} (+ 'n_smooth',
    'n_apex', the counts the reference logs at DP:730).  `e` is not modified; when
    `apply_plastic_strain` is true `ep_prev` is updated in place and returned as 'ep'.
    """
    return _return_map(e, None, ep_prev, shear, bulk, eta, c, apply_plastic_strain, tsx=False, device=device)


def construct_constitutive_problem_tsx(e, e0, ep_prev, shear, bulk, eta, c, apply_plastic_strain=False, device=None):
    """Drop-in for tsx-tunnel/pythonFEM.py:990-1157: adds the initial strain `e0` (4,1) and the
    all-elastic early-out (zeros for 'lambda_final' and 'ep')."""
    return _return_map(e, e0, ep_prev, shear, bulk, eta, c, apply_plastic_strain, tsx=True, device=device)


def construct_constitutive_problem_vm(e, ep_prev, shear, bulk, a, Y, apply_plastic_strain=False, e0=None, device=None):
    """The second material model, no counterpart in the reference: von Mises plasticity with linear kinematic hardening
    (include/fep.h, fep_return_map_vm_host).  `a` the hardening modulus, `Y` = sqrt(2/3) sigma_y the yield radius, per point;
    the other arguments as construct_constitutive_problem, `e0` an optional (4,1) initial strain.  Returns
    {'s', 'ds', 'ind_p', 'ep', 'n_plast'}; with `apply_plastic_strain`, `ep_prev` is updated in place and returned as 'ep'."""
    r = _return_map(e, e0, ep_prev, shear, bulk, a, Y, apply_plastic_strain, tsx=False, device=device,
                    entry='fep_return_map_vm_host')
    return {'s': r['s'], 'ds': r['ds'], 'ind_p': r['ind_p'], 'ep': r['ep'], 'n_plast': r['n_smooth']}


def construct_constitutive_problem_mc(e, ep_prev, shear, bulk, sin_phi, c, apply_plastic_strain=False, e0=None, device=None):
    """The third material model, no counterpart in the reference: associative, perfectly plastic Mohr-Coulomb, the return
    map in principal stresses with its spectral tangent (include/fep.h, fep_return_map_mc_host).  `sin_phi` in (0, 1) the
    sine of the friction angle, `c` > 0 the cohesion, per point; the other arguments as construct_constitutive_problem,
    `e0` an optional (4,1) initial strain.  Returns {'s', 'ds', 'ind_p', 'ep', 'n_smooth', 'n_apex'}: 'n_smooth' counts the
    points on the smooth face and on the two edges, 'n_apex' those at the apex; with `apply_plastic_strain`, `ep_prev` is
    updated in place and returned as 'ep'."""
    r = _return_map(e, e0, ep_prev, shear, bulk, sin_phi, c, apply_plastic_strain, tsx=False, device=device,
                    entry='fep_return_map_mc_host')
    return {k: r[k] for k in ('s', 'ds', 'ind_p', 'ep', 'n_smooth', 'n_apex')}


def construct_constitutive_problem_vmps(e, ep_prev, shear, bulk, a, Y, apply_plastic_strain=False, e0=None, device=None):
    """The fourth material model, no counterpart in the reference: von Mises plasticity with linear kinematic hardening in
    plane stress (include/fep.h, fep_return_map_vmps_host): the law of construct_constitutive_problem_vm with s33 = 0 and
    the out-of-plane strain free, the multiplier by a bounded Newton iteration per point.  Arguments and the returned
    {'s' (row 3 = 0), 'ds', 'ind_p', 'ep', 'n_plast'} as construct_constitutive_problem_vm; row 3 of `e0` and `ep_prev`
    does not enter (a non-finite value in it makes the point elastic with a NaN in 's'), and on accept row 3 of 'ep' takes
    minus the sum of the in-plane normal increments."""
    r = _return_map(e, e0, ep_prev, shear, bulk, a, Y, apply_plastic_strain, tsx=False, device=device,
                    entry='fep_return_map_vmps_host')
    return {'s': r['s'], 'ds': r['ds'], 'ind_p': r['ind_p'], 'ep': r['ep'], 'n_plast': r['n_smooth']}


def construct_constitutive_problem_vmi(e, ep_prev, shear, bulk, a, Y, curve, apply_plastic_strain=False, e0=None, device=None):
    """The fifth material model, no counterpart in the reference: von Mises plasticity with isotropic hardening on a
    piecewise-linear curve next to the linear kinematic one (include/fep.h, fep_return_map_vmi_host).  `curve` = (kappa, slope),
    1 .. 8 segments (hardening.hardening_curve / voce_curve build one from a uniaxial table), the same for every point; `Y` is
    the INITIAL yield radius and the current one is Y + R(kappa).  The rows of `ep_prev` are (p11, p22, gamma12, kappa): p33 =
    -(p11 + p22) is implied and row 3 holds the accumulated plastic multiplier (equivalent plastic strain sqrt(2/3) kappa).
    The other arguments and the returned {'s', 'ds', 'ind_p', 'ep', 'n_plast'} as construct_constitutive_problem_vm.  A curve
    that breaks the law's preconditions for these materials (hardening.check_curve) is refused with ValueError."""
    curve = check_curve(*curve, shear=shear, a=a, Y=Y)
    r = _return_map(e, e0, ep_prev, shear, bulk, a, Y, apply_plastic_strain, tsx=False, device=device,
                    entry='fep_return_map_vmi_host', curve=curve)
    return {'s': r['s'], 'ds': r['ds'], 'ind_p': r['ind_p'], 'ep': r['ep'], 'n_plast': r['n_smooth']}


# FEP_MODEL_DP, FEP_MODEL_VM, FEP_MODEL_MC, FEP_MODEL_VMPS, FEP_MODEL_VMI (4 is not a model)
MODELS = {'dp': 0, 'vm': 1, 'mc': 2, 'vmps': 3, 'vmi': 5}


def construct_constitutive_problem_field(model, e, e0_field, ep_prev, shear, bulk, m3, m4, apply_plastic_strain=False,
                                         e0=None, e0_scale=1.0, device=None):
    """The return map of `model` ('dp', 'vm' or 'mc'; 'vmps' and 'vmi' take a field in `MeshContext.step` only) with an initial strain per point, no counterpart in the reference
    (include/fep.h, fep_return_map_field_host): point k runs on `e0 + e0_scale * e0_field[:, k]`, `e0_field` (4, n_int) with
    rows 11, 22, 12 (engineering shear), 33, `e0` an optional uniform (4,1) part.  `m3`, `m4` are the model's third and
    fourth parameter arrays (eta, c / a, Y / sin_phi, c); the other arguments as construct_constitutive_problem.  Returns
    {'s', 'ds', 'ind_p', 'ep', 'n_smooth', 'n_apex'} with the counts as the model's own wrapper reports them (von Mises:
    its plastic points in 'n_smooth'); with `apply_plastic_strain`, `ep_prev` is updated in place and returned as 'ep'."""
    if model not in ('dp', 'vm', 'mc'):
        raise ValueError("model must be one of ['dp', 'mc', 'vm']")
    if e0_field is None:
        raise ValueError('e0_field is required (the plain wrappers run without a field)')
    r = _return_map(e, e0, ep_prev, shear, bulk, m3, m4, apply_plastic_strain, tsx=False, device=device,
                    field=(model, e0_field, e0_scale))
    return {k: r[k] for k in ('s', 'ds', 'ind_p', 'ep', 'n_smooth', 'n_apex')}


def in_situ_strain(s0, shear, bulk):
    """The strain whose elastic stress is `s0` ((4, n) rows 11, 22, 12, 33; `shear`, `bulk` scalars or (n,)): per point
    e = dev(s0) / (2G) + tr(s0) / (9K) on the normal components and s12 / G for the engineering shear.  NumPy arrays in,
    NumPy array out; torch tensors in, a tensor on their device out (elementwise: no kernel of its own)."""
    if type(s0).__module__.split('.')[0] == 'torch':
        import torch
        G = torch.as_tensor(shear, dtype=s0.dtype, device=s0.device).reshape(-1)
        K = torch.as_tensor(bulk, dtype=s0.dtype, device=s0.device).reshape(-1)
        m = (s0[0] + s0[1] + s0[3]) / 3
        return torch.stack([(s0[0] - m) / (2 * G) + m / (3 * K), (s0[1] - m) / (2 * G) + m / (3 * K), s0[2] / G,
                            (s0[3] - m) / (2 * G) + m / (3 * K)])
    s0 = np.asarray(s0, dtype=np.float64)
    G = np.asarray(shear, dtype=np.float64).reshape(-1)
    K = np.asarray(bulk, dtype=np.float64).reshape(-1)
    m = (s0[0] + s0[1] + s0[3]) / 3
    return np.stack([(s0[0] - m) / (2 * G) + m / (3 * K), (s0[1] - m) / (2 * G) + m / (3 * K), s0[2] / G,
                     (s0[3] - m) / (2 * G) + m / (3 * K)])


def linear_in_situ(s0_ref, y_ref, grad):
    """The callable (x, y) -> s0_ref + grad * (y - y_ref), a (4, n) stress with rows 11, 22, 12, 33: an in-situ state that
    grows linearly with depth (`s0_ref` at the height `y_ref`, `grad` its change per unit of y; scalars or 4 values each).
    Works on NumPy arrays and on torch tensors alike."""
    a = [float(v) for v in np.broadcast_to(np.asarray(s0_ref, dtype=np.float64).ravel(), (4,))]
    g = [float(v) for v in np.broadcast_to(np.asarray(grad, dtype=np.float64).ravel(), (4,))]
    y0 = float(y_ref)

    def s0(x, y):
        rows = [a[i] + g[i] * (y - y0) for i in range(4)]
        if type(y).__module__.split('.')[0] == 'torch':
            import torch
            return torch.stack(rows)
        return np.stack(rows)
    return s0


# ---------------------------------------------------------------------------------------
# mesh context: static operands + fused step
# ---------------------------------------------------------------------------------------
class MeshContext:
    """Owns the device-resident static operands of one mesh (element table, dphi, weights,
    materials, CSR pattern and gather lists) — what `get_elastic_stiffness_matrix` computes once
    in the reference (DP:977) — and runs the fused hot path on them."""

    def __init__(self, elements, coordinates, dhatp1=None, dhatp2=None, wf=None, element_type=None, device=None):
        l = _lib.lib()
        elements = np.asarray(elements)
        n_p, n_e = elements.shape
        t = _coerce(element_type) if element_type is not None else _NP_TO_TYPE[n_p]
        if ELEMENT_SHAPE[t][0] != n_p:
            raise ValueError(f'{t} needs {ELEMENT_SHAPE[t][0]} nodes per element, got {n_p}')
        n_q = ELEMENT_SHAPE[t][1]
        if dhatp1 is None:
            dhatp1, dhatp2, wf = element_tables(t)
        d1 = np.ascontiguousarray(np.broadcast_to(np.asarray(dhatp1, dtype=np.float64), (n_p, n_q)))
        d2 = np.ascontiguousarray(np.broadcast_to(np.asarray(dhatp2, dtype=np.float64), (n_p, n_q)))
        w = _f64(wf).ravel()
        if w.size != n_q:
            raise ValueError(f'{t} needs {n_q} weight factors')
        coordinates = _f64(coordinates)
        n_n = coordinates.shape[1]
        if elements.size and (elements.min() < 0 or elements.max() >= n_n):
            raise IndexError('element node ids must be 0-based and < n_n')
        el32 = np.ascontiguousarray(elements, dtype=np.int32)
        self.device = default_device() if device is None else device
        self.element_type = t
        self._h = C.c_void_p()
        _lib.check(l.fep_ctx_create(C.byref(self._h), self.device, t.value, n_e, n_n, _lib.ptr(el32),
                                    _lib.ptr(coordinates), _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(w)), 'fep_ctx_create')
        sz = (C.c_int64 * 8)()
        _lib.check(l.fep_ctx_sizes(self._h, sz), 'fep_ctx_sizes')
        (self.n_e, self.n_n, self.n_p, self.n_q, self.n_int, self.n_dof, self.nnz, self.n_blk) = [int(v) for v in sz]
        self.elements = el32
        self._pattern = None
        self._geom = None
        self._hatp_own = None
        self.model = 'dp'
        self._hardening = (np.zeros(1), np.zeros(1))       # fep_ctx_set_hardening's default: one segment of slope 0
        self._mats = None                                   # (shear, bulk, third, fourth) of the last set_materials

    # -- lifetime
    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            _lib.lib().fep_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- static data
    def geometry(self):
        """(dphi_1, dphi_2, weight, det): (n_p,n_int), (n_p,n_int), (1,n_int), (n_int,)  DP:530-546,585"""
        if self._geom is None:
            d1 = np.empty((self.n_p, self.n_int))
            d2 = np.empty((self.n_p, self.n_int))
            w = np.empty((1, self.n_int))
            det = np.empty(self.n_int)
            _lib.check(_lib.lib().fep_ctx_geometry_host(self._h, _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(w), _lib.ptr(det)),
                       'fep_ctx_geometry_host')
            self._geom = (d1, d2, w, det)
        return self._geom

    def pattern(self):
        """CSR pattern of K on DOFs: (indptr int32 (n_dof+1), indices int32 (nnz)), sorted columns."""
        if self._pattern is None:
            ip = np.empty(self.n_dof + 1, dtype=np.int32)
            ix = np.empty(self.nnz, dtype=np.int32)
            _lib.check(_lib.lib().fep_ctx_pattern_host(self._h, _lib.ptr(ip), _lib.ptr(ix)), 'fep_ctx_pattern_host')
            self._pattern = (ip, ix)
        return self._pattern

    def kernel_names(self, which=0):
        """The kernels one step launches, named as rocprofv3 prints them, joined by ' + ' (which = 0: every output,
        1: the K,F-only step of a Newton iterate)."""
        import ctypes
        buf = ctypes.create_string_buffer(512)
        _lib.check(_lib.lib().fep_ctx_kernel_names(self._h, int(which), buf, 512), 'fep_ctx_kernel_names')
        return buf.value.decode()

    def csr(self, data):
        ip, ix = self.pattern()
        return ssp.csr_matrix((data, ix, ip), shape=(self.n_dof, self.n_dof))

    def set_materials(self, shear, bulk, eta, c):
        a = [_f64(np.broadcast_to(np.asarray(v, dtype=np.float64).ravel(), (self.n_int,))) for v in (shear, bulk, eta, c)]
        if self.model == 'vmi':
            check_curve(*self._hardening, shear=a[0], a=a[2], Y=a[3])
        _lib.check(_lib.lib().fep_ctx_set_materials_host(self._h, *[_lib.ptr(v) for v in a]), 'fep_ctx_set_materials_host')
        self._mats = a

    def set_model(self, model):
        """'dp' (Drucker-Prager, the default), 'vm' (von Mises with linear kinematic hardening: `set_materials` then takes
        (shear, bulk, a, Y), the results carry the plastic count in 'n_smooth' and 'n_apex' is 0) or 'mc' (Mohr-Coulomb:
        `set_materials` takes (shear, bulk, sin_phi, c), 'n_smooth' counts face and edges, 'n_apex' the apex) or 'vmps' (von
        Mises in plane stress: everything as 'vm', the stress has s33 = 0, and the context's K at U = 0 is the elastic
        plane-stress stiffness) or 'vmi' (von Mises with isotropic hardening on the curve of `set_hardening` next to the
        kinematic one: materials as 'vm' with Y the initial yield radius, row 3 of the plastic strain is kappa).  Before or
        after `set_materials`."""
        if model not in MODELS:
            raise ValueError(f"model must be one of {sorted(MODELS)}")
        _lib.check(_lib.lib().fep_ctx_set_model(self._h, MODELS[model]), 'fep_ctx_set_model')
        self.model = model

    def set_hardening(self, kappa, slope):
        """The hardening curve of a 'vmi' context (fep_ctx_set_hardening): breakpoints `kappa` (kappa[0] = 0, increasing) and
        one slope dR/dkappa per segment, 1 .. 8 segments, the last running to infinity; before or after `set_materials`.
        Without a call the context holds one segment of slope 0.  ValueError for a curve that is not as stated or, once the
        materials are known, breaks the law's preconditions (hardening.check_curve); FepError (FEP_ESTATE) on a context of
        another model.  A refused call changes nothing."""
        if self.model == 'vmi' and self._mats is not None:
            curve = check_curve(kappa, slope, shear=self._mats[0], a=self._mats[2], Y=self._mats[3])
        else:
            curve = check_curve(kappa, slope)
        _lib.check(_lib.lib().fep_ctx_set_hardening(self._h, curve[0].size, _lib.ptr(curve[0]), _lib.ptr(curve[1])),
                   'fep_ctx_set_hardening')
        self._hardening = curve

    @property
    def hardening(self):
        """(kappa, slope) of a 'vmi' context's curve (copies); None on a context of another model."""
        return (self._hardening[0].copy(), self._hardening[1].copy()) if self.model == 'vmi' else None

    def device_ptr(self, which):
        p = C.c_void_p()
        _lib.check(_lib.lib().fep_ctx_device_ptr(self._h, which, C.byref(p)), 'fep_ctx_device_ptr')
        return p.value

    # -- hot path on host arrays
    def step(self, U, ep_prev=None, e0=None, apply_plastic_strain=False, want=('s', 'ds', 'ind_p', 'K', 'F'),
             e0_field=None, e0_scale=1.0):
        """One pass strain -> return map -> tangent -> internal force (DP:1043-1058) for the
        displacement `U` ((2,n_n), or flat DOF order).  Returns a dict with the requested keys among
        'E' (3,n_int), 's' (4,n_int), 'ds' (9,n_int), 'ind_p', 'K' (csr), 'F' (n_dof,), plus
        'n_smooth', 'n_apex'.  `ep_prev` (4,n_int) is updated in place on accept.  `e0_field` (4,n_int): an initial strain
        per integration point, point k running on `e0 + e0_scale * e0_field[:, k]` (fep_step_field_host)."""
        U = np.asarray(U, dtype=np.float64)
        if U.size != self.n_dof:
            raise ValueError(f'U must hold {self.n_dof} values')
        fld = None
        if e0_field is not None:
            fld = _f64(e0_field)
            if fld.shape != (4, self.n_int):
                raise ValueError(f'e0_field must be (4,{self.n_int}), got {fld.shape}')
        # the reference's (2, n_n) array goes down as it is: the library interleaves it while staging the transfer
        # (a NumPy `reshape(-1, order='F')` of 1 M nodes costs 2.5 ms, as much as the whole transfer)
        planar = fld is None and U.ndim == 2 and U.shape[0] == 2 and U.flags.c_contiguous
        u = U if planar else np.ascontiguousarray(U.reshape(-1, order='F') if U.ndim == 2 else U)
        n = self.n_int
        e0v = None if e0 is None else _f64(e0).ravel()
        ep = None
        if ep_prev is not None:
            ok = (ep_prev.dtype == np.float64 and ep_prev.flags.c_contiguous and ep_prev.shape == (4, n))
            ep = ep_prev if ok else _f64(ep_prev, (4, n)).copy()
        out = {}
        E = _lib.pinned_empty((3, n)) if 'E' in want else None          # page-locked: results are DMA-ed straight into them
        s = _lib.pinned_empty((4, n)) if 's' in want else None
        ds = _lib.pinned_empty((9, n)) if 'ds' in want else None
        ind = _lib.pinned_empty(n, np.uint8) if 'ind_p' in want else None
        kd = _lib.pinned_empty(self.nnz) if 'K' in want else None
        F = _lib.pinned_empty(self.n_dof) if 'F' in want else None
        counts = np.zeros(2, dtype=np.int64)
        accept = bool(apply_plastic_strain) and ep is not None
        if fld is not None:
            _lib.check(_lib.lib().fep_step_field_host(self._h, _lib.ptr(u), _lib.ptr(e0v), _lib.ptr(fld), float(e0_scale),
                                                      _lib.ptr(ep), int(accept), _lib.ptr(E), _lib.ptr(s), _lib.ptr(ds),
                                                      _lib.ptr(ind), _lib.ptr(kd), _lib.ptr(F), _lib.ptr(counts)),
                       'fep_step_field_host')
        else:
            fn = _lib.lib().fep_step_host_planar if planar else _lib.lib().fep_step_host
            _lib.check(fn(self._h, _lib.ptr(u), _lib.ptr(e0v), _lib.ptr(ep), int(accept), _lib.ptr(E), _lib.ptr(s),
                          _lib.ptr(ds), _lib.ptr(ind), _lib.ptr(kd), _lib.ptr(F), _lib.ptr(counts)), 'fep_step_host')
        if accept and ep is not ep_prev:
            ep_prev[...] = ep
        for k, v in (('E', E), ('s', s), ('ds', ds), ('F', F)):
            if v is not None:
                out[k] = v
        if ind is not None:
            out['ind_p'] = ind.view(np.bool_)
        if kd is not None:
            out['K'] = self.csr(kd)
        out['n_smooth'], out['n_apex'] = int(counts[0]), int(counts[1])
        return out

    def assemble(self, ds=None, s=None):
        """K = B^T blockdiag(w*ds) B and F = B^T (w*s[0:3]) from given point data (DP:1047-1058).
        Returns (K csr or None, F or None).  `ds` must be symmetric per point: only its upper triangle (rows 0, 1, 2, 4,
        5, 8) is read (include/fep.h, fep_assemble_host)."""
        n = self.n_int
        dsv = None if ds is None else _f64(ds, (9, n))
        sv = None if s is None else _f64(np.asarray(s)[0:3], (3, n))
        kd = _lib.pinned_empty(self.nnz) if ds is not None else None
        F = _lib.pinned_empty(self.n_dof) if s is not None else None
        _lib.check(_lib.lib().fep_assemble_host(self._h, _lib.ptr(dsv), _lib.ptr(sv), _lib.ptr(kd), _lib.ptr(F)),
                   'fep_assemble_host')
        return (None if kd is None else self.csr(kd)), F

    # -- hot path on device-resident arrays (raw device pointers as ints; used by bench.py / torch)
    def step_dev(self, stream, u, ep=0, accept=False, e0=None, e_out=0, s=0, ds=0, ind_p=0, k_data=0, f_out=0, counts=0,
                 e0_field=None, e0_scale=1.0):
        """`e0_field`: device pointer (int) of a (4, n_int) initial-strain field, or None (fep_step_field_dev / fep_step_dev)."""
        e0v = None if e0 is None else _f64(e0).ravel()
        if e0_field is not None:
            _lib.check(_lib.lib().fep_step_field_dev(self._h, stream, u, _lib.ptr(e0v), e0_field or None, float(e0_scale),
                                                     ep or None, int(bool(accept)), e_out or None, s or None, ds or None,
                                                     ind_p or None, k_data or None, f_out or None, counts or None),
                       'fep_step_field_dev')
            return
        _lib.check(_lib.lib().fep_step_dev(self._h, stream, u, _lib.ptr(e0v), ep or None, int(bool(accept)), e_out or None,
                                           s or None, ds or None, ind_p or None, k_data or None, f_out or None,
                                           counts or None), 'fep_step_dev')

    def assemble_dev(self, stream, ds=0, s=0, k_data=0, f_out=0):
        _lib.check(_lib.lib().fep_assemble_dev(self._h, stream, ds or None, s or None, k_data or None, f_out or None),
                   'fep_assemble_dev')

    def transform(self, q_int):
        """Nodal values of an integration-point field (DP:760-816) -> (n_n,) ndarray."""
        q = _f64(q_int).ravel()
        if q.size != self.n_int:
            raise ValueError(f'q_int must hold {self.n_int} values')
        out = np.empty(self.n_n)
        _lib.check(_lib.lib().fep_transform_host(self._h, _lib.ptr(q), _lib.ptr(out)), 'fep_transform_host')
        return out

    def transform_dev(self, stream, q_int, q_node):
        _lib.check(_lib.lib().fep_transform_dev(self._h, stream, q_int, q_node), 'fep_transform_dev')

    # -- recovered-stress error indicator (include/fep.h; the NumPy twin is estimate.py)
    def recover_stress(self, s):
        """Recovered nodal stress of the point stress `s` (4, n_int) -> (4, n_n) ndarray (fep_recover_stress_host)."""
        sv = _f64(s, (4, self.n_int))
        out = np.empty((4, self.n_n))
        _lib.check(_lib.lib().fep_recover_stress_host(self._h, _lib.ptr(sv), _lib.ptr(out)), 'fep_recover_stress_host')
        return out

    def estimate(self, s, hatp=None):
        """The indicator of the point stress `s` (4, n_int): {'eta2' (n_e,), 'total' (their fixed-order sum), 'max',
        'n_nonfinite', 's_node' (4, n_n)} (fep_recover_stress_host, fep_estimate_host).  `hatp` as in load_volume."""
        sv = _f64(s, (4, self.n_int))
        sn = self.recover_stress(sv)
        eta2, stats = np.empty(self.n_e), np.empty(4)
        _lib.check(_lib.lib().fep_estimate_host(self._h, _lib.ptr(self._hatp(hatp)), _lib.ptr(sv), _lib.ptr(sn), _lib.ptr(eta2),
                                                _lib.ptr(stats)), 'fep_estimate_host')
        return {'eta2': eta2, 'total': float(stats[0]), 'max': float(stats[1]), 'n_nonfinite': int(stats[2]), 's_node': sn}

    def _torch_stream(self):
        import torch
        return torch, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def recover_stress_dev(self, s, out=None):
        """The same on a float64 torch tensor `s` (4, n_int) of the context's GPU, on the current stream -> a (4, n_n) tensor
        (`out`, or a new one).  Only enqueues one kernel."""
        torch, stream = self._torch_stream()
        if s.dtype != torch.float64 or tuple(s.shape) != (4, self.n_int) or not s.is_contiguous():
            raise ValueError(f's must be a contiguous float64 tensor of (4, {self.n_int})')
        if out is None:
            out = torch.empty((4, self.n_n), dtype=torch.float64, device=s.device)
        _lib.check(_lib.lib().fep_recover_stress_dev(self._h, stream, C.c_void_p(s.data_ptr()), C.c_void_p(out.data_ptr())),
                   'fep_recover_stress_dev')
        return out

    def estimate_dev(self, s, s_node=None, hatp=None, stats=True):
        """Device-resident indicator of the tensor `s` (4, n_int) -> (eta2 (n_e,), stats (4,) = [total, max, n_nonfinite, n_e]
        or None, s_node (4, n_n)), float64 tensors written on the current stream; nothing is read back or synchronised.
        `s_node`: the recovered stress if the caller already has it."""
        torch, stream = self._torch_stream()
        if s_node is None:
            s_node = self.recover_stress_dev(s)
        elif s_node.dtype != torch.float64 or tuple(s_node.shape) != (4, self.n_n) or not s_node.is_contiguous():
            raise ValueError(f's_node must be a contiguous float64 tensor of (4, {self.n_n})')
        if s.dtype != torch.float64 or tuple(s.shape) != (4, self.n_int) or not s.is_contiguous():
            raise ValueError(f's must be a contiguous float64 tensor of (4, {self.n_int})')
        eta2 = torch.empty(self.n_e, dtype=torch.float64, device=s.device)
        st = torch.empty(4, dtype=torch.float64, device=s.device) if stats else None
        _lib.check(_lib.lib().fep_estimate_dev(self._h, stream, _lib.ptr(self._hatp(hatp)), C.c_void_p(s.data_ptr()),
                                               C.c_void_p(s_node.data_ptr()), C.c_void_p(eta2.data_ptr()),
                                               None if st is None else C.c_void_p(st.data_ptr())), 'fep_estimate_dev')
        return eta2, st, s_node

    # -- external loads (EL:246-292)
    def _hatp(self, hatp):
        if hatp is None:
            if self._hatp_own is None:                                       # the library's table, evaluated once
                own = get_local_basis_volume(self.element_type, get_quadrature_volume(self.element_type)[0])[0]
                self._hatp_own = np.ascontiguousarray(np.broadcast_to(np.asarray(own, dtype=np.float64), (self.n_p, self.n_q)))
            return self._hatp_own
        return np.ascontiguousarray(np.broadcast_to(np.asarray(hatp, dtype=np.float64), (self.n_p, self.n_q)))

    def point_coords(self, hatp=None):
        """Coordinates of the integration points -> (2, n_int) ndarray: what an `e0_field` is evaluated at
        (fep_ctx_point_coords_host).  `hatp` as in load_volume."""
        out = np.empty((2, self.n_int))
        _lib.check(_lib.lib().fep_ctx_point_coords_host(self._h, _lib.ptr(self._hatp(hatp)), _lib.ptr(out)),
                   'fep_ctx_point_coords_host')
        return out

    def point_coords_dev(self, stream, xq, hatp=None):
        """The same into the device pointer `xq` (2, n_int).  Only enqueues one kernel."""
        _lib.check(_lib.lib().fep_ctx_point_coords_dev(self._h, stream, _lib.ptr(self._hatp(hatp)), xq),
                   'fep_ctx_point_coords_dev')

    def load_volume(self, f_v_int=None, uniform=None, hatp=None, weight=None):
        """Body-force vector (EL:246-292) -> (2, n_n) ndarray.  Either `f_v_int` (2, n_int), a value per integration
        point, or `uniform` = (fx, fy), the same force everywhere (self-weight) without a field in memory.  `hatp`: the
        (n_p, n_q) basis-function values, default the library's table of the context's element type; `weight`: (n_int),
        default the context's own."""
        if (f_v_int is None) == (uniform is None):
            raise ValueError('give exactly one of f_v_int and uniform')
        h = self._hatp(hatp)
        f = None if f_v_int is None else _f64(f_v_int, (2, self.n_int))
        fx, fy = (0.0, 0.0) if uniform is None else (float(uniform[0]), float(uniform[1]))
        w = None if weight is None else _f64(weight).ravel()
        if w is not None and w.size != self.n_int:
            raise ValueError(f'weight must hold {self.n_int} values')
        out = np.empty(self.n_dof)
        _lib.check(_lib.lib().fep_load_volume_host(self._h, _lib.ptr(h), _lib.ptr(f), fx, fy, _lib.ptr(w), _lib.ptr(out)),
                   'fep_load_volume_host')
        return np.ascontiguousarray(out.reshape(self.n_n, 2).T)

    def load_volume_dev(self, stream, f_out, f_v_int=0, uniform=None, hatp=None, weight=0):
        """The same on device pointers (ints): `f_out` (n_dof) interleaved like F of step_dev, `f_v_int` (2, n_int) planar or
        0 with `uniform` = (fx, fy).  Only enqueues one kernel: capturable in a graph."""
        if bool(f_v_int) == (uniform is not None):
            raise ValueError('give exactly one of f_v_int and uniform')
        fx, fy = (0.0, 0.0) if uniform is None else (float(uniform[0]), float(uniform[1]))
        _lib.check(_lib.lib().fep_load_volume_dev(self._h, stream, _lib.ptr(self._hatp(hatp)), f_v_int or None, fx, fy,
                                                  weight or None, f_out), 'fep_load_volume_dev')

    def profile_begin(self):
        """Start bracketing every kernel of the following step_dev/assemble_dev calls with HIP events."""
        _lib.check(_lib.lib().fep_ctx_profile_begin(self._h), 'fep_ctx_profile_begin')

    def profile_end(self, stream):
        """-> ({'element': ms, 'csr': ms, 'force': ms} average per launch, n_steps)."""
        ms = (C.c_double * 3)()
        n = C.c_int()
        _lib.check(_lib.lib().fep_ctx_profile_end(self._h, stream, ms, C.byref(n)), 'fep_ctx_profile_end')
        return {'element': ms[0], 'csr': ms[1], 'force': ms[2]}, n.value


# ---------------------------------------------------------------------------------------
# a6  get_elastic_stiffness_matrix
# ---------------------------------------------------------------------------------------
def _strain_displacement_csr(ctx):
    """B (3 n_int x 2 n_n) in canonical CSR exactly as SciPy builds it from the reference's
    triplets (DP:549-571): 6 n_p stored entries per point incl. explicit zeros, sorted columns."""
    d1, d2, _, _ = ctx.geometry()
    n_p, n_q, n_e, n_int = ctx.n_p, ctx.n_q, ctx.n_e, ctx.n_int
    order = np.argsort(ctx.elements, axis=0, kind='stable')                 # columns sorted by node id
    nodes = np.take_along_axis(ctx.elements, order, axis=0).astype(np.int32)
    ordk = np.repeat(order, n_q, axis=1)                                    # (n_p, n_int)
    g1 = np.take_along_axis(d1, ordk, axis=0).T                             # (n_int, n_p)
    g2 = np.take_along_axis(d2, ordk, axis=0).T
    data = np.zeros((n_int, 3, n_p, 2))
    data[:, 0, :, 0] = g1
    data[:, 1, :, 1] = g2
    data[:, 2, :, 0] = g2
    data[:, 2, :, 1] = g1
    cols_e = np.empty((n_e, n_p, 2), dtype=np.int32)
    cols_e[:, :, 0] = 2 * nodes.T
    cols_e[:, :, 1] = 2 * nodes.T + 1
    cols = np.broadcast_to(cols_e[:, None, None, :, :], (n_e, n_q, 3, n_p, 2))
    indptr = np.arange(0, 3 * n_int + 1, dtype=np.int64) * (2 * n_p)
    if indptr[-1] < 2 ** 31:
        indptr = indptr.astype(np.int32)
    return ssp.csr_matrix((data.ravel(), np.ascontiguousarray(cols).ravel(), indptr), shape=(3 * n_int, 2 * ctx.n_n))


def _elastic_D_csr(weight, shear, bulk):
    """D (DP:579-592): block-diagonal elastic tensor times weight, all 9 entries per point stored."""
    n_int = weight.size
    iota = np.array([[1], [1], [0]])
    vol = iota * iota.T
    dev = np.diag([1, 1, 0.5]) - vol / 3
    elast = 2 * dev.reshape((-1, 1)) * shear + vol.reshape((-1, 1)) * bulk      # symmetric: row- = column-major
    vd = elast * (np.ones((9, 1)) * weight.reshape(1, -1))
    base = 3 * np.arange(n_int, dtype=np.int64)
    idx = (base[:, None, None] + np.arange(3)[None, None, :]) + np.zeros((1, 3, 1), dtype=np.int64)
    indptr = 3 * np.arange(3 * n_int + 1, dtype=np.int64)
    return ssp.csr_matrix((vd.T.ravel(), idx.ravel(), indptr), shape=(3 * n_int, 3 * n_int))


def get_elastic_stiffness_matrix(elements, coordinates, shear, bulk, dhatp1, dhatp2, wf, device=None):
    """Drop-in for DP:491-601 / TSX:432-542: returns (K, B, weight, id, jd, D).

    Geometry (Jacobians, dphi, weight) and K_elast = B^T D B are computed on the GPU; `B`, `D`,
    `id`, `jd` are index/packaging work done on the host from the GPU's dphi/weight.  `K` is a CSR
    matrix on the full symbolic pattern (the reference's SciPy product drops numerically-zero
    entries).  The mesh context that produced them rides along as `K.fep_ctx` /
    `B.fep_ctx`; pass either to `assemble_tangent`."""
    ctx = MeshContext(elements, coordinates, dhatp1, dhatp2, wf, device=device)
    shear = _f64(shear).ravel()
    bulk = _f64(bulk).ravel()
    ctx.set_materials(shear, bulk, np.ones(ctx.n_int), np.ones(ctx.n_int))
    # elastic tangent everywhere <=> U = 0 (crit1 = -c < 0): K_elast is one pass of the hot path
    K = ctx.step(np.zeros(ctx.n_dof), want=('K',))['K']
    _, _, weight, _ = ctx.geometry()
    B = _strain_displacement_csr(ctx)
    D = _elastic_D_csr(weight, shear, bulk)
    aux = np.arange(3 * ctx.n_int).reshape((3, ctx.n_int), order='F') + 1      # DP:557
    iD = np.tile(aux, (3, 1))                                                  # DP:589
    jD = np.repeat(aux, 3, axis=0)                                             # DP:590
    K.fep_ctx = ctx
    B.fep_ctx = ctx
    _remember_context(weight, ctx)
    return K, B, weight, iD, jD, D


def get_elastic_stiffness_matrix_el(elements, coordinates, shear, bulk, dhatp1, dhatp2, wf, device=None):
    """Elasticity2D flavour (EL:368-477): `elements` is 1-based and is shifted IN PLACE (EL:389, C10);
    returns only (K, weight)."""
    elements -= 1
    K, _, weight, *_ = get_elastic_stiffness_matrix(elements, coordinates, shear, bulk, dhatp1, dhatp2, wf, device)
    return K, weight


# ---------------------------------------------------------------------------------------
# external loads: get_vector_volume (EL:246-292), get_vector_traction (EL:295-364)
# ---------------------------------------------------------------------------------------
# The reference's get_vector_volume receives `weight` but no handle of ours: the context that produced a weight array is
# found by the array's identity.  Both sides are held weakly (the context owns the array through its geometry cache, K and B
# own the context), so an entry lives exactly as long as the arrays the caller still holds.
_CTX_OF_WEIGHT = {}


def _remember_context(weight, ctx):
    key = id(weight)

    def forget(_, key=key):
        _CTX_OF_WEIGHT.pop(key, None)
    _CTX_OF_WEIGHT[key] = (weakref.ref(weight, forget), weakref.ref(ctx))


def _context_for(elements, n_n, weight):
    hit = _CTX_OF_WEIGHT.get(id(weight))
    if hit is None or hit[0]() is not weight:
        return None
    ctx = hit[1]()
    if ctx is None or not ctx._h or ctx.n_n != n_n or ctx.elements.shape != elements.shape \
            or not np.array_equal(ctx.elements, elements):
        return None
    return ctx


def _sparse_rows(dense, touched):
    """(2, n_n) csc_matrix with both rows stored for every touched node, zeros included: what the reference's sum of
    triplets yields (EL:289-290)."""
    cols = np.flatnonzero(touched)
    indptr = np.zeros(dense.shape[1] + 1, dtype=np.int32)
    indptr[1:] = 2 * np.cumsum(touched)
    return ssp.csc_matrix((dense[:, cols].T.ravel(), np.tile(np.array([0, 1], dtype=np.int32), cols.size), indptr),
                          shape=dense.shape)


def get_vector_volume(elements, coordinates, f_V_int, hatp, weight, device=None):
    """Drop-in for EL:246-292 / TSX:311-357: the body-force vector as a (2, n_n) csc_matrix.  `elements` 0-based (the
    reference's driver calls it after get_elastic_stiffness_matrix shifted them).  The sum runs on the GPU
    (fep_load_volume_host) with the caller's `hatp` and `weight`; the mesh context is the one whose
    get_elastic_stiffness_matrix* call returned this very `weight` array, else a new one built from `elements` /
    `coordinates` with the library's tables for the element type that `hatp.shape[0]` names."""
    elements = np.asarray(elements)
    coordinates = np.asarray(coordinates)
    n_n = coordinates.shape[1]
    ctx = _context_for(elements, n_n, weight)
    if ctx is None:
        ctx = MeshContext(elements, coordinates, device=device)
    f = ctx.load_volume(f_v_int=np.asarray(f_V_int, dtype=np.float64)[0:2], hatp=hatp, weight=weight)
    touched = np.zeros(n_n, dtype=bool)
    touched[elements.ravel()] = True
    return _sparse_rows(f, touched)


def load_traction(edges, coordinates, t_int, hatp_s, dhatp1_s, wf_s, device=None):
    """Surface-load vector over boundary edges -> (2, n_n) ndarray (fep_load_traction_host): `edges` (n_p_s, n_e_s) 0-based
    node ids (end, end[, middle]), `t_int` (2, n_e_s * n_q_s) a traction PER surface point, Jacobian = arc length, so
    edges of any direction are right."""
    coordinates = _f64(coordinates)
    n_n = coordinates.shape[1]
    ed = np.ascontiguousarray(edges, dtype=np.int32)
    n_p_s, n_e_s = ed.shape
    wf = _f64(wf_s).ravel()
    n_q_s = wf.size
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(hatp_s, dtype=np.float64), (n_p_s, n_q_s)))
    dh = np.ascontiguousarray(np.broadcast_to(np.asarray(dhatp1_s, dtype=np.float64), (n_p_s, n_q_s)))
    t = _f64(t_int, (2, n_e_s * n_q_s))
    out = np.empty(2 * n_n)
    dev = default_device() if device is None else device
    _lib.check(_lib.lib().fep_load_traction_host(dev, n_n, n_e_s, n_p_s, n_q_s, _lib.ptr(ed), _lib.ptr(coordinates),
                                                 _lib.ptr(h), _lib.ptr(dh), _lib.ptr(wf), _lib.ptr(t), _lib.ptr(out)),
               'fep_load_traction_host')
    return np.ascontiguousarray(out.reshape(n_n, 2).T)


def get_vector_traction(elements_s, coordinates, f_t_int, hatp_s, dhatp1_s, wf_s, device=None):
    """Drop-in for EL:295-364: (2, n_n) csc_matrix.  `elements_s` as the reference's `neumann_nodes` (0-based, float).
    The reference applies the LAST point's traction `f_t_int[:, -1]` at every point (EL:352-353): that quirk is kept here,
    by broadcasting, while the library honours a value per point (`load_traction`).  On the reference's horizontal edges
    its Jacobian |dx/dxi| and the library's arc length agree."""
    ed = np.asarray(elements_s).astype(np.int64)
    f_t_int = np.asarray(f_t_int, dtype=np.float64)
    n_pts = ed.shape[1] * np.asarray(wf_s).size
    t = np.repeat(f_t_int[0:2, -1:], n_pts, axis=1)
    f = load_traction(ed, coordinates, t, hatp_s, dhatp1_s, wf_s, device=device)
    touched = np.zeros(np.asarray(coordinates).shape[1], dtype=bool)
    touched[ed.ravel()] = True
    return _sparse_rows(f, touched)


def assemble_tangent(handle, ds, s=None):
    """Replaces the inline DP:1047-1050 (+1058): K_tangent (csr) and F from `ds` (9,n_int) and
    `s` (4,n_int).  `handle` is a MeshContext or any object carrying `.fep_ctx` (the K/B returned
    by get_elastic_stiffness_matrix).  Returns (K_tangent, F); F is None when `s` is None.  `ds` must be symmetric per
    point (the reference's tangents are): only its upper triangle, rows 0, 1, 2, 4, 5, 8, is read."""
    ctx = handle if isinstance(handle, MeshContext) else handle.fep_ctx
    return ctx.assemble(ds, s)

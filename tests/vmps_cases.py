"""Shared by the tests of the plane-stress von Mises model (test_vmps_host.py, test_vmps_gpu.py, test_vmps_step_gpu.py): the
fixtures of tests/golden/make_golden_return_map_mp_vmps.py (read only; the high-precision reference is not imported here),
the error measures per family and output with the bounds of DESIGN.md section 7, the caller of the mesh-free device entry
point, the materials and the uniaxial closed form.

tests/return_map_mp_cases.py and tests/model_ref.py tie their tables to their own models ('ABCDE', DEV_ENTRY), so what this
model needs of them is restated here.  A bound is eight times the error of the float64 restatement (tests/vmps_ref.py) against
the fixtures, MEASURED below as test_vmps_host.py reproduces it, at least the unit roundoff 2^-53 (the fixtures are rounded to
float64), and never more than the project's standing bounds: 1e-13 of the array maximum and 1e-12 per point, in family D
(seventeen decades: no array-wide bound) 5e-12 per point.  Family E (pairs one ulp apart across the yield surface) compares
the stress alone, and its flags not at all."""
import ctypes
import functools

import numpy as np

from conftest import load_golden
from return_map_mp_cases import MARGIN, UNIT, merge  # noqa: F401
from vm_cases import BULK, HARDENING, POISSON, SHEAR, SIGMA_Y, YIELD, YOUNG, fep  # noqa: F401
from vmps_ref import surface_residual

FAMILIES = 'ACDEF'
STANDING = {'A': (1e-13, 1e-12), 'C': (1e-13, 1e-12), 'D': (None, 5e-12), 'E': (1e-13, 1e-12), 'F': (1e-13, 1e-12)}
KEYS = ('s', 'ds', 'ep')
UNIFORM = (SHEAR, BULK, HARDENING, YIELD)

# (array-wide, per point) errors of the restatement against the fixtures, rounded up to two digits: DESIGN.md section 7
MEASURED = {
    ('A', 'ds'): (3.9e-16, 7.6e-16),
    ('A', 'ep'): (2.8e-16, 6.8e-14),
    ('A', 's'): (8.3e-16, 2.2e-15),
    ('C', 'ds'): (3.9e-16, 5.7e-16),
    ('C', 'ep'): (4.3e-16, 3.1e-15),
    ('C', 's'): (1.8e-16, 4.5e-16),
    ('D', 'ds'): (5.0e-17, 4.3e-16),
    ('D', 'ep'): (4.1e-16, 8.9e-16),
    ('D', 's'): (1.6e-16, 4.4e-16),
    ('E', 's'): (2.3e-16, 2.5e-16),
    ('F', 'ds'): (2.6e-16, 7.4e-16),
    ('F', 'ep'): (2.1e-16, 2.2e-13),
    ('F', 's'): (1.5e-16, 4.4e-16),
}
# max over the plastic points of a family of |sqrt(eta'^T P eta') - Y| / Y, eta' = s - a M p_new from the returned s and the
# new p: a difference of two numbers of the size of the back stress, which is 1e8 Y at D's largest overshoots with hardening and
# 1e3 Y in F (the figure is that cancellation, u a |p_new| / Y, not a distance the iteration left)
SURFACE_MEASURED = {'A': 1.8e-15, 'C': 1.3e-15, 'D': 4.8e-09, 'F': 1.5e-13}
MAX_ITERATIONS = 7                                                      # the most Newton iterations a point of the fixtures takes


@functools.lru_cache(maxsize=None)
def fixture():
    g = load_golden('return_map_mp_vmps')
    fix = {k: g[k] for k in g.files}
    for v in fix.values():
        v.setflags(write=False)
    return fix


def groups(fix):
    """The two launches: (indices, e0 or None) of the points without and with the initial strain."""
    w = fix['with_e0']
    return (np.flatnonzero(~w), None), (np.flatnonzero(w), fix['e0'].reshape(4, 1))


def errors(fix, got, idx):
    """got: dict s, ds, ep of the points idx -> {(family, key): (array-wide, per point)}; ds without the `no_tangent` points;
    family E: s alone."""
    out = {}
    fam = fix['family'][idx]
    for f in np.unique(fam):
        name = FAMILIES[f]
        for key in (('s',) if name == 'E' else [k for k in KEYS if k in got]):
            sel = fam == f
            if key == 'ds':
                sel = sel & ~fix['no_tangent'][idx]
            a, b = np.asarray(got[key])[:, sel], fix[key][:, idx[sel]]
            d, s = np.abs(a - b).max(axis=0), np.abs(b).max(axis=0)
            pt = np.where(s > 0, d / np.where(s > 0, s, 1.0), d)
            out[name, key] = (float(d.max() / max(s.max(), 1e-300)), float(pt.max()))
    return out


def surface_errors(fix, s, ep, idx):
    """{family: max |sqrt(eta'^T P eta') - Y| / Y} over the plastic points of idx outside family E, from the returned stress
    and the NEW plastic strain."""
    lab, fam = fix['label'][idx], fix['family'][idx]
    res = np.abs(surface_residual(s, ep, fix['m3'][idx], fix['m4'][idx])) / fix['m4'][idx]
    return {FAMILIES[f]: float(res[(fam == f) & (lab == 1)].max()) for f in np.unique(fam) if FAMILIES[f] != 'E'}


def bound(family, key):
    """(array-wide or None, per point)"""
    wide, pt = (max(v, UNIT) for v in MEASURED[family, key])
    s_wide, s_pt = STANDING[family]
    return (None if s_wide is None else min(MARGIN * wide, s_wide)), min(MARGIN * pt, s_pt)


def check(errs):
    """Prints every figure, then asserts all of them."""
    bad = []
    for (family, key), (wide, pt) in sorted(errs.items()):
        b_wide, b_pt = bound(family, key)
        print(f'vmps {family} {key:2s} array-wide {wide:.2e} (<= {b_wide})  per point {pt:.2e} (<= {b_pt:.2e})')
        if (b_wide is not None and not wide <= b_wide) or not pt <= b_pt:
            bad.append((family, key, wide, pt))
    assert not bad, bad


def check_surface(errs):
    bad = []
    for family, v in sorted(errs.items()):
        b = MARGIN * max(SURFACE_MEASURED[family], UNIT)
        print(f'vmps {family} yield surface {v:.2e} (<= {b:.2e})')
        if not v <= b:
            bad.append((family, v))
    assert not bad, bad


def check_flags(fix, idx, got):
    """ind_p of every point outside family E and both counters (n_apex = 0): equal to the labels' where the launch has no point
    of E; a point of E may sit on either side, so there the counter is the call's own ind_p."""
    lab = fix['label'][idx]
    keep = fix['family'][idx] != FAMILIES.index('E')
    assert np.array_equal(np.asarray(got['ind_p'])[keep], (lab != 0)[keep])
    assert got['n_apex'] == 0 and got['n_smooth'] == int(np.asarray(got['ind_p']).sum())
    if keep.all():
        assert got['n_smooth'] == int((lab != 0).sum())


def dev_return_map(e, order, p, e0, mats, accept, entry='fep_return_map_vmps_dev'):
    """model_ref.dev_return_map for this model (that one looks its entry point up by the names of its own models): the mesh-free
    device entry point on torch tensors; the strain (3, n) is handed over in `order`, `p` may be None.  -> s, ds, ind_p, the two
    counters as n_smooth / n_apex, 'ep' the device copy of p afterwards."""
    import torch
    dev = torch.device('cuda', 0)
    n = np.size(mats[0])
    up = lambda v: torch.from_numpy(np.array(v, dtype=np.float64, order='C')).to(dev)     # noqa: E731  (a writable copy)
    ed = up(e.T if order == 'F' else e)
    ps, cs = (3, 1) if order == 'F' else (1, n)
    pd = None if p is None else up(p)
    md = [up(m) for m in mats]
    f64 = dict(dtype=torch.float64, device=dev)
    S, DS = torch.zeros((4, n), **f64), torch.zeros((9, n), **f64)
    ind, cnt = torch.zeros(n, dtype=torch.uint8, device=dev), torch.full((2,), -1, dtype=torch.int64, device=dev)
    e0v = None if e0 is None else np.ascontiguousarray(e0, dtype=np.float64).ravel()
    rc = getattr(fep.lib(), entry)(0, torch.cuda.current_stream().cuda_stream, n, ed.data_ptr(), ps, cs,
                                   None if e0v is None else e0v.ctypes.data_as(ctypes.c_void_p),
                                   None if pd is None else pd.data_ptr(), *(m.data_ptr() for m in md),
                                   int(accept), S.data_ptr(), DS.data_ptr(), ind.data_ptr(), cnt.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    k = cnt.cpu().numpy()
    return {'s': S.cpu().numpy(), 'ds': DS.cpu().numpy(), 'ind_p': ind.cpu().numpy().astype(bool), 'n_smooth': int(k[0]),
            'n_apex': int(k[1]), 'ep': None if pd is None else pd.cpu().numpy()}


def uniaxial(sigma, young=YOUNG, poisson=POISSON, sigma_y=SIGMA_Y, a=HARDENING):
    """The closed form of uniaxial tension sigma >= sigma_y from a virgin state: (e (3,), s (4,), p (4,), tangent modulus)."""
    epl = (sigma - sigma_y) / (1.5 * a)
    e = np.array([sigma / young + epl, -poisson * sigma / young - epl / 2, 0.0])
    return e, np.array([sigma, 0.0, 0.0, 0.0]), np.array([epl, -epl / 2, 0.0, -epl / 2]), young * 1.5 * a / (young + 1.5 * a)


# ---------------------------------------------------------------------------------------
# mesh states: model_step_cases.state / build for this model (those draw from their own two models)
# ---------------------------------------------------------------------------------------
VM_CRIT_FLOOR = 1e-9                                                    # |crit| / Y below which rounding may decide the flag
STEP_NAMES = ('strip1', 'curved', 'block257')                           # the smallest named mesh, a curved one, a block edge


def state(t, elem, coord, rng):
    """(U, ep, per-point materials, e0): a random displacement scaled so that the median point sits on the yield surface, a
    traceless previous plastic strain, materials +-40 % per point, a (4, 1) initial strain."""
    from elem_ref import ElemRef
    from model_ref import traceless
    from vmps_ref import vmps_return_map
    ref = ElemRef(elem, coord, fep.element_tables(t))
    n = ref.n_int
    U = rng.normal(0, 1.0, size=(2, coord.shape[1]))
    nrm = vmps_return_map(ref.strain(U)[0], None, *UNIFORM)['crit'] + YIELD
    U *= YIELD / np.median(nrm)
    ep = traceless(rng, n, 0.1 * YIELD / (2 * SHEAR))
    f = rng.uniform(0.6, 1.4, n)
    per_point = (SHEAR * f, BULK * f[::-1], HARDENING * rng.uniform(0, 2, n), YIELD * rng.uniform(0.6, 1.4, n))
    e0 = rng.normal(0, 0.2 * YIELD / (2 * SHEAR), size=(4, 1))
    return U, ep, per_point, e0


@functools.lru_cache(maxsize=None)
def build(t, name):
    """-> dict elem, coord, U, ep, mats, e0 (or None), accept of the case, the same on every route: the mesh and the flags of
    model_step_cases (per-point materials, initial strain, accept: the bits of the case's number), this module's state."""
    import model_step_cases as msc
    rng = np.random.default_rng(msc.seed('vmps', t, name))
    elem, coord = msc.mesh(t, name, rng)
    pp, with_e0, accept = msc.flags(t, name)
    U, ep, per_point, e0 = state(t, elem, coord, rng)
    n = ep.shape[1]
    mats = per_point if pp else tuple(v * np.ones(n) for v in UNIFORM)
    return dict(elem=elem, coord=coord, U=U, ep=ep, mats=mats, e0=e0 if with_e0 else None, accept=accept)


def plane_strain_z3(e, p, mats, restate=None):
    """Per point the out-of-plane initial strain z3 at which the plane-strain law's s[3] vanishes (the secant method on the
    float64 restatement tests/vm_ref.py; s33 is increasing and piecewise smooth in z3) -> [(z3, the restatement there)]."""
    from vm_ref import vm_return_map
    out = []
    for k in range(e.shape[1]):
        m = [np.asarray(v, dtype=float).ravel()[k if np.size(v) > 1 else 0] for v in mats]
        f = lambda z3: vm_return_map(e[:, k:k + 1], p[:, k:k + 1], *m, True, e0=np.array([0.0, 0.0, 0.0, z3]))      # noqa: E731
        lam = m[1] - 2 * m[0] / 3
        x0 = -lam * (e[0, k] - p[0, k] + e[1, k] - p[1, k]) / (lam + 2 * m[0]) + p[3, k]
        x1 = x0 + 1e-3 * m[3] / (2 * m[0])
        f0, f1 = f(x0)['s'][3, 0], f(x1)['s'][3, 0]
        for _ in range(60):
            if f1 == f0:
                break
            x0, x1, f0 = x1, x1 - f1 * (x1 - x0) / (f1 - f0), f1
            f1 = f(x1)['s'][3, 0]
        out.append((x1, f(x1)))
    return out


def equivalence_points(a, n=40, seed=31):
    """(e, p, mats) of n steel points at two yield strains, traceless p: more than half of them plastic."""
    rng = np.random.default_rng(seed)
    y = YIELD / (2 * SHEAR)
    e = rng.normal(0, 2.0 * y, size=(3, n))
    p = rng.normal(0, 0.3 * y, size=(4, n))
    p[3] = -(p[0] + p[1])
    return e, p, (SHEAR, BULK, a, YIELD)

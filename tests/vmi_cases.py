"""Shared by the tests of the von Mises model with isotropic hardening (test_vmi_host.py, test_vmi_gpu.py): the fixtures of
tests/golden/make_golden_vmi_mp.py (read only; the high-precision reference is not imported here), the error measures per
family and output with the bounds of DESIGN.md section 7, the caller of the mesh-free device entry point, the curves and the
mesh states of the step tests.

A bound is eight times the error of the float64 restatement (tests/vmi_ref.py) against the fixtures, MEASURED below as
test_vmi_host.py reproduces it, at least the unit roundoff 2^-53 (the fixtures are rounded to float64), and never more than the
project's standing bounds: 1e-13 of the array maximum and 1e-12 per point, in family D (sixteen decades of overshoot: no
array-wide bound) 5e-12 per point.  Family E (pairs one ulp apart across the yield surface or a breakpoint) compares the
stress alone, and its flags not at all.  The tangent jumps where the return ends on a breakpoint (include/fep.h): `ds` is not
compared at points the reference marks `no_tangent`, nor where its new kappa lies within NEAR of a breakpoint, relative to kappa:
the multiplier is a quotient of rounded numbers, so the restatement and the kernels may accept the segment on the other side
there.  NEAR = 1e-13 is 900 unit roundoffs, where the multiplier's own error is a few; family B's returns that end 2 and 3 ulps
of the strain from a breakpoint are such points."""
import ctypes
import functools

import numpy as np

from conftest import load_golden
from return_map_mp_cases import MARGIN, UNIT, merge  # noqa: F401
from vm_cases import BULK, HARDENING, SHEAR, YIELD, fep  # noqa: F401

FAMILIES = 'ABCDE'
STANDING = {'A': (1e-13, 1e-12), 'B': (1e-13, 1e-12), 'C': (1e-13, 1e-12), 'D': (None, 5e-12), 'E': (1e-13, 1e-12)}
KEYS = ('s', 'ds', 'ep')
UNIFORM = (SHEAR, BULK, HARDENING, YIELD)
NEAR = 1e-13
N_CURVES = 4

# (array-wide, per point) errors of the restatement against the fixtures, rounded up to two digits: DESIGN.md section 7
MEASURED = {
    ('A', 'ds'): (3.3e-16, 5.5e-16),
    ('A', 'ep'): (3.2e-16, 6.9e-16),
    ('A', 's'): (2.8e-16, 8.7e-16),
    ('B', 'ds'): (3.1e-16, 5.0e-16),
    ('B', 'ep'): (3.1e-16, 4.4e-16),
    ('B', 's'): (2.2e-16, 5.9e-16),
    ('C', 'ds'): (3.9e-16, 4.7e-16),
    ('C', 'ep'): (2.2e-16, 3.5e-16),
    ('C', 's'): (3.1e-16, 4.7e-15),
    ('D', 'ds'): (3.4e-16, 4.4e-16),
    ('D', 'ep'): (2.2e-16, 6.9e-16),
    ('D', 's'): (2.8e-16, 3.7e-15),
    ('E', 's'): (3.3e-16, 5.4e-16),
}


@functools.lru_cache(maxsize=None)
def cpu_cycle(element_type, isotropic=15000.0, hardening=0.0):
    """solve_cutout_cyclic at level 0 on the CPU restatement with the sparse direct solve and the load of vm_cases.cpu_cycle
    (peak traction 200): by default purely isotropic hardening of the same total modulus as that run's kinematic a = 10 000
    (dR/dkappa = 2/3 dsigma_y/deps = a).  Computed once per session, never modified."""
    from vm_cases import top_load
    from vmi_ref import VMIRefContext
    return fep.solve_cutout_cyclic(element_type, level=0, context_factory=VMIRefContext, linear_solver='direct',
                                   f_ext=top_load(element_type, 0, (0, 200.0)), hardening=hardening, isotropic=isotropic)


@functools.lru_cache(maxsize=None)
def fixture():
    g = load_golden('return_map_mp_vmi')
    fix = {k: g[k] for k in g.files}
    for v in fix.values():
        v.setflags(write=False)
    return fix


def curve(c):
    """(kappa, slope) of the fixture's curve c: 0 flat, 1 linear, 2 eight saturating segments, 3 four with one softening."""
    fix = fixture()
    return fix[f'kappa_{c}'], fix[f'slope_{c}']


def launches(fix):
    """The eight launches: (indices, e0 or None, curve number)."""
    out = []
    for c in range(N_CURVES):
        for w in (False, True):
            out.append((np.flatnonzero((fix['curve'] == c) & (fix['with_e0'] == w)), fix['e0'].reshape(4, 1) if w else None, c))
    return out


def errors(fix, got, idx):
    """got: dict s, ds, ep of the points idx -> {(family, key): (array-wide, per point)}; ds without the `no_tangent` points
    and those within NEAR of a breakpoint; family E: s alone."""
    out = {}
    fam = fix['family'][idx]
    for f in np.unique(fam):
        name = FAMILIES[f]
        for key in (('s',) if name == 'E' else [k for k in KEYS if k in got]):
            sel = fam == f
            if key == 'ds':
                sel = sel & ~fix['no_tangent'][idx] & ~(fix['dist'][idx] < NEAR)
            if not sel.any():
                continue
            a, b = np.asarray(got[key])[:, sel], fix[key][:, idx[sel]]
            d, s = np.abs(a - b).max(axis=0), np.abs(b).max(axis=0)
            pt = np.where(s > 0, d / np.where(s > 0, s, 1.0), d)
            out[name, key] = (float(d.max() / max(s.max(), 1e-300)), float(pt.max()))
    return out


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
        print(f'vmi {family} {key:2s} array-wide {wide:.2e} (<= {b_wide})  per point {pt:.2e} (<= {b_pt:.2e})')
        if (b_wide is not None and not wide <= b_wide) or not pt <= b_pt:
            bad.append((family, key, wide, pt))
    assert not bad, bad


def check_flags(fix, idx, got):
    """ind_p of every point outside family E and both counters (n_apex = 0): equal to the labels' where the launch has no point
    of E; a point of E may sit on either side of the yield surface, so there the counter is the call's own ind_p."""
    lab = fix['label'][idx]
    keep = fix['family'][idx] != FAMILIES.index('E')
    assert np.array_equal(np.asarray(got['ind_p'])[keep], (lab != 0)[keep])
    assert got['n_apex'] == 0 and got['n_smooth'] == int(np.asarray(got['ind_p']).sum())
    if keep.all():
        assert got['n_smooth'] == int((lab != 0).sum())


def dev_return_map(e, order, p, e0, mats, crv, accept):
    """The mesh-free device entry point fep_return_map_vmi_dev on torch tensors (model_ref.dev_return_map looks its entry points
    up by the names of its own models and has no place for a curve); the strain (3, n) is handed over in `order`, `p` may be
    None.  -> s, ds, ind_p, the two counters as n_smooth / n_apex, 'ep' the device copy of p afterwards."""
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
    kap, slo = (np.ascontiguousarray(v, dtype=np.float64) for v in crv)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                       # noqa: E731
    rc = fep.lib().fep_return_map_vmi_dev(0, torch.cuda.current_stream().cuda_stream, n, ed.data_ptr(), ps, cs,
                                          None if e0v is None else vp(e0v), None if pd is None else pd.data_ptr(),
                                          *(m.data_ptr() for m in md), kap.size, vp(kap), vp(slo),
                                          int(accept), S.data_ptr(), DS.data_ptr(), ind.data_ptr(), cnt.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    k = cnt.cpu().numpy()
    return {'s': S.cpu().numpy(), 'ds': DS.cpu().numpy(), 'ind_p': ind.cpu().numpy().astype(bool), 'n_smooth': int(k[0]),
            'n_apex': int(k[1]), 'ep': None if pd is None else pd.cpu().numpy()}


# ---------------------------------------------------------------------------------------
# random points and mesh states for the comparisons against the restatement
# ---------------------------------------------------------------------------------------
CRIT_FLOOR = 1e-9                                                       # |crit| / Y below which rounding may decide the flag
BREAK_FLOOR = 1e-9                                                      # distance of an accepted kappa to a breakpoint


def state_rows(rng, n, scale, kappa_max):
    """(4, n) state: three plastic-strain rows of size `scale` and kappa uniform in [0, kappa_max]."""
    p = rng.normal(0, scale, size=(4, n))
    p[3] = rng.uniform(0, kappa_max, n)
    return p


def away_from_breakpoints(ref, crv):
    """No accepted kappa of the restatement's result `ref` (with 'ep' of an accepting call) within BREAK_FLOOR of a breakpoint."""
    k = ref['ep'][3][ref['ind_p']]
    return all((np.abs(k - b) > BREAK_FLOOR).all() for b in crv[0][1:])


def points(n, uniform, seed, crv):
    """Mesh-free inputs (e, p, e0, four materials): strains of a few yield strains, kappa spread over the whole curve."""
    rng = np.random.default_rng(seed)
    one = np.ones(n)
    f = one if uniform else rng.uniform(0.6, 1.4, n)
    e = rng.normal(0, 1.8e-3, size=(3, n))
    p = state_rows(rng, n, 1e-3, 1.3 * crv[0][-1])
    e0 = rng.normal(0, 1e-3, size=(4, 1))
    return e, p, e0, (SHEAR * f, BULK * f[::-1], HARDENING * one if uniform else HARDENING * rng.uniform(0, 2, n), YIELD * f)

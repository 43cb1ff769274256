"""Shared by test_nonfinite_host.py and test_nonfinite_gpu.py: the cases that put a NaN or an infinity into the DATA of a call
(never into an index, a table or a size) and what each of them has to reach.  The conditions are asserted on the restatements
alone by the host module, so that a case which misses its target blames this generator, on the CPU, before a GPU run meets it.
The four rules the cases exist for are in DESIGN.md section 7 and include/fep.h (fep_return_map_*).

Points.  Per model the 1000 points of the mesh-free tests (`thousand`, shared with test_return_map_mp_gpu.py), tiled to
3 * 256 + 1 points, with poisoned copies of point 0 at lanes 0, 63, 64, 255, 256 and n - 1, the wave and workgroup edges of the
ballot counters.  Twelve poisons, each lane of a launch a different one, so two launches (`LAUNCHES`): NaN in each strain
component, +Inf and -Inf in e[0], NaN in ep[0], ep[2], ep[3], NaN in each of the four material parameters.  A further launch per
component of e0 puts the NaN there and poisons every point.  For 'vmi' (von Mises with isotropic hardening; the points of its
mesh-free tests on the eight-segment curve) row 3 of ep is kappa, so ('p', 3, NaN) is a NaN kappa; a third launch of that model
alone holds +Inf and -Inf there (`launches`).  A non-finite kappa counts like a NaN trial strain (include/fep.h; the kernel's
poison = -fabs(0.0 * k0)): the point is elastic with the elastic tangent and a NaN stress, no counter counts it and its column
of ep stays as it went in.

Structural zeros.  The Drucker-Prager oracle and the von Mises restatement form `dev @ E`, `vol @ E`, `2 Dev G + Vol K` as
matrix products and so multiply the zeros of those matrices by the poison: 0 * Inf and 0 * NaN are NaN.  The kernels never
form these products (dv2 = Et2 / 2, d02 = d12 = 0, d22 = G are written out), and neither does the Mohr-Coulomb restatement.
So where a restatement is non-finite in the shear stress s[2] or in a tangent entry of the shear row or column (`SHEAR_S`,
`SHEAR_DS`) a kernel may hold the finite value of its formula; anywhere else the finiteness must agree, and a kernel is never
non-finite where the restatement is finite (`masks_agree`).  The Mohr-Coulomb kernel and its restatement agree everywhere.
The 'vmi' restatement needs the allowance as von Mises does: it adds (K tr + poison) * (1, 1, 0, 1) to the stress and forms
2 Dev G + Vol K, so its s[2] and its shear tangent entries are NaN where tr, the poison or a material is, while the kernel
writes s2 = 2G dv2 and d02 = d12 = 0 (test_nonfinite_host.py shows the restatement's side on the CPU).  An infinite strain makes
the point plastic in the 'vmi' kernel as in the von Mises one (`vm_infinite`).

Meshes.  Per element type the 257-element mesh of model_step_cases with that module's state (Drucker-Prager: the state of
test_element_route_gpu.py), and U[:, k] = NaN at one interior vertex or, P2 / Q2 / P4, at one midside or interior node.
'vmi' has one kind more, 'kappa': a clean U and ep[3, k] = NaN at the middle point k of the element nearest the centre.

Solver cases.  The two smallest cases of solver_cases.py with a multigrid hierarchy; NaN in (a) a K entry of a free row,
(b) b at a free DOF, (c) b at a constrained DOF, (d) the K entries whose row and column are both constrained."""
import zlib

import numpy as np

import model_step_cases as msc
import solver_cases as sc
from conftest import dp_materials
from elem_ref import ElemRef

MODELS = ('dp', 'vm', 'mc', 'vmi')
N_POINTS = 3 * 256 + 1
LANES = (0, 63, 64, 255, 256, N_POINTS - 1)
NAN, INF = float('nan'), float('inf')
# (array, row, value): 'e' strain (3, n), 'p' previous plastic strain (4, n), 'm' the four material arrays
POISONS = (('e', 0, NAN), ('e', 1, NAN), ('e', 2, NAN), ('e', 0, INF), ('e', 0, -INF), ('p', 0, NAN),
           ('p', 2, NAN), ('p', 3, NAN), ('m', 0, NAN), ('m', 1, NAN), ('m', 2, NAN), ('m', 3, NAN))
LAUNCHES = (POISONS[0:6], POISONS[6:12])
VMI_KAPPA_POISONS = (('p', 3, INF), ('p', 3, -INF))                     # 'vmi' alone, a launch of their own
VMI_POINT_CURVE = 2                                                     # of the mesh-free 'vmi' points
MAX_POISONED_POINTS, MAX_DIRTY_ELEMENTS = 0.01, 0.05
SHEAR_S = (2,)                                                          # rows of s (4, n)
SHEAR_DS = (2, 5, 6, 7, 8)                                              # rows of ds (9, n), row-major 3x3
TOL, TOL_PT = 1e-13, 1e-12                                              # of the array maximum, per point
MAX_ITER = 200                                                          # of every poisoned solve


# ---------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------
def launches(model):
    """The launches of `model`: LAUNCHES, and for 'vmi' a third with an infinite kappa of either sign."""
    return LAUNCHES + ((VMI_KAPPA_POISONS,) if model == 'vmi' else ())


def launch_ids():
    return [(m, k) for m in MODELS for k in range(len(launches(m)))]


def launch_lanes(poisons):
    """The lanes that hold the poisons of a launch: all six, or for a shorter launch the two at the workgroup edge."""
    return LANES if len(poisons) == len(LANES) else LANES[3:3 + len(poisons)]


def point_curve(model):
    """(kappa, slope) of the mesh-free calls of 'vmi'; None for the other models."""
    if model != 'vmi':
        return None
    from vmi_cases import curve
    return curve(VMI_POINT_CURVE)


def thousand(model):
    """(e, p, materials, the restatement's result, class per point: 0 elastic, 1 counts[0], 2 counts[1]) of the 1000-point set
    of the model's mesh-free test (Drucker-Prager: test_parity_gpu's random points with a band at the apex)."""
    n = 1000
    if model == 'mc':
        from mc_cases import points
        from mc_ref import mc_return_map
        e, p, _, *mats = points(n, False, 100 + n)
        ref = mc_return_map(e, p, *mats)
        return e, p, mats, ref, np.where(ref['branch'] == 0, 0, np.where(ref['branch'] == 4, 2, 1))
    if model == 'vmi':
        from vmi_cases import points
        from vmi_ref import vmi_return_map
        e, p, _, mats = points(n, False, 1100, point_curve(model))
        ref = vmi_return_map(e, p, *mats, point_curve(model))
        return e, p, list(mats), ref, ref['ind_p'].astype(np.int64)
    if model == 'vm':
        from test_vm_gpu import _points
        from vm_ref import vm_return_map
        e, p, _, *mats = _points(n, False, 100 + n)
        ref = vm_return_map(e, p, *mats)
        return e, p, mats, ref, ref['ind_p'].astype(np.int64)
    from oracle import fep_oracle as orc
    rng = np.random.default_rng(99)
    sh, bu, eta, c = dp_materials(n)
    mats = [sh * rng.uniform(0.5, 2, n), bu * rng.uniform(0.5, 2, n), eta * rng.uniform(0.5, 1.5, n), c * rng.uniform(0.5, 2, n)]
    e = rng.normal(0, 2e-4, size=(3, n))
    e[:, : n // 20] += 4e-4                                                 # a band of apex points
    p = rng.normal(0, 2e-5, size=(4, n))
    ref = orc.return_map(e, p.copy(), *mats, False)
    apex = ref['ind_p'] & (np.abs(ref['ds']).sum(axis=0) == 0)              # the apex tangent is zero
    assert int(apex.sum()) == ref['n_apex']
    return e, p, mats, ref, np.where(apex, 2, ref['ind_p'].astype(np.int64))


def restate(model, e, p, mats, e0=None, accept=False, curve='points'):
    """The model's restatement -> s, ds, ind_p, ep (the updated copy when accepting), n_smooth, n_apex.  No argument is
    modified.  'vmi': on `curve`, by default the one of the mesh-free points; a mesh case passes its own (None: the context's
    default).  Drucker-Prager: the oracle, in its TSX flavour when there is an initial strain (a call without a plastic
    point then returns before it touches ep: the copy comes back as it went in)."""
    with np.errstate(all='ignore'):
        if model == 'dp':
            from oracle import fep_oracle as orc
            pc = np.array(p, dtype=float)
            r = orc.return_map(np.array(e, dtype=float), pc, *[np.asarray(m, dtype=float) for m in mats], accept,
                               e0=None if e0 is None else np.asarray(e0, dtype=float).reshape(4, 1), tsx=e0 is not None)
            return dict(s=r['s'], ds=r['ds'], ind_p=r['ind_p'], ep=pc, n_smooth=r['n_smooth'], n_apex=r['n_apex'])
        crv = (point_curve(model) if isinstance(curve, str) else curve) if model == 'vmi' else None
        r = msc.return_map(model, e, p, tuple(mats), e0, accept, crv)
        return dict(s=r['s'], ds=r['ds'], ind_p=r['ind_p'], ep=r['ep'] if accept else np.array(p, dtype=float),
                    n_smooth=r['n_smooth'], n_apex=r['n_apex'])


def _plastic_strain(model, p):
    """The four components of the plastic strain in the state p: 'vmi' keeps kappa in row 3 and implies p33 = -(p11 + p22)."""
    p = np.asarray(p, dtype=float)
    return np.array([p[0], p[1], p[2], -(p[0] + p[1])]) if model == 'vmi' else p


def trial_strain_nan(e, p, e0=None, model=None):
    """Per point: whether (e + e0) - ep has a NaN component (an infinity alone is none); 'vmi': or kappa is not finite."""
    with np.errstate(all='ignore'):
        Et = np.concatenate([np.asarray(e, dtype=float), np.zeros((1, np.shape(e)[1]))])
        if e0 is not None:
            Et = Et + np.asarray(e0, dtype=float).reshape(4, 1)
        nan = np.isnan(Et - _plastic_strain(model, p)).any(axis=0)
        return nan | ~np.isfinite(np.asarray(p, dtype=float)[3]) if model == 'vmi' else nan


def vm_infinite(model, e, p, e0=None):
    """Per point: a von Mises point whose trial strain holds an infinity and no NaN.  The kernel forms the deviator as
    (2/3) Et0 - Et1 / 3 - Et3 / 3, which is infinite, so its norm is, the point is plastic (and counted) and N = Inf / Inf makes
    every entry of s and ds NaN.  The restatement forms Et - tr / 3 = Inf - Inf = NaN, so its criterion is NaN and the point
    elastic, with a NaN stress beside the finite elastic tangent.  Neither hides the infinity; the flag and the tangent's
    finiteness differ, and the tests assert each side's as stated here.  The same holds of 'vmi', whose kernel forms the same
    deviator and whose multiplier on the last segment is then infinite."""
    n = np.shape(e)[1]
    if model not in ('vm', 'vmi'):
        return np.zeros(n, dtype=bool)
    with np.errstate(all='ignore'):
        Et = np.concatenate([np.asarray(e, dtype=float), np.zeros((1, n))])
        if e0 is not None:
            Et = Et + np.asarray(e0, dtype=float).reshape(4, 1)
        Et = Et - _plastic_strain(model, p)
    odd = np.isinf(Et).any(axis=0) & ~np.isnan(Et).any(axis=0)
    return odd & np.isfinite(np.asarray(p, dtype=float)[3]) if model == 'vmi' else odd   # (a non-finite kappa: elastic)


def elastic_tangent(model, mats):
    """ds (9, n) of the elastic branch: the restatement at zero strain."""
    n = np.size(mats[0])
    r = restate(model, np.zeros((3, n)), np.zeros((4, n)), mats)               # (on any curve: no point yields)
    assert not r['ind_p'].any()
    return r['ds']


def point_launch(model, k):
    """Launch k of launches(model) -> dict: 'clean' and 'poisoned' inputs (e, p, mats), 'lanes', 'poisons', 'cls' the
    class of every point of the clean launch.  The clean launch holds the unpoisoned copy of point 0 at every lane."""
    e1, p1, mats1, _, cls1 = thousand(model)
    idx = np.arange(N_POINTS) % 1000
    poisons = launches(model)[k]
    idx[np.array(LANES)] = 0
    lanes = np.array(launch_lanes(poisons))
    e, p, mats = np.array(e1[:, idx]), np.array(p1[:, idx]), [np.array(np.asarray(m)[idx], dtype=float) for m in mats1]
    pe, pp, pm = e.copy(), p.copy(), [m.copy() for m in mats]
    for lane, (arr, row, val) in zip(lanes, poisons):
        if arr == 'e':
            pe[row, lane] = val
        elif arr == 'p':
            pp[row, lane] = val
        else:
            pm[row][lane] = val
    return dict(clean=(e, p, mats), poisoned=(pe, pp, pm), lanes=lanes, poisons=poisons, cls=cls1[idx])


def masks_agree(model, got, ref, key):
    """Finiteness of the kernel's `got[key]` against the restatement's (module docstring): equal, except that a von Mises or
    Drucker-Prager kernel may be finite in the shear entries where the restatement is not.  -> (ok, the mask of entries at
    which both are finite)."""
    g, r = ~np.isfinite(got[key]), ~np.isfinite(ref[key])
    allowed = np.zeros_like(r)
    if model != 'mc' and key in ('s', 'ds'):
        allowed[list(SHEAR_S if key == 's' else SHEAR_DS)] = True
    ok = not (g & ~r).any() and not ((r & ~g) & ~allowed).any()
    return ok, ~g & ~r


# ---------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------
N_VERTICES = {'P1': 3, 'P2': 3, 'Q1': 4, 'Q2': 4, 'P4': 3}
NODE_KINDS = {'P1': ('vertex',), 'Q1': ('vertex',), 'P2': ('vertex', 'midside'), 'Q2': ('vertex', 'midside'),
              'P4': ('vertex', 'interior')}


def mesh_cases():
    return [(t, kind) for t in msc.TYPES for kind in NODE_KINDS[t]]


def model_mesh_cases():
    """(model, t, kind): the node kinds for every model, and 'kappa' for 'vmi'."""
    return [(m, t, kind) for m in MODELS for t, kind in mesh_cases() + ([(t, 'kappa') for t in msc.TYPES] if m == 'vmi' else [])]


_MESH_CASES = {}


def mesh_case(model, t, kind):
    """-> dict elem, coord, U, U_bad (U with NaN in both components of node `k`), ep, ep_bad (ep itself, except for the kind
    'kappa': U_bad is U and ep_bad has a NaN kappa at POINT `k`, the only dirty point), mats, e0, curve, k, and what `k` makes
    dirty:
    'elements' and 'points' (bool), 'nodes' (ids), 'dofs' (bool, DOF = 2 node + component) and `blocks`, the sorted keys
    n * n_n + m of the node blocks of K with a dirty contributor.  The same case on every route; cached, read-only."""
    key = (model, t, kind)
    if key in _MESH_CASES:
        return _MESH_CASES[key]
    curve = None
    if model == 'dp':
        from test_element_route_gpu import _state
        rng = np.random.default_rng(zlib.crc32(f'dp {t} block257'.encode()))
        elem, coord = msc.mesh(t, 'block257', rng)
        U, ep, mats, e0, _ = _state('plain', coord, 10.0 / 43, elem.shape[1] * msc.NQ[t], rng)
    else:
        c = msc.build(model, t, 'block257')
        elem, coord, U, ep, mats, e0, curve = (c[k] for k in ('elem', 'coord', 'U', 'ep', 'mats', 'e0', 'curve'))
    elem = np.asarray(elem, dtype=np.int64)
    n_n, nq = coord.shape[1], msc.NQ[t]
    nv = N_VERTICES[t]
    count = np.bincount(elem.ravel(), minlength=n_n)
    is_vertex = np.zeros(n_n, dtype=bool)
    is_vertex[elem[:nv].ravel()] = True
    lo, hi = coord.min(axis=1, keepdims=True), coord.max(axis=1, keepdims=True)
    inside = ((coord > lo + 1e-9) & (coord < hi - 1e-9)).all(axis=0)
    centre = (lo + hi) / 2
    if kind == 'kappa':
        assert model == 'vmi'
        el = np.flatnonzero(inside[elem].all(axis=0))                       # the elements with no node on the boundary
        el = int(el[np.argmin(((coord[:, elem[:nv, el]].mean(axis=1) - centre) ** 2).sum(axis=0))])
        k = el * nq + nq // 2
        dirty_e = np.arange(elem.shape[1]) == el
        points = np.arange(elem.shape[1] * nq) == k
        U_bad = np.array(U, dtype=float)
        ep_bad = np.array(ep, dtype=float)
        ep_bad[3, k] = NAN
        return _finish_mesh_case(key, elem, coord, U, U_bad, ep, ep_bad, mats, e0, curve, k, dirty_e, points, n_n)
    if kind == 'vertex':
        cand = is_vertex & inside
    elif kind == 'midside':
        cand = ~is_vertex & inside & (count == 2)
    else:                                                                   # P4: a node inside one element
        cand = ~is_vertex & (count == 1)
    cand = np.flatnonzero(cand)
    k = int(cand[np.argmin(((coord[:, cand] - centre) ** 2).sum(axis=0))])  # the candidate nearest the centre
    dirty_e = (elem == k).any(axis=0)
    U_bad = np.array(U, dtype=float)
    U_bad[:, k] = NAN
    return _finish_mesh_case(key, elem, coord, U, U_bad, ep, ep, mats, e0, curve, k, dirty_e, np.repeat(dirty_e, nq), n_n)


def _finish_mesh_case(key, elem, coord, U, U_bad, ep, ep_bad, mats, e0, curve, k, dirty_e, points, n_n):
    nodes = np.unique(elem[:, dirty_e])
    dofs = np.zeros(2 * n_n, dtype=bool)
    dofs[2 * nodes] = dofs[2 * nodes + 1] = True
    de = elem[:, dirty_e]
    blocks = np.unique((de[:, None, :] * n_n + de[None, :, :]).ravel())
    out = dict(elem=elem, coord=coord, U=np.array(U, dtype=float), U_bad=U_bad, ep=ep, ep_bad=ep_bad, mats=tuple(mats), e0=e0,
               curve=curve, k=k, elements=dirty_e, points=points, nodes=nodes, dofs=dofs, blocks=blocks)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _MESH_CASES[key] = out
    return out


def dirty_entries(case, pattern):
    """bool (nnz,): the CSR entries of `pattern` = (indptr, indices) that lie in a node block with a dirty contributor."""
    ip, ix = (np.asarray(a, dtype=np.int64) for a in pattern)
    n_n = case['coord'].shape[1]
    rows = np.repeat(np.arange(ip.size - 1, dtype=np.int64), np.diff(ip))
    return np.isin((rows // 2) * n_n + ix // 2, case['blocks'])


def elem_ref(case, t, pattern=None, record=False):
    return ElemRef(case['elem'], case['coord'], msc.fep.element_tables(t), pattern=pattern, record=record)


# ---------------------------------------------------------------------------------------
# solver cases
# ---------------------------------------------------------------------------------------
def solver_names():
    """The two smallest cases of solver_cases.CASES whose hierarchy has at least two levels."""
    with_levels = [n for n, c in sc.CASES.items() if len(c['nodes']) >= 2]
    return tuple(sorted(with_levels, key=lambda n: sc.CASES[n]['nodes'][0])[:2])


SOLVER_POISONS = ('a', 'b', 'c', 'd')


def solver_poison(K, b, qf, which):
    """(K data, b) with the poison `which` on the CSR matrix K (sorted, on the solver's pattern), the right-hand side b and
    the free-DOF mask qf.  (a) the diagonal entry of the middle free row, (b) b at that DOF, (c) b at every constrained DOF,
    (d) every stored entry whose row and column are both constrained."""
    data, rhs = np.array(K.data, dtype=float), np.array(b, dtype=float)
    qf = np.asarray(qf, dtype=bool)
    free = np.flatnonzero(qf)
    i = int(free[free.size // 2])
    rows = np.repeat(np.arange(K.shape[0]), np.diff(K.indptr))
    if which == 'a':
        at = np.flatnonzero((rows == i) & (K.indices == i))
        assert at.size == 1
        data[at] = NAN
    elif which == 'b':
        rhs[i] = NAN
    elif which == 'c':
        rhs[~qf] = NAN
    elif which == 'd':
        at = ~qf[rows] & ~qf[K.indices]
        assert at.sum() >= (~qf).sum() > 0                                  # at least the diagonals
        data[at] = NAN
    else:
        raise ValueError(which)
    return data, rhs


# ---------------------------------------------------------------------------------------
# the load-step loop with a failed solve
# ---------------------------------------------------------------------------------------
FOOTING = dict(element_type='P1', level=1, zeta_max=0.25)                   # the smallest P1 footing of the driver tests


def failing_solve(monkeypatch, k):
    """A test double, not a product change: from now on the ops of every driver run return from the k-th call of `solve`
    (1-based; call 1 is the elastic solve before the loop) what a failed solve returns, all NaN.  The real solve still
    runs, on the same solver object.  -> the list that receives the number of calls made."""
    from importlib import import_module
    newton = import_module('fem-elastoplasticity_amd.newton')
    real_make, calls = newton.make_ops, []

    def make_ops(*a, **kw):
        ops = real_make(*a, **kw)
        real_solve = ops.solve
        calls.append(0)

        def solve(*sa, **skw):
            x = real_solve(*sa, **skw)
            calls[-1] += 1
            if calls[-1] == k:
                x = x * 0.0 + NAN
            return x
        ops.solve = solve
        return ops
    monkeypatch.setattr(newton, 'make_ops', make_ops)
    return calls


def check_recovery(clean, bad, zeta_max):
    """The accepted load factors of a run whose first solve of the second load step failed, against the clean run's: the
    first step as it was, the second at half its increment, the end reached."""
    zc, zb = np.asarray(clean['zeta']), np.asarray(bad['zeta'])
    assert zb[0] == zc[0] and zc[1] > zc[0]
    assert zb[1] == zc[0] + (zc[1] - zc[0]) / 2, (zc[:3], zb[:3])
    assert zb[-1] >= zeta_max and (np.diff(zb) > 0).all()
    assert np.isfinite(bad['U_last']).all() and np.isfinite(bad['Ep']).all()

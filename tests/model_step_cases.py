"""Shared by test_model_step_cases_host.py and test_model_step_routes_gpu.py: the case grid of the von Mises, Mohr-Coulomb
and isotropic-hardening von Mises ('vmi') steps (model x element type x route x mesh), the meshes, the state of every case and
the conditions a case has
to meet before a kernel is compared on it.  The conditions are asserted on the restatements alone by the host module, so
that a case which does not reach what it exists for blames this generator, on the CPU, before a GPU run meets it.

Meshes: the named meshes of test_element_route_gpu.py at its sizes, and per type three block-edge meshes of 256, 257 and
255 elements (a jittered rectangle, at most one trailing element dropped): n_int modulo the 256-lane workgroup of the point
kernels is then 0, NQ and 256 - NQ, so that the last workgroup is full, holds one element, or lacks one, and (NQ not a
divisor of 256) an element's points are split across two workgroups.

State: the generators of the step tests (test_vm_gpu._case, test_mc_gpu._draw_case) on these meshes.  Von Mises: a random
displacement scaled so that the median point sits on the yield surface.  Mohr-Coulomb: one that grows eightfold from left to
right, scaled the same way, so that the right part reaches the apex.  Both with a previous plastic strain.  Uniform or
per-point materials (+-40 %, sin phi in 0.2 - 0.6), the (4, 1) initial strain or none, accepting or not: the three bits of
the case's number, so that all eight combinations occur for every model.  'vmi' (tests/vmi_ref.py): the displacement and the
state of test_vmi_gpu._case (the median point at 1.5 times the initial yield radius, kappa uniform on [0, 1.3 kappa_last] of
the case's curve; on the one-segment curves, which have no last breakpoint, that function's 0.02), and a hardening curve by
the case's number (`curve_id`): the four curves of the high-precision fixture (flat, one linear segment, eight saturating
segments, four with one softening) and None, a context on which set_hardening is never called, so that every element type
meets all five over its mesh names.  The generator is seeded from the model, the type
and the mesh name alone: every route sees the same case.  A case takes the first state its generator draws that meets the
conditions (build)."""
import zlib

import numpy as np

import meshes
from elem_ref import ElemRef
from mc_cases import COHESION, DIST_FLOOR, EPS_Y, P_BULK, P_SHEAR, R_FLOOR, SIN_PHI
from mc_ref import mc_return_map
from model_ref import traceless
from vm_cases import BULK, HARDENING, SHEAR, YIELD, fep
from vm_ref import vm_return_map
import vmi_cases
from vmi_ref import vmi_return_map

MODELS = ('vm', 'mc', 'vmi')
TYPES = ('P1', 'P2', 'Q1', 'Q2', 'P4')
ROUTES = {'P1': ('node', 'patch', 'coo'), 'P2': ('default', 'coo'), 'Q1': ('default', 'coo'), 'Q2': ('default', 'coo'),
          'P4': ('default', 'coo')}
NQ = {'P1': 1, 'P2': 7, 'Q1': 4, 'Q2': 9, 'P4': 12}
BLOCK = 256                                                             # lanes per workgroup of the point kernels (kBlock)
UNIFORM = {'vm': (SHEAR, BULK, HARDENING, YIELD), 'mc': (P_SHEAR, P_BULK, SIN_PHI, COHESION), 'vmi': vmi_cases.UNIFORM}
CURVES = (0, 1, 2, 3, None)                                             # fixture curves; None: set_hardening is not called
FLAT = (np.zeros(1), np.zeros(1))                                       # what a context without set_hardening runs on
KAPPA_ONE_SEGMENT = 0.02                                                # test_vmi_gpu._case: kappa range where kappa_last = 0
VM_CRIT_FLOOR = 1e-9                                                    # |crit| / Y below which rounding may decide the flag
MAX_EXCLUDED = 0.005                                                    # share of a case's points
MIN_PER_BRANCH, N_INT_ALL_BRANCHES = 3, 1000
MAX_DRAWS = 8                                                           # of a case's state, from the case's one generator


def names(t):
    shaped = ['strip1', 'strip2', 'renumbered', 'mixed', 'curved', 'aniso'] + (['delaunay'] if t[0] == 'P' else [])
    return shaped + ['block256', 'block257', 'block255']


def cases():
    return [(m, t, r, n) for m in MODELS for t in TYPES for r in ROUTES[t] for n in names(t)]


def seed(model, t, name):
    return zlib.crc32(f'{model} {t} {name}'.encode())


def flags(t, name):
    """(per-point materials, initial strain, accept) of the case: the bits of its number."""
    k = TYPES.index(t) + names(t).index(name)
    return bool(k & 1), bool(k & 2), bool(k & 4)


def curve_id(model, t, name):
    """The hardening curve of a 'vmi' case: an entry of CURVES by the case's number (the one `flags` reads)."""
    return CURVES[(TYPES.index(t) + names(t).index(name)) % len(CURVES)] if model == 'vmi' else None


def curve_of(model, t, name):
    """(kappa, slope) of the case as set_hardening takes them, or None: the other models, and the 'vmi' cases that leave the
    context's default curve in place (the restatement runs those on FLAT)."""
    c = curve_id(model, t, name)
    return None if c is None else vmi_cases.curve(c)


def mesh(t, name, rng):
    """(elem, coord)"""
    if not name.startswith('block'):
        return meshes.named(t, name, rng)[:2]
    n_e = int(name[5:])
    ny = (8 if t[0] == 'P' else 16) if n_e != 257 else (3 if t[0] == 'P' else 6)
    elem, coord = meshes.rect(t, 43 if n_e == 257 else 16, ny)
    coord = meshes.jitter(elem, coord, 0.1, rng)
    assert 0 <= elem.shape[1] - n_e <= 1
    return meshes.drop_last(elem, elem.shape[1] - n_e), coord


def state(model, t, elem, coord, rng, curve=None):
    """(U, ep, per-point materials, e0): every draw is made whatever the case's flags select.  `curve` ('vmi' alone) sets the
    range of kappa."""
    ref = ElemRef(elem, coord, fep.element_tables(t))
    n = ref.n_int
    U = rng.normal(0, 1.0, size=(2, coord.shape[1]))
    if model == 'vm':
        nrm = vm_return_map(ref.strain(U)[0], None, *UNIFORM['vm'])['crit'] + YIELD
        U *= YIELD / np.median(nrm)                                         # the median point sits on the yield surface
        ep = traceless(rng, n, 0.1 * YIELD / (2 * SHEAR))
        f = rng.uniform(0.6, 1.4, n)
        per_point = (SHEAR * f, BULK * f[::-1], HARDENING * rng.uniform(0, 2, n), YIELD * rng.uniform(0.6, 1.4, n))
        e0 = rng.normal(0, 0.2 * YIELD / (2 * SHEAR), size=(4, 1))
    elif model == 'vmi':
        flat = vmi_return_map(ref.strain(U)[0], None, *UNIFORM['vmi'], FLAT)
        U *= 1.5 * YIELD / np.median(flat['crit'] + YIELD)
        last = 0.0 if curve is None else float(curve[0][-1])
        ep = vmi_cases.state_rows(rng, n, 0.1 * YIELD / (2 * SHEAR), 1.3 * last if last > 0 else KAPPA_ONE_SEGMENT)
        f = rng.uniform(0.6, 1.4, n)
        per_point = (SHEAR * f, BULK * f[::-1], HARDENING * rng.uniform(0, 2, n), YIELD * rng.uniform(0.6, 1.4, n))
        e0 = rng.normal(0, 0.2 * YIELD / (2 * SHEAR), size=(4, 1))
    else:
        x = coord[0] - coord[0].min()
        U *= 0.5 + 3.5 * x / x.max()                                        # eightfold from left to right: the apex on the right
        k0 = 2 * COHESION * np.sqrt(1 - SIN_PHI ** 2)
        r = mc_return_map(ref.strain(U)[0], None, *UNIFORM['mc'])
        U *= k0 / np.median(r['f'] + k0)
        ep = EPS_Y * rng.normal(0, 0.25, size=(4, n))
        ep[[0, 1, 3]] -= (ep[0] + ep[1] + ep[3]) / 3 * rng.uniform(0.8, 1.0, n)
        f = rng.uniform(0.6, 1.4, n)
        per_point = (P_SHEAR * f, P_BULK * f[::-1], rng.uniform(0.2, 0.6, n), COHESION * rng.uniform(0.6, 1.4, n))
        e0 = EPS_Y * rng.normal(0, 0.2, size=(4, 1))
    return U, ep, per_point, e0


def build(model, t, name):
    """-> dict elem, coord, U, ep, mats, e0 (or None), accept, draw, curve ((kappa, slope) or None) of the case, the same on
    every route: the mesh, then the
    first state drawn from the case's generator that meets check_conditions on the float64 reference strain, with and
    without the previous plastic strain (as test_mc_gpu._case takes the first seed that keeps the floors).  With uniform
    materials the apex, at 2.7 c, is reached by 1 to 5 of the 1152 points of a P1 mesh, so a draw may miss the three points
    a branch has to have; the draw that is taken is decided here, on the restatement, before any kernel runs."""
    rng = np.random.default_rng(seed(model, t, name))
    elem, coord = mesh(t, name, rng)
    pp, with_e0, accept = flags(t, name)
    ref = ElemRef(elem, coord, fep.element_tables(t))
    one = np.ones(ref.n_int)
    curve = curve_of(model, t, name)
    for draw in range(MAX_DRAWS):
        U, ep, per_point, e0 = state(model, t, elem, coord, rng, curve)
        mats = per_point if pp else tuple(v * one for v in UNIFORM[model])
        c = dict(elem=elem, coord=coord, U=U, ep=ep, mats=mats, e0=e0 if with_e0 else None, accept=accept, draw=draw,
                 curve=curve)
        try:
            E = ref.strain(U)[0]
            for p in (ep, None):
                r = return_map(model, E, p, mats, c['e0'], False, curve)
                check_conditions(model, r, excluded(model, r, mats, curve), curve)
            return c
        except AssertionError:
            continue
    raise AssertionError(f'{model} {t} {name}: no state in {MAX_DRAWS} draws meets the conditions')


def return_map(model, E, ep, mats, e0, accept, curve=None):
    """The model's restatement on the strain E; 'n_smooth' / 'n_apex' as a context's step counts them.  'vmi' runs on `curve`
    (None: FLAT) and also returns 'seg0', the segment kappa starts in, 'kappa_new', the kappa an accepting call leaves
    (the restatement's own sum kappa + lam, whether or not this call accepts), and 'with_state'."""
    if model == 'vm':
        r = vm_return_map(E, ep, *mats, apply_plastic_strain=accept, e0=e0)
        return dict(r, n_smooth=r['n_plast'], n_apex=0, branch=r['ind_p'].astype(np.int64))
    if model == 'vmi':
        crv = FLAT if curve is None else curve
        r = vmi_return_map(E, ep, *mats, crv, apply_plastic_strain=accept, e0=e0)
        k0 = np.zeros(np.shape(E)[1]) if ep is None else np.asarray(ep, dtype=float)[3]
        with np.errstate(invalid='ignore'):
            seg0 = np.clip(np.searchsorted(crv[0], k0, side='right') - 1, 0, None)
            return dict(r, n_smooth=r['n_plast'], n_apex=0, branch=r['ind_p'].astype(np.int64), seg0=seg0,
                        kappa_new=k0 + r['lam'], with_state=ep is not None)
    return mc_return_map(E, ep, *mats, apply_plastic_strain=accept, e0=e0)


def excluded(model, ref, mats, curve=None):
    """The points at which rounding of the strain may decide the flag or (Mohr-Coulomb) amplify into the tangent; 'vmi': the
    flag, or the segment an accepted kappa lands in (the tangent jumps at a breakpoint)."""
    if model == 'vm':
        return np.abs(ref['crit']) < VM_CRIT_FLOOR * np.asarray(mats[3])
    if model == 'vmi':
        out = np.abs(ref['crit']) < vmi_cases.CRIT_FLOOR * np.asarray(mats[3])
        for b in (FLAT if curve is None else curve)[0][1:]:
            out = out | (ref['ind_p'] & ~(np.abs(ref['kappa_new'] - b) > vmi_cases.BREAK_FLOOR))
        return out
    return (ref['r_rel'] < R_FLOOR) | (ref['dist'] < DIST_FLOOR)


def check_conditions(model, ref, excl, curve=None):
    """What a case must reach, on the restatement `ref` of its return map: conditions of the generator, not of a kernel.
    'vmi' on a curve of several segments, from N_INT_ALL_BRANCHES points on and with the case's state (a step from kappa = 0
    starts every point in the first segment): every segment accepted by MIN_PER_BRANCH plastic points, as many that end in a
    later segment than they started in, and as many in a softening segment where the curve has one."""
    n = excl.size
    assert excl.mean() <= MAX_EXCLUDED, ('excluded', int(excl.sum()), n)
    if model in ('vm', 'vmi'):
        assert 0.2 <= ref['ind_p'].mean() <= 0.8, ('plastic share', ref['ind_p'].mean())
        if model == 'vmi' and curve is not None and len(curve[0]) > 1 and n >= N_INT_ALL_BRANCHES and ref['with_state']:
            seg = ref['seg'][ref['ind_p']]
            per_segment = np.bincount(seg, minlength=len(curve[0]))
            assert per_segment.min() >= MIN_PER_BRANCH, ('points per segment', per_segment)
            crossed = int((seg > ref['seg0'][ref['ind_p']]).sum())
            assert crossed >= MIN_PER_BRANCH, ('crossed a breakpoint', crossed)
            for j in np.flatnonzero(np.asarray(curve[1]) < 0):
                assert per_segment[j] >= MIN_PER_BRANCH, ('softening segment', j, per_segment)
    elif n >= N_INT_ALL_BRANCHES:
        per_branch = np.bincount(ref['branch'], minlength=5)
        assert per_branch.min() >= MIN_PER_BRANCH, ('points per branch', per_branch)

"""Shared by test_model_step_cases_host.py and test_model_step_routes_gpu.py: the case grid of the von Mises and
Mohr-Coulomb steps (model x element type x route x mesh), the meshes, the state of every case and the conditions a case has
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
the case's number, so that all eight combinations occur for every model.  The generator is seeded from the model, the type
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

MODELS = ('vm', 'mc')
TYPES = ('P1', 'P2', 'Q1', 'Q2', 'P4')
ROUTES = {'P1': ('node', 'patch', 'coo'), 'P2': ('default', 'coo'), 'Q1': ('default', 'coo'), 'Q2': ('default', 'coo'),
          'P4': ('default', 'coo')}
NQ = {'P1': 1, 'P2': 7, 'Q1': 4, 'Q2': 9, 'P4': 12}
BLOCK = 256                                                             # lanes per workgroup of the point kernels (kBlock)
UNIFORM = {'vm': (SHEAR, BULK, HARDENING, YIELD), 'mc': (P_SHEAR, P_BULK, SIN_PHI, COHESION)}
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


def state(model, t, elem, coord, rng):
    """(U, ep, per-point materials, e0): every draw is made whatever the case's flags select."""
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
    """-> dict elem, coord, U, ep, mats, e0 (or None), accept, draw of the case, the same on every route: the mesh, then the
    first state drawn from the case's generator that meets check_conditions on the float64 reference strain, with and
    without the previous plastic strain (as test_mc_gpu._case takes the first seed that keeps the floors).  With uniform
    materials the apex, at 2.7 c, is reached by 1 to 5 of the 1152 points of a P1 mesh, so a draw may miss the three points
    a branch has to have; the draw that is taken is decided here, on the restatement, before any kernel runs."""
    rng = np.random.default_rng(seed(model, t, name))
    elem, coord = mesh(t, name, rng)
    pp, with_e0, accept = flags(t, name)
    ref = ElemRef(elem, coord, fep.element_tables(t))
    one = np.ones(ref.n_int)
    for draw in range(MAX_DRAWS):
        U, ep, per_point, e0 = state(model, t, elem, coord, rng)
        mats = per_point if pp else tuple(v * one for v in UNIFORM[model])
        c = dict(elem=elem, coord=coord, U=U, ep=ep, mats=mats, e0=e0 if with_e0 else None, accept=accept, draw=draw)
        try:
            E = ref.strain(U)[0]
            for p in (ep, None):
                r = return_map(model, E, p, mats, c['e0'], False)
                check_conditions(model, r, excluded(model, r, mats))
            return c
        except AssertionError:
            continue
    raise AssertionError(f'{model} {t} {name}: no state in {MAX_DRAWS} draws meets the conditions')


def return_map(model, E, ep, mats, e0, accept):
    """The model's restatement on the strain E; 'n_smooth' / 'n_apex' as a context's step counts them."""
    if model == 'vm':
        r = vm_return_map(E, ep, *mats, apply_plastic_strain=accept, e0=e0)
        return dict(r, n_smooth=r['n_plast'], n_apex=0, branch=r['ind_p'].astype(np.int64))
    return mc_return_map(E, ep, *mats, apply_plastic_strain=accept, e0=e0)


def excluded(model, ref, mats):
    """The points at which rounding of the strain may decide the flag or (Mohr-Coulomb) amplify into the tangent."""
    if model == 'vm':
        return np.abs(ref['crit']) < VM_CRIT_FLOOR * np.asarray(mats[3])
    return (ref['r_rel'] < R_FLOOR) | (ref['dist'] < DIST_FLOOR)


def check_conditions(model, ref, excl):
    """What a case must reach, on the restatement `ref` of its return map: conditions of the generator, not of a kernel."""
    n = excl.size
    assert excl.mean() <= MAX_EXCLUDED, ('excluded', int(excl.sum()), n)
    if model == 'vm':
        assert 0.2 <= ref['ind_p'].mean() <= 0.8, ('plastic share', ref['ind_p'].mean())
    elif n >= N_INT_ALL_BRANCHES:
        per_branch = np.bincount(ref['branch'], minlength=5)
        assert per_branch.min() >= MIN_PER_BRANCH, ('points per branch', per_branch)

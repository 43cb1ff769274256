"""Shared by test_e0_field_host.py and test_e0_field_gpu.py: the case grid of the steps with an initial strain per point
(model x element type x route x mesh), the state of every case and the conditions it has to meet, built as
tests/model_step_cases.py builds its cases: the first draw of the case's generator that meets `check_conditions` on the
float64 reference strain, decided on the CPU (test_e0_field_host.py) before a kernel meets it.

Meshes: per type the three block-edge meshes of model_step_cases.py (255, 256, 257 elements: n_int modulo the point kernels'
256 lanes is 256 - NQ, 0 and NQ) and one unstructured named mesh ('delaunay' for the triangles, 'renumbered' for the
quadrilaterals).  State: model_step_cases.state for von Mises, Mohr-Coulomb and 'vmi' (isotropic hardening: on one of the five
curves of that module, by the case's number; the field is scaled by the von Mises yield strain), its von Mises generator restated for
Drucker-Prager (a random displacement scaled so that the median point sits on the cone).  The field is eps_y * normal(0, 0.2),
drawn independently in all four rows and at every point, so that a wrong row stride or point index cannot cancel; in half of
the cases it is combined with a non-zero uniform e0 and scale = 0.37, in the others it stands alone with scale = 1.
Per-point materials and accepting calls as model_step_cases.flags has them."""
import zlib

import numpy as np

import e0_field_ref as fref
import model_step_cases as cases
from conftest import dp_materials
from elem_ref import ElemRef
from mc_cases import EPS_Y
from vm_cases import SHEAR, YIELD, fep

MODELS = ('dp', 'vm', 'mc', 'vmi')
TYPES, ROUTES, NQ, BLOCK = cases.TYPES, cases.ROUTES, cases.NQ, cases.BLOCK
MAX_EXCLUDED, MAX_DRAWS = cases.MAX_EXCLUDED, cases.MAX_DRAWS
DP_CRIT_FLOOR = cases.VM_CRIT_FLOOR                                      # |crit1|, |crit2| over c: the von Mises floor
SCALE = 0.37
MESH_FREE_N = (1, 255, 256, 257)


def names(t):
    return ['block255', 'block256', 'block257', 'delaunay' if t[0] == 'P' else 'renumbered']


def grid():
    return [(m, t, r, n) for m in MODELS for t in TYPES for r in ROUTES[t] for n in names(t)]


def seed(model, t, name):
    return zlib.crc32(f'field {model} {t} {name}'.encode())


def flags(model, t, name):
    """(per-point materials, uniform part and scale 0.37, accept)"""
    k = MODELS.index(model) + TYPES.index(t) + names(t).index(name)
    return bool(k & 1), bool(k & 2), bool(k & 4)


def curve_id(model, t, name):
    """The hardening curve of a 'vmi' case (model_step_cases.CURVES), by the case's number as in that module."""
    return cases.CURVES[(TYPES.index(t) + names(t).index(name)) % len(cases.CURVES)] if model == 'vmi' else None


def curve_of(model, t, name):
    c = curve_id(model, t, name)
    return None if c is None else cases.vmi_cases.curve(c)


MESH_FREE_CURVE = 2                                                      # of the mesh-free 'vmi' points


def eps_y(model):
    if model in ('vm', 'vmi'):
        return YIELD / (2 * SHEAR)
    if model == 'mc':
        return EPS_Y
    sh, _, _, c = dp_materials(1)
    return float(c[0] / (2 * sh[0]))


def dp_state(elem, coord, ref, rng):
    """(U, ep, per-point materials, e0) of a Drucker-Prager case: the median point on the cone."""
    n = ref.n_int
    sh, bu, eta, c = (float(v[0]) for v in dp_materials(1))
    U = rng.normal(0, 1.0, size=(2, coord.shape[1]))
    E = ref.strain(U)[0]
    one = np.ones(n)
    crit1, _ = fref.dp_crits(E, None, (sh * one, bu * one, eta * one, c * one), np.zeros((4, n)))
    U *= c / np.median(crit1 + c)                                       # crit1 + c is homogeneous of degree one in U
    ey = c / (2 * sh)
    ep = cases.traceless(rng, n, 0.1 * ey)
    f = rng.uniform(0.6, 1.4, n)
    per_point = (sh * f, bu * f[::-1], eta * rng.uniform(0.6, 1.4, n), c * rng.uniform(0.6, 1.4, n))
    e0 = rng.normal(0, 0.2 * ey, size=(4, 1))
    return U, ep, per_point, e0


def uniform(model, n):
    if model == 'dp':
        return dp_materials(n)
    return tuple(v * np.ones(n) for v in cases.UNIFORM[model])


def excluded(model, r, mats, curve=None):
    """The points at which rounding of the strain may decide the flag (or, Mohr-Coulomb, amplify into the tangent; 'vmi': the
    segment of the curve)."""
    if model == 'dp':
        c = np.asarray(mats[3])
        return (np.abs(r['crit1']) < DP_CRIT_FLOOR * c) | ((r['crit1'] > 0) & (np.abs(r['crit2']) < DP_CRIT_FLOOR * c))
    return cases.excluded(model, r, mats, curve)


def check_conditions(model, r, excl, curve=None):
    assert excl.mean() <= MAX_EXCLUDED, ('excluded', int(excl.sum()), excl.size)
    if model == 'dp':
        assert 0.2 <= r['ind_p'].mean() <= 0.8, ('plastic share', r['ind_p'].mean())
    else:
        cases.check_conditions(model, r, excl, curve)


_BUILT = {}


def build(model, t, name):
    """-> dict elem, coord, U, ep, mats, e0 (or None), field, scale, accept, draw, curve ('vmi': (kappa, slope) or None for
    the context's default; None for the other models): the same on every route, computed once
    per session and never modified by the tests (they copy what a call updates)."""
    key = (model, t, name)
    if key in _BUILT:
        return _BUILT[key]
    rng = np.random.default_rng(seed(model, t, name))
    elem, coord = cases.mesh(t, name, rng)
    pp, with_e0, accept = flags(model, t, name)
    ref = ElemRef(elem, coord, fep.element_tables(t))
    n = ref.n_int
    curve = curve_of(model, t, name)
    for draw in range(MAX_DRAWS):
        U, ep, per_point, e0 = dp_state(elem, coord, ref, rng) if model == 'dp' else cases.state(model, t, elem, coord, rng, curve)
        field = eps_y(model) * rng.normal(0, 0.2, size=(4, n))
        mats = per_point if pp else uniform(model, n)
        c = dict(elem=elem, coord=coord, U=U, ep=ep, mats=mats, e0=e0 if with_e0 else None, field=field,
                 scale=SCALE if with_e0 else 1.0, accept=accept, draw=draw, curve=curve)
        try:
            E = ref.strain(U)[0]
            z = fref.z_of(c['e0'], field, c['scale'])
            for p in (ep, None):
                r = fref.return_map(model, E, p, mats, z, False, curve=curve)
                check_conditions(model, r, excluded(model, r, mats, curve), curve)
            _BUILT[key] = c
            return c
        except AssertionError:
            continue
    raise AssertionError(f'{model} {t} {name}: no state in {MAX_DRAWS} draws meets the conditions')


def mesh_free(model, n, seed_):
    """Mesh-free points of `model`: (E (3, n), ep, mats, e0, field) around the yield surface, per-point materials; 'vmi': kappa
    spread over curve MESH_FREE_CURVE."""
    rng = np.random.default_rng(zlib.crc32(f'mesh-free {model} {n} {seed_}'.encode()))
    ey = eps_y(model)
    E = ey * rng.normal(0, 1.5, size=(3, n))
    ep = cases.traceless(rng, n, 0.1 * ey)
    f = rng.uniform(0.6, 1.4, n)
    u = uniform(model, n)
    third = rng.uniform(0.2, 0.6, n) if model == 'mc' else u[2] * rng.uniform(0.6, 1.4, n)
    mats = (u[0] * f, u[1] * f[::-1], third, u[3] * rng.uniform(0.6, 1.4, n))
    e0 = rng.normal(0, 0.2 * ey, size=(4, 1))
    field = ey * rng.normal(0, 0.2, size=(4, n))
    if model == 'vmi':
        ep[3] = rng.uniform(0, 1.3 * cases.vmi_cases.curve(MESH_FREE_CURVE)[0][-1], n)
    return E, ep, mats, e0, field


# ---- K0 box: a rectangle at rest under self-weight -------------------------------------------------------------------------
# The identity the box rests on, B^T w s0 = f_V at the free DOFs, is exact only where the tabulated quadrature integrates the
# products exactly.  The tables of P1 (one point) and Q1 (2 x 2 Gauss points computed to the last bit) do, to rounding; the P2
# and P4 tables carry the reference's 13-digit points and integrate the monomials up to degree 3 to 1.4e-13 and 5.6e-13 only
# (quadrature_defect, asserted by test_e0_field_host.py), a thousand times the assembly bound.  So the box is set on the
# two types whose table is shown exact there (Q2's nine-point rule is not a tensor Gauss rule and is left out with P2 and P4).
K0_TYPES = ('P1', 'Q1')


def quadrature_defect(t, degree=3):
    """Largest relative error of the tabulated rule of type t on the monomials x^i y^j, i + j <= degree (quadrilaterals: i, j
    <= degree each), against the exact integral over the reference element."""
    from math import factorial
    tt = fep.LagrangeElementType[t]
    xi, wf = fep.get_quadrature_volume(tt)
    xi, wf = np.asarray(xi, dtype=float), np.asarray(wf, dtype=float).ravel()
    worst = 0.0
    for i in range(degree + 1):
        for j in range(degree + 1):
            if t[0] == 'P':
                if i + j > degree:
                    continue
                exact = factorial(i) * factorial(j) / factorial(i + j + 2)
            else:
                exact = (0.0 if i % 2 else 2.0 / (i + 1)) * (0.0 if j % 2 else 2.0 / (j + 1))
            got = float((wf * xi[0] ** i * xi[1] ** j).sum())
            worst = max(worst, abs(got - exact) / (exact if exact else 1.0))
    return worst
K0, P_TOP, GAMMA, Y_TOP = 0.8, 20.0, 0.3, 50.0


def k0_box(t):
    """[-50, 50]^2 without a hole (the TSX driver puts rollers on its four sides), affine elements: triangles with their
    vertices jittered (P2 raised afterwards, so that its sides stay straight), quadrilaterals as the rectangles they are.
    -> dict elem, coord, in_situ (linear, vertical gradient), body_force = (0, -grad_22), materials in two layers (per
    point, by the height of the point), s0 (4, n_int) of the float64 point coordinates."""
    import meshes
    rng = np.random.default_rng(zlib.crc32(f'k0 {t}'.encode()))
    if t[0] == 'P':
        elem, coord = meshes.rect('P1', 6, 5, 100.0, 100.0)
        coord = meshes.jitter(elem, coord, 0.2, rng)
        if t != 'P1':
            elem, coord = meshes.raise_p1(t, elem, coord)
    else:
        elem, coord = meshes.rect(t, 6, 5, 100.0, 100.0)
    coord = coord - 50.0
    in_situ = fep.linear_in_situ((-K0 * P_TOP, -P_TOP, 0.0, -K0 * P_TOP), Y_TOP, (K0 * GAMMA, GAMMA, 0.0, K0 * GAMMA))
    xq = fref.point_coords(fep, t, elem, coord)[0]
    n = xq.shape[1]
    young, nu = 60000, 0.2                                              # newton._tsx_setup
    fr = 49 * np.pi / 180
    stiff = np.where(xq[1] < 0, 3.0, 1.0)
    mats = (young / (2 * (1 + nu)) * stiff, young / (3 * (1 - 2 * nu)) * stiff,
            3 * np.tan(fr) / np.sqrt(9 + 12 * np.tan(fr) ** 2) * np.ones(n), 3 * 18.7 / np.sqrt(9 + 12 * np.tan(fr) ** 2) * np.ones(n))
    return dict(elem=elem, coord=coord, in_situ=in_situ, body_force=(0.0, -GAMMA), mats=mats, s0=in_situ(xq[0], xq[1]), xq=xq)

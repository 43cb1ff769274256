"""Shared by test_plastic_exact_host.py and test_plastic_exact_gpu.py: load histories whose finite-element solution is known
in closed form for every material model, through the whole stack (step, assembly, solver, newton._load_history_loop).

A homogeneous stress state whose deviator keeps its direction is the plastic patch test.  The isoparametric elements
reproduce a linear displacement exactly, so the strain is one value at every integration point; the return maps are radial
(or a projection along one fixed normal), so backward Euler is exact at any step size; and the load vector is the free-DOF
part of `internal_force` of the case's unit stress (as test_vmps_step_gpu._uniaxial_problem builds it), so the uniform stress
is in discrete equilibrium whatever the quadrature does.  The discrete solution on any mesh of any type is then the linear
field of a scalar, piecewise-linear law that is written down below in plain Python floats, independently of newton.py, of the
contexts and of the look-alikes.  What the loop accepts, what it carries from step to step and what crosses a refinement all
show in U and in the plastic state.

Case S, pure shear: sigma = (t, -t, 0, 0), models 'vm', 'vmi', 'vmps'  (shear_law).
Case C, confined compression: top pressure q, rollers on both sides and the bottom, models 'dp', 'mc'  (confined_law).

Meshes: the 3 x 2 cell rectangle 4 x 2 of every type of model_step_cases.TYPES, jittered by 0.25 of the node spacing (P4: 0.2)
from np.random.default_rng(1), so that P2 / Q2 / P4 elements are curved; for P1 and Q1 also a mesh of 264 and 288 integration
points ('block': the second 256-lane workgroup of the point kernels is partial).  ONE exclusion: case C on Q2 runs on the
unjittered rectangle.  The 8-node element's inherited quadrature rule does not integrate the derivatives of its shape
functions exactly on a curved element, so a uniform sigma_11 — which in case C should load only the constrained side DOFs —
leaves forces of 3 to 19 % on free interior DOFs, already in the elastic steps (case S has no such component: its whole
stress is the unit stress of f_ext).

Histories are lists of the load factor itself (t, or q).  Their conditions (check_history) are asserted from the closed form
alone: no step within MARGIN_CROSSING of a yield or breakpoint crossing, every segment of the curve accepted by a step, and an
elastic step directly after a plastic one.  'vmi' curves keep Y + R(kappa) > 0 and a + slope > 0 along the history: with a
softening total modulus the load could not be prescribed.

The 'vmi' cycle is named 'stall': on the P1 and P4 meshes its step 13, the first purely elastic unloading step after the reverse
plastic excursion, was not converged by 25 Newton iterates of newton._load_history_loop before that loop learned to retry a
step from K_elast.  RETRIES names the steps of 'stall' that the CPU look-alike retries, per type.  The other
histories meet the same stall (the 'vm' and 'vmps' cycles at step 5 on most meshes, 'mono8' at its last step on P1 and P4): which
mesh does is decided by rounding, so for those the tests assert only where a retry may happen at all, at an elastic step directly
after a plastic one."""
import math
from importlib import import_module

import numpy as np

import meshes
import mc_cases
import vm_cases
from model_step_cases import NQ, TYPES
from return_map_mp_cases import MARGIN, UNIT  # noqa: F401  (MARGIN: the project's 8x rule, used by both test modules)

fep = import_module('fem-elastoplasticity_amd')

SQRT2 = math.sqrt(2.0)
SIZE = (4.0, 2.0)
JITTER = {'P1': 0.25, 'P2': 0.25, 'Q1': 0.25, 'Q2': 0.25, 'P4': 0.2}
BLOCK_CELLS = {'P1': (12, 11), 'Q1': (9, 8)}                               # 264 elements x 1 point, 72 elements x 4 points
MARGIN_CROSSING = 1e-3
MASK_TOL = 1e-9                                                            # of the rectangle's size: which side a node lies on

MODELS = {'S': ('vm', 'vmi', 'vmps'), 'C': ('dp', 'mc')}
UNIT_STRESS = {'S': (1.0, -1.0, 0.0, 0.0), 'C': (0.0, -1.0, 0.0, 0.0)}

# case S: the materials of the cyclic benchmark (vm_cases); 'vmi' adds a hardening curve
S_MATERIALS = (vm_cases.SHEAR, vm_cases.BULK, vm_cases.HARDENING, float(vm_cases.YIELD))
CURVE3 = ((0.0, 2e-3, 8e-3), (40000.0, 8000.0, 1000.0))
CURVE8 = ((0.0, 1e-3, 2e-3, 4e-3, 6e-3, 9e-3, 1.3e-2, 1.8e-2), (40000.0, 30000.0, 20000.0, 14000.0, 9000.0, 5000.0, 2500.0, 1000.0))
PEAK = 1.27 * float(vm_cases.YIELD) / SQRT2
CYCLE = tuple(PEAK * f for f in np.concatenate([np.linspace(0, 1, 6)[1:], np.linspace(1, -1.2, 9)[1:],
                                                np.linspace(-1.2, 1.3, 9)[1:]]))

# case C: the strip footing's Young's modulus, friction angle and cohesion, but Poisson's ratio 0.25.  In confined compression
# the stress ratio is nu / (1 - nu); with the reference's nu = 0.48 it is 0.92 and no pressure ever reaches either yield
# surface: Mohr-Coulomb yields only if nu / (1 - nu) < (1 - sin phi) / (1 + sin phi) = 0.49.
C_YOUNG, C_POISSON, C_PHI, C_COHESION = 1e7, 0.25, math.pi / 9, 450.0
C_SHEAR = C_YOUNG / (2 * (1 + C_POISSON))
C_BULK = C_YOUNG / (3 * (1 - 2 * C_POISSON))
C_MATERIALS = {'dp': (C_SHEAR, C_BULK, 3 * math.tan(C_PHI) / math.sqrt(9 + 12 * math.tan(C_PHI) ** 2),
                      3 * C_COHESION / math.sqrt(9 + 12 * math.tan(C_PHI) ** 2)),
               'mc': (C_SHEAR, C_BULK, math.sin(C_PHI), C_COHESION)}
C_FACTORS = (0.4, 0.8, 1.3, 1.7, 1.4, 1.1, 1.5, 1.9, 2.2)                  # of the pressure at first yield: load, unload, reload


# ---------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------
def shear_law(ts, shear, a, Y, curve=None, kappa_row=False):
    """Pure shear sigma = (t, -t, 0, 0) under load control, for the three von Mises models.

    The stress is its own deviator and has no 33 component, so the plastic strain is p = (pi, -pi, 0, 0): traceless with
    p33 = 0.  From the statements of include/fep.h: the relative stress is xi = s - a p = (t - a pi)(1, -1, 0, 0), with the norm
    |xi| = sqrt(2) |t - a pi|; write x = sqrt(2) (t - a pi).  The step is elastic while |x| <= Y + R(kappa).  Otherwise the
    radial return moves p along N = xi / |xi| = sign(x) (1, -1, 0, 0) / sqrt(2) by the multiplier dl > 0: d pi = sign(x) dl /
    sqrt(2), d kappa = dl, which lowers |x| by a dl, and dl is the root of  |x| - a dl = Y + R(kappa + dl).  R is piecewise
    linear: from the segment kappa starts in, dl = (|x| - Y - R_j - slope_j (kappa - kappa_j)) / (a + slope_j), accepted in
    the first segment j whose end kappa + dl does not pass.  The strain is eps = t / 2G + pi (the elastic part of a pure deviator
    plus the plastic one), eps_22 = -eps, and U = (eps x, -eps y).

    'vmps' (plane stress) obeys the same scalar law: with tr sigma = 0 and s33 = 0 the plane-stress constraint sigma_33 = 0 is
    met by the plane-strain solution itself (eps_33 = -nu (s11 + s22) / E + p33 = 0), the projected norm sqrt(eta^T P eta) of a
    traceless in-plane eta is its 3-D norm, and the flow (pi, -pi, 0) keeps p33 = -(p11 + p22) = 0.  'vm' is the law with R = 0.

    -> one dict per t: load, strain (e11, e22, g12), stress (4), ep (4: row 3 is kappa with `kappa_row`, the 'vmi' state, else
    p33 = 0), plastic, seg (the accepted segment, -1 elastic), margin (the relative distance to the nearest crossing)."""
    kap, slo = ((0.0,), (0.0,)) if curve is None else curve
    R = [0.0]
    for j in range(1, len(kap)):
        R.append(R[-1] + slo[j - 1] * (kap[j] - kap[j - 1]))
    assert all(a + h > 0 for h in slo), 'load control needs a + slope > 0'
    pi = kappa = 0.0
    rows = []
    for t in ts:
        x = SQRT2 * (t - a * pi)
        j = max(i for i in range(len(kap)) if kap[i] <= kappa)
        radius = Y + R[j] + slo[j] * (kappa - kap[j])
        assert radius > 0
        plastic = abs(x) > radius
        margin = abs(abs(x) - radius) / radius
        if plastic:
            while True:
                dl = (abs(x) - (Y + R[j] + slo[j] * (kappa - kap[j]))) / (a + slo[j])
                if j + 1 == len(kap) or kappa + dl <= kap[j + 1]:
                    break
                j += 1
            kappa += dl
            pi += math.copysign(dl, x) / SQRT2
            margin = min([margin] + [abs(kappa - b) / b for b in kap[1:]])
        eps = t / (2 * shear) + pi
        rows.append(dict(load=t, strain=(eps, -eps, 0.0), stress=(t, -t, 0.0, 0.0), ep=(pi, -pi, 0.0, kappa if kappa_row else 0.0),
                         plastic=plastic, seg=j if plastic else -1, margin=margin))
    return rows


def _yield_value(model, s11, s22, m3, m4):
    """The yield function of 'dp' / 'mc' at the stress (s11, s22, 0, s33 = s11)."""
    if model == 'dp':                                                      # rho / sqrt2 + eta sigma_m - c
        m = (2 * s11 + s22) / 3
        rho = math.sqrt(2 * (s11 - m) ** 2 + (s22 - m) ** 2)
        return rho / SQRT2 + m3 * m - m4
    hi, lo = max(s11, s22), min(s11, s22)                                  # (1 + s) sig_1 - (1 - s) sig_3 - 2 c cos(phi)
    return (1 + m3) * hi - (1 - m3) * lo - 2 * m4 * math.sqrt(1 - m3 * m3)


def first_yield_pressure(model):
    """The pressure at which the elastic path sigma = -q (k0, 1, 0, k0), k0 = nu / (1 - nu), meets the yield surface."""
    G, K, m3, m4 = C_MATERIALS[model]
    k0 = (K - 2 * G / 3) / (K + 4 * G / 3)
    slope = _yield_value(model, -k0, -1.0, m3, 0.0)                        # the yield function is linear along the ray
    assert slope > 0, 'the material never yields in confined compression'
    return (m4 if model == 'dp' else 2 * m4 * math.sqrt(1 - m3 * m3)) / slope


def confined_law(qs, model, shear, bulk, m3, m4):
    """Confined compression under load control: eps_11 = eps_33 = gamma_12 = 0, sigma_22 = -q, sigma_11 = sigma_33 by symmetry.

    Both models are perfectly plastic and associative, and the state stays on ONE flat piece of the yield surface with a fixed
    normal d (rows 11, 22, 33), so the plastic strain is p = L d with one scalar L and the closest-point projection is exact at
    any step size:
      'dp'  the smooth cone.  With sigma_m = m and the deviator (|s| / 2, -|s|, |s| / 2): rho = sqrt(3/2) |s|, yield
            sqrt(3) |s| / 2 + eta m = c, and sigma_22 = m - |s| = -q give |s| = (c + eta q) / (sqrt(3) / 2 + eta).  The normal is
            N / sqrt2 + eta / 3: d = (1 / (2 sqrt3) + eta / 3, -1 / sqrt3 + eta / 3, d11).  Every plastic point is counted smooth.
      'mc'  sigma_1 = sigma_2 = sigma_11 = sigma_33 > sigma_3 = sigma_22: the LEFT EDGE (mc_ref: sig1 = sig2), which the mesh
            cases of mc_cases.py cannot reach.  (1 + s) sigma_11 + (1 - s) q = 2 c cos(phi), d = ((1 + s) / 2, -(1 - s), d11).
    While plastic the stress follows from q alone; L from eps_11 = 0 = eps_11^e + L d11; eps_22 = eps_22^e + L d22.  An elastic
    step keeps L: sigma_22 = (K + 4G/3)(eps_22 - p22) - 2 (K - 2G/3) p11 = -q gives eps_22, then sigma_11.  U = (0, eps_22 y).

    -> one dict per q, as shear_law's (seg is 0 for a plastic step)."""
    lam, M = bulk - 2 * shear / 3, bulk + 4 * shear / 3
    if model == 'dp':
        d = (1 / (2 * math.sqrt(3)) + m3 / 3, -1 / math.sqrt(3) + m3 / 3)
    else:
        d = ((1 + m3) / 2, -(1 - m3))
    L = 0.0
    rows = []
    scale = m4 if model == 'dp' else 2 * m4 * math.sqrt(1 - m3 * m3)
    for q in qs:
        p11, p22 = L * d[0], L * d[1]
        e22 = p22 + (-q + 2 * lam * p11) / M
        s11 = lam * (e22 - p22) - (M + lam) * p11
        f = _yield_value(model, s11, -q, m3, m4)
        plastic = f > 0
        if plastic:
            if model == 'dp':
                dev = (m4 + m3 * q) / (math.sqrt(3) / 2 + m3)
                s11 = -q + 1.5 * dev
            else:
                s11 = (2 * m4 * math.sqrt(1 - m3 * m3) - (1 - m3) * q) / (1 + m3)
            assert s11 > -q
            mean = (2 * s11 - q) / 3
            L_new = -((s11 - mean) / (2 * shear) + mean / (3 * bulk)) / d[0]
            assert L_new > L
            L = L_new
            e22 = (-q - mean) / (2 * shear) + mean / (3 * bulk) + L * d[1]
        rows.append(dict(load=q, strain=(0.0, e22, 0.0), stress=(s11, -q, 0.0, s11), ep=(L * d[0], L * d[1], 0.0, L * d[0]),
                         plastic=plastic, seg=0 if plastic else -1, margin=abs(f) / scale))
    return rows


# ---------------------------------------------------------------------------------------
# histories
# ---------------------------------------------------------------------------------------
def _mono8():
    """Monotone loading over the eight-segment curve: an elastic step, the stress at the middle of every segment (of the last
    one: half the last breakpoint past it), t(kappa) = (Y + R(kappa) + a kappa) / sqrt2, and an elastic step back."""
    G, _, a, Y = S_MATERIALS
    kap, slo = CURVE8
    ts, R = [0.5 * Y / SQRT2], 0.0
    for j in range(len(kap)):
        mid = 0.5 * (kap[j] + kap[j + 1]) if j + 1 < len(kap) else 1.5 * kap[j]
        ts.append((Y + R + slo[j] * (mid - kap[j]) + a * mid) / SQRT2)
        if j + 1 < len(kap):
            R += slo[j] * (kap[j + 1] - kap[j])
    return tuple(ts + [0.6 * ts[-1]])


HISTORIES = {('S', 'vm'): ('cycle',), ('S', 'vmps'): ('cycle',), ('S', 'vmi'): ('stall', 'mono8'),
             ('C', 'dp'): ('reload',), ('C', 'mc'): ('reload',)}
STALL_STEP = 13
RETRIES = {'P1': [STALL_STEP], 'P2': [], 'Q1': [], 'Q2': [], 'P4': [STALL_STEP]}   # of 'stall' on the small meshes


def materials(case, model):
    return S_MATERIALS if case == 'S' else C_MATERIALS[model]


def curve_of(model, name):
    """(kappa, slope) that a 'vmi' context's set_hardening takes for the history, else None."""
    if model != 'vmi':
        return None
    return CURVE8 if name == 'mono8' else CURVE3


def loads(case, model, name):
    if case == 'C':
        return tuple(f * first_yield_pressure(model) for f in C_FACTORS)
    return _mono8() if name == 'mono8' else CYCLE


def exact(case, model, name):
    """The closed form of the history: one dict per step (shear_law / confined_law)."""
    G, K, m3, m4 = materials(case, model)
    if case == 'C':
        return confined_law(loads(case, model, name), model, G, K, m3, m4)
    return shear_law(loads(case, model, name), G, m3, m4, curve_of(model, name), kappa_row=model == 'vmi')


def n_segments(model, name):
    c = curve_of(model, name)
    return 1 if c is None else len(c[0])


def check_history(case, model, name):
    """The conditions on a history, from the closed form alone."""
    rows = exact(case, model, name)
    assert min(r['margin'] for r in rows) > MARGIN_CROSSING, [r['margin'] for r in rows]
    assert {r['seg'] for r in rows if r['plastic']} == set(range(n_segments(model, name)))
    flags = [r['plastic'] for r in rows]
    assert any(a and not b for a, b in zip(flags, flags[1:])), 'no elastic step directly after a plastic one'
    if name in ('cycle', 'stall'):                                         # at least two reversals of the plastic flow
        signs = [math.copysign(1.0, r['load']) for r in rows if r['plastic']]
        assert sum(a != b for a, b in zip(signs, signs[1:])) >= 2
    if name == 'reload':                                                   # load, elastic unload, reload past the old maximum
        q = [r['load'] for r in rows]
        top = next(i for i in range(len(q) - 1) if flags[i] and not flags[i + 1])
        again = next(i for i in range(top + 1, len(q)) if flags[i])
        assert q[top] == max(q[:top + 1]) and q[top + 1] < q[top] and q[again] > q[top]
        assert any(q[i] > q[i - 1] and not flags[i] for i in range(top + 2, again)), 'no elastic reloading step'
    return rows


def displacement(case, row, coord):
    """The exact U (2, n_n) of a step: the linear field of the step's strain that the rollers fix."""
    e = row['strain']
    return np.stack([e[0] * coord[0], e[1] * coord[1]])


# ---------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------
def mesh(case, t, size='small'):
    """(elem, coord): the jittered 3 x 2 rectangle, or ('block', P1 and Q1) the mesh whose second workgroup is partial."""
    nx, ny = (3, 2) if size == 'small' else BLOCK_CELLS[t]
    elem, coord = meshes.rect(t, nx, ny, *SIZE)
    if not (case == 'C' and t == 'Q2'):                                    # the one exclusion (module docstring)
        coord = meshes.jitter(elem, coord, JITTER[t], np.random.default_rng(1))
    n_int = elem.shape[1] * NQ[t]
    assert n_int < 511 and (size == 'small' or 257 <= n_int)
    return np.ascontiguousarray(elem, dtype=np.int64), np.ascontiguousarray(coord)


def sizes(t):
    return ('small', 'block') if t in BLOCK_CELLS else ('small',)


def free_mask(case, coord):
    """(2, n_n) bool.  Case S: u_x = 0 on x = 0, u_y = 0 on y = 0.  Case C: u_x = 0 on both vertical sides, u_y = 0 on the bottom.
    A node is on a side when it is within MASK_TOL of it, relative to the rectangle."""
    x, y = coord
    on = lambda v, side, span: np.abs(v - side) <= MASK_TOL * span                  # noqa: E731
    left, right, bottom = on(x, 0.0, SIZE[0]), on(x, SIZE[0], SIZE[0]), on(y, 0.0, SIZE[1])
    assert left.any() and right.any() and bottom.any()
    return np.stack([~(left | right) if case == 'C' else ~left, ~bottom])


def problem(case, t, size='small', on=None):
    """-> dict elem, coord, free (2, n_n), f_ext (2 n_n,) interleaved as the drivers' vectors, n_int.  f_ext is the internal
    force of the case's unit stress at the free DOFs, summed on the host by the pinned CPU assembly.  `on`: (elem, coord) of
    another mesh of the rectangle instead of `mesh(case, t, size)`."""
    from vm_ref import VMRefContext
    elem, coord = mesh(case, t, size) if on is None else on
    ref = VMRefContext(elem, coord, *fep.element_tables(t))
    ref.set_materials(*S_MATERIALS)
    unit = np.array(UNIT_STRESS[case]).reshape(4, 1) * np.ones((1, ref.n_int))
    f = np.asarray(ref.orc.internal_force(ref.c['B'], ref.c['weight'], unit)).ravel()
    free = free_mask(case, coord)
    return dict(elem=elem, coord=coord, free=free, f_ext=np.where(free.flatten(order='F'), f, 0.0), n_int=ref.n_int)


def _DPContext(*a):
    """tests/oracle_context.OracleContext (the Drucker-Prager look-alike) with the `set_model` that make_context calls."""
    from oracle_context import OracleContext

    class DP(OracleContext):
        def set_model(self, model):
            assert model == 'dp'
    return DP(*a)


def lookalike(model):
    """The CPU look-alike context class of a model."""
    if model == 'dp':
        return _DPContext
    name = {'vm': ('vm_ref', 'VMRefContext'), 'vmi': ('vmi_ref', 'VMIRefContext'), 'vmps': ('vmps_ref', 'VMPSRefContext'),
            'mc': ('mc_ref', 'MCRefContext')}[model]
    return getattr(import_module(name[0]), name[1])


def make_context(factory, case, model, name, elem, coord, t):
    ctx = factory(elem, coord, *fep.element_tables(t))
    ctx.set_model(model)
    ctx.set_materials(*materials(case, model))
    if model == 'vmi':
        ctx.set_hardening(*(np.array(v) for v in curve_of(model, name)))
    return ctx


def run(newton, ctx, prob, zetas, solver='direct', U=None, Ep=None, pcg_rtol=1e-11, keep_ops=False):
    """newton._load_history_loop on the context -> hist with, per accepted step, 'U' (2, n_n), 'Ep' (4, n_int), 'ind_p', 'counts'
    (n_smooth, n_apex), 'newton_its', and the loop's own 'failed_at', 'retries', 'n_calls'; 'state' = (U, Ep) as vectors of
    the ops.  `U`, `Ep`: the state to go on from, as arrays (they become vectors of the new ops) or as such vectors.  With
    `keep_ops` the ops stay open as hist['ops'] (the caller closes them); the context is the caller's in any case."""
    hist = {'zeta': [], 'U': [], 'Ep': [], 'ind_p': [], 'counts': [], 'newton_its': [], 'n_calls': 0}
    ops = newton.make_ops(ctx, prob['free'].flatten(order='F'), solver, pcg_rtol)
    try:
        K_elast = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']
        ops.setup_amg(K_elast, prob['coord'])
        if isinstance(U, np.ndarray):
            U = ops.vec(U)
        if isinstance(Ep, np.ndarray):
            Ep = ops.field(np.array(Ep))                                   # a copy: the accepting calls update it in place
        state = [ops.new_ep() if Ep is None else Ep]

        def accepted(r, zeta, U_k, its):
            hist['U'].append(np.array(ops.host(U_k)).reshape((2, -1), order='F').copy())
            hist['Ep'].append(np.array(ops.host(state[0])))
            hist['ind_p'].append(np.array(ops.host(r['ind_p'])).astype(bool).ravel())
            hist['counts'].append((int(r['n_smooth']), int(r['n_apex'])))
            hist['newton_its'].append(its)
        U_end, Ep_end = newton._load_history_loop(ops, K_elast, ops.vec(prob['f_ext']), zetas, hist, accepted=accepted,
                                                  U=U, Ep=state[0])
        hist['state'] = (U_end, Ep_end)
        hist['pcg_iters'] = ops.pcg_iters
    except BaseException:
        ops.close()
        raise
    if keep_ops:
        hist['ops'] = ops
    else:
        ops.close()
    return hist


def errors(case, hist, rows, coord):
    """(U, Ep): the maximum over the accepted steps of |U - U_exact| / max|U_exact|, and of |Ep - Ep_exact| / max|Ep_exact| (a
    state that is exactly zero has to be reproduced exactly: its error counts as absolute)."""
    e_u = e_p = 0.0
    for U, Ep, row in zip(hist['U'], hist['Ep'], rows):
        Ux = displacement(case, row, coord)
        e_u = max(e_u, float(np.abs(U - Ux).max() / np.abs(Ux).max()))
        px = np.array(row['ep']).reshape(4, 1)
        e_p = max(e_p, float(np.abs(Ep - px).max() / (np.abs(px).max() or 1.0)))
    return e_u, e_p


# ---------------------------------------------------------------------------------------
# refinement in the middle of a history (triangles)
# ---------------------------------------------------------------------------------------
REFINED = [(model, t) for model in ('vm', 'vmi') for t in ('P1', 'P2')]
REFINE_AFTER = 4                                                           # the last step of the first loading: plastic
REFINE_HISTORY = {'vm': 'cycle', 'vmi': 'stall'}


def refine_parent():
    """The P1 vertex mesh that is refined, and the marks: the 3 x 2 rectangle with jittered vertices (so that a P2 mesh raised
    from it has straight sides: the children's midside nodes then lie where the parent's shape functions put them), and the
    elements whose centroid lies in the left half, a geometric subset that the closure of the marks has to extend."""
    e1, c1 = meshes.rect('P1', 3, 2, *SIZE)
    c1 = meshes.jitter(e1, c1, JITTER['P1'], np.random.default_rng(1))
    e1 = np.ascontiguousarray(e1, dtype=np.int64)
    marked = c1[0][e1].mean(axis=0) < 0.5 * SIZE[0]
    assert 0 < marked.sum() < marked.size
    return e1, np.ascontiguousarray(c1), marked


def raised(t, e1, c1):
    """(elem, coord) of the P1 vertex mesh as type t."""
    elem, coord = meshes.raise_p1(t, e1, c1)
    return np.ascontiguousarray(elem, dtype=np.int64), np.ascontiguousarray(coord, dtype=float)


def transfer_scale(t):
    """The factor of test_transfer_host.test_polynomials_are_reproduced's per-entry bound, (n_p + 8) u sum_a |W_a| |u_a|, with
    the sum bounded by the largest row sum of |W| times max|u|: -> (n_p + 8) u max_rows sum_a |W_a|."""
    W = np.abs(np.asarray(fep.transfer_tables(t)['W']))
    return (W.shape[-1] + 8) * UNIT * float(W.sum(axis=-1).max())


def check_child_state(t, parent, Ep_parent, Ep_child):
    """Every point of a child carries the state of a point of its parent, bit for bit."""
    nq = NQ[t]
    for ch, par in enumerate(np.asarray(parent)):
        own = Ep_parent[:, par * nq:(par + 1) * nq]
        for k in range(ch * nq, (ch + 1) * nq):
            assert any(Ep_child[:, k].tobytes() == own[:, j].tobytes() for j in range(nq)), (ch, k)


def refined_cpu(newton, model, t):
    """The look-alike's run with the NumPy refinement and transfer (no GPU): the history to REFINE_AFTER on the parent, marked
    refinement, transfer of U and the plastic state, the remaining steps on the children -> dict with the two hists, the
    transferred state, the child problem, the parent numbering and `rows`."""
    name = REFINE_HISTORY[model]
    rows, zetas = exact('S', model, name), loads('S', model, name)
    e1, c1, marked = refine_parent()
    prob = problem('S', t, on=raised(t, e1, c1))
    ctx = make_context(lookalike(model), 'S', model, name, prob['elem'], prob['coord'], t)
    first = run(newton, ctx, prob, zetas[:REFINE_AFTER + 1])
    cc, ec, parent = fep.refine_marked(c1, e1, marked)
    corners = fep.child_corners(c1, e1, marked)
    child = problem('S', t, on=raised(t, ec, cc))
    U_c = fep.transfer_nodes_np(t, prob['elem'], child['elem'], parent, corners, first['U'][-1].T.copy(),
                                n_n_child=child['coord'].shape[1]).reshape(-1)
    Ep_c = fep.transfer_points_np(t, parent, corners, first['Ep'][-1])
    ctx2 = make_context(lookalike(model), 'S', model, name, child['elem'], child['coord'], t)
    rest = run(newton, ctx2, child, zetas[REFINE_AFTER + 1:], U=U_c, Ep=Ep_c)
    return dict(first=first, rest=rest, U_c=U_c.reshape((2, -1), order='F'), Ep_c=Ep_c, prob=prob, child=child, parent=parent,
                rows=rows)


def refined_errors(r):
    """(U, Ep): `errors` over both parts of the refined history, and the transferred U against the step's closed form."""
    k = REFINE_AFTER
    a = errors('S', r['first'], r['rows'][:k + 1], r['prob']['coord'])
    b = errors('S', r['rest'], r['rows'][k + 1:], r['child']['coord'])
    return max(a[0], b[0]), max(a[1], b[1])


# PLASTIC_EXACT_REFINED_CPU[model, type] = (U, Ep): refined_errors of refined_cpu, rounded up to two digits
PLASTIC_EXACT_REFINED_CPU = {
    ('vm', 'P1'): (4.5e-15, 1.1e-14),
    ('vm', 'P2'): (4.3e-15, 1.4e-14),
    ('vmi', 'P1'): (1.7e-14, 6.7e-15),
    ('vmi', 'P2'): (9.8e-15, 5.1e-14),
}


# ---------------------------------------------------------------------------------------
# the closed forms against the many-digit return maps
# ---------------------------------------------------------------------------------------
def cross_check(case, model, name):
    """The model's many-digit return map (return_map_mp.py, vmi_mp.py, vmps_mp.py) at ONE point, driven step by step with the
    closed form's strains and its own accepted state -> (stress, state) errors and the labels.  The history is the array: the
    stress error is the largest difference of any step over the largest stress of the history (the array-wide measure of
    those modules), the state error the maximum over the steps of the largest component's difference over the step's
    largest component (their per-point measure, the tighter one).  The stress is not measured per step, for a reason that lies
    in this check and in neither side: the map is handed the closed form's strain ROUNDED to float64, eps = t / 2G + pi, and an
    elastic step turns that rounding, up to UNIT |eps|, into 2G UNIT |eps| of stress whatever |t| is.  In the cycles |t| falls
    to 0.1 PEAK while 2G |pi| is 3 to 9 PEAK, so the rounding of the input alone is 30 to 90 UNIT of such a step's own stress."""
    G, K, m3, m4 = materials(case, model)
    rows = exact(case, model, name)
    p = [0.0] * 4
    d_s = e_p = 0.0
    labels = []
    zero = [0.0] * 4
    for row in rows:
        if model == 'vmi':
            import vmi_mp
            r = vmi_mp.point(row['strain'], p, zero, G, K, m3, m4, vmi_mp.Curve(*curve_of(model, name)))
        elif model == 'vmps':
            import vmps_mp
            r = vmps_mp.point(row['strain'], p, zero, G, K, m3, m4)
        else:
            import return_map_mp
            r = return_map_mp.point(model, row['strain'], p, zero, G, K, m3, m4)
        s, p = [float(v) for v in r['s']], [float(v) for v in r['ep']]
        labels.append(int(r['label']))
        d_s = max(d_s, max(abs(u - v) for u, v in zip(s, row['stress'])))
        scale = max(abs(v) for v in row['ep'])
        e_p = max(e_p, max(abs(u - v) for u, v in zip(p, row['ep'])) / (scale or 1.0))
    return d_s / max(abs(v) for row in rows for v in row['stress']), e_p, labels, rows


def cross_check_bound(model, key):
    """The bound of family A (well inside a branch) that the model's many-digit module is held to, MARGIN times the restatement's
    measured error, at least UNIT, at most the standing bound: array-wide for 's', per point for 'ep' (cross_check)."""
    which = 0 if key == 's' else 1
    if model == 'vmi':
        import vmi_cases
        return vmi_cases.bound('A', key)[which]
    if model == 'vmps':
        import vmps_cases
        return vmps_cases.bound('A', key)[which]
    import return_map_mp_cases
    return return_map_mp_cases.bound(model, 'A', key)[which]


# ---------------------------------------------------------------------------------------
# recorded errors of the CPU look-alikes
# ---------------------------------------------------------------------------------------
# PLASTIC_EXACT_CPU[case, model, type] = (U, Ep): `errors` of the look-alike's run (direct solve) over the model's histories on the
# small mesh and, for P1 and Q1, the block mesh, rounded up to two digits; test_plastic_exact_host.py re-measures every figure.
PLASTIC_EXACT_CPU = {
    ('S', 'vm', 'P1'): (4.9e-15, 1.6e-14),
    ('S', 'vm', 'P2'): (2.2e-15, 1.1e-14),
    ('S', 'vm', 'Q1'): (3.8e-15, 1.5e-14),
    ('S', 'vm', 'Q2'): (5.3e-15, 1.8e-14),
    ('S', 'vm', 'P4'): (4.0e-15, 4.3e-14),
    ('S', 'vmi', 'P1'): (2.8e-14, 3.3e-14),
    ('S', 'vmi', 'P2'): (2.1e-14, 3.7e-14),
    ('S', 'vmi', 'Q1'): (1.9e-14, 3.2e-14),
    ('S', 'vmi', 'Q2'): (1.9e-14, 2.6e-14),
    ('S', 'vmi', 'P4'): (2.6e-14, 1.2e-13),
    ('S', 'vmps', 'P1'): (3.2e-15, 2.6e-14),
    ('S', 'vmps', 'P2'): (2.5e-15, 3.3e-14),
    ('S', 'vmps', 'Q1'): (2.4e-15, 3.3e-14),
    ('S', 'vmps', 'Q2'): (1.9e-15, 1.3e-14),
    ('S', 'vmps', 'P4'): (2.7e-15, 6.6e-14),
    ('C', 'dp', 'P1'): (7.1e-16, 2.1e-14),
    ('C', 'dp', 'P2'): (2.9e-14, 1.0e-12),
    ('C', 'dp', 'Q1'): (8.0e-16, 1.5e-14),
    ('C', 'dp', 'Q2'): (7.1e-16, 7.2e-15),
    ('C', 'dp', 'P4'): (4.1e-13, 2.5e-11),
    ('C', 'mc', 'P1'): (1.3e-14, 3.7e-13),
    ('C', 'mc', 'P2'): (8.3e-13, 3.7e-11),
    ('C', 'mc', 'Q1'): (3.5e-14, 7.3e-13),
    ('C', 'mc', 'Q2'): (3.7e-13, 1.4e-11),
    ('C', 'mc', 'P4'): (1.8e-11, 6.0e-10),
}

CASES = [(case, model, t) for case in ('S', 'C') for model in MODELS[case] for t in TYPES]
assert mc_cases.YOUNG == C_YOUNG and abs(mc_cases.PHI - C_PHI) < 1e-15 and mc_cases.COHESION == C_COHESION

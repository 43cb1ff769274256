"""
Closed-form elasticity through the product (exact_cases.py): the cases of tests/test_exact_solutions_host.py with the meshes
from refine_uniform(device=, curves=) and create_midpoints(device=, curves=), K from MeshContext.step(0, want=('K',)) and
the pressure from fep.load_traction(device=).  The free DOFs are solved with SciPy LU on the host: the kernels under test are
the mesh, assembly and load kernels.  Every mesh passes exact_cases.check_mesh, as it does in the host file.

Bounds, each with the worst value measured on the MI355X beside it (MEASURED_GPU and MEASURED_PATCH_GPU below hold every case's):
  U against the oracle's U on the same mesh     30 x the case's sensitivity (exact_cases.MEASURED), at most 1e-9: 4.5e-14 to
                                                1.4e-11 over the cases.  Measured 2.4e-15 to 5.7e-13, at most 0.22 of the bound
  order rule on the GPU's own errors            exact_cases.rule: energy >= k - 0.3, max >= k + 0.2 (default Q2: 0.8, 1.5).
                                                Measured: the oracle's orders to the two digits printed on every case and route;
                                                the thinnest margin is P1 with the pressure, 1.42 against 1.2
  device solve (multigrid, rtol 1e-13)          1e-9 of the LU solution.  Measured 3.2e-13 after 48 iterations
  patch test                                    4 x the ratios of exact_cases.PATCH (the oracle's), strain and interior force.
                                                Measured at most 0.27 (strain) and 0.43 (force) of the bound
"""
from importlib import import_module

import numpy as np
import pytest

import exact_cases as xc
from conftest import relerr
from routes import assert_route
from test_exact_solutions_host import ELASTIC_C, oracle_level

pytestmark = pytest.mark.gpu

DEV = 0

# Measured on the MI355X: case (and route) -> (relerr of U against the oracle, max order, energy order)
MEASURED_GPU = {
    ('P1 ring, Dirichlet', 'default'): (1.8e-14, 1.83, 1.88),# bound 4.8e-13
    ('P1 ring, Dirichlet', 'patch'): (2.4e-14, 1.83, 1.88), # bound 4.8e-13
    ('P1 ring, Dirichlet', 'coo'): (1.9e-14, 1.83, 1.88),   # bound 4.8e-13
    ('P1 ring, pressure', 'default'): (8.3e-14, 1.42, 1.55),# bound 1.1e-12
    ('P1 ring, pressure', 'patch'): (7.1e-14, 1.42, 1.55),  # bound 1.1e-12
    ('P1 ring, pressure', 'coo'): (5.9e-14, 1.42, 1.55),    # bound 1.1e-12
    ('P2 ring, Dirichlet', 'default'): (4.4e-14, 2.53, 2.49),# bound 5.1e-13
    ('P2 ring, pressure', 'default'): (9.3e-14, 2.71, 2.58),# bound 2.1e-12
    ('P4 ring, Dirichlet', 'default'): (2.0e-13, 4.48, 3.95),# bound 2.2e-12
    ('P4 ring, pressure', 'default'): (5.7e-13, 4.65, 3.99),# bound 1.4e-11
    ('P1 ring5, pressure', 'default'): (9.2e-14, 1.50, 1.58),# bound 1.7e-12
    ('P1 ring5, pressure', 'patch'): (9.3e-14, 1.50, 1.58), # bound 1.7e-12
    ('P1 ring5, pressure', 'coo'): (8.8e-14, 1.50, 1.58),   # bound 1.7e-12
    ('P2 ring5, pressure', 'default'): (1.0e-13, 2.88, 2.58),# bound 1.4e-12
    ('P4 ring5, Dirichlet', 'default'): (1.6e-13, 4.48, 3.95),# bound 1.5e-12
    ('P4 ring5, pressure', 'default'): (4.8e-13, 4.61, 3.99),# bound 9.0e-12
    ('P1 square', 'default'): (3.0e-15, 1.69, 1.87),        # bound 4.5e-14
    ('P1 square', 'patch'): (2.4e-15, 1.69, 1.87),          # bound 4.5e-14
    ('P1 square', 'coo'): (3.0e-15, 1.69, 1.87),            # bound 4.5e-14
    ('P2 square', 'default'): (1.1e-14, 2.87, 2.48),        # bound 1.1e-13
    ('P4 square', 'default'): (6.2e-14, 4.65, 3.98),        # bound 4.5e-13
    ('Q1 rect', 'default'): (2.7e-14, 2.01, 1.99),          # bound 1.8e-13
    ('Q2 rect', 'default'): (5.8e-14, 1.80, 0.96),          # bound 2.6e-13
    ('Q2 rect, Gauss', 'default'): (1.2e-13, 3.80, 2.95),   # bound 9.0e-13
}
# patch case, route -> (strain ratio, interior-force ratio)
MEASURED_PATCH_GPU = {
    ('P1 ring', 'default'): (3.55, 8.14),                   # bounds 14.20, 24.52
    ('P1 ring', 'patch'): (3.55, 5.82),                     # bounds 14.20, 24.52
    ('P1 ring', 'coo'): (3.55, 5.82),                       # bounds 14.20, 24.52
    ('P1 ring5', 'default'): (3.55, 8.14),                  # bounds 14.20, 18.80
    ('P1 ring5', 'patch'): (3.55, 5.82),                    # bounds 14.20, 18.80
    ('P1 ring5', 'coo'): (3.55, 5.82),                      # bounds 14.20, 18.80
    ('P1 square', 'default'): (1.47, 29.69),                # bounds 5.72, 99.84
    ('P1 square', 'patch'): (1.47, 29.69),                  # bounds 5.72, 99.84
    ('P1 square', 'coo'): (1.47, 29.69),                    # bounds 5.72, 99.84
    ('P2 ring', 'default'): (8.76, 1077.36),                # bounds 36.08, 4336.56
    ('P2 ring', 'coo'): (8.76, 1077.36),                    # bounds 36.08, 4336.56
    ('P2 ring5', 'default'): (8.76, 1077.36),               # bounds 36.08, 4336.56
    ('P2 ring5', 'coo'): (8.76, 1077.36),                   # bounds 36.08, 4336.56
    ('P2 square', 'default'): (7.18, 895.57),               # bounds 28.72, 3627.80
    ('P2 square', 'coo'): (7.18, 895.57),                   # bounds 28.72, 3627.80
    ('P4 ring', 'default'): (7.84, 16497.95),               # bounds 32.16, 66063.16
    ('P4 ring', 'coo'): (7.84, 16497.95),                   # bounds 32.16, 66063.16
    ('P4 ring5', 'default'): (7.84, 16497.95),              # bounds 32.16, 66063.16
    ('P4 ring5', 'coo'): (7.84, 16497.95),                  # bounds 32.16, 66063.16
    ('P4 square', 'default'): (3.93, 15660.92),             # bounds 14.68, 62851.40
    ('P4 square', 'coo'): (3.93, 15660.92),                 # bounds 14.68, 62851.40
    ('Q1 rect', 'default'): (1.83, 7.22),                   # bounds 9.56, 23.84
    ('Q1 rect', 'coo'): (1.83, 7.22),                       # bounds 9.56, 23.84
    ('Q2 rect', 'default'): (6.21, 14.40),                  # bounds 27.60, 68.68
    ('Q2 rect', 'coo'): (6.21, 14.40),                      # bounds 27.60, 68.68
    ('P1 curved', 'default'): (18.23, 38.01),               # bounds 67.72, 151.00
    ('P1 curved', 'patch'): (16.93, 34.57),                 # bounds 67.72, 151.00
    ('P1 curved', 'coo'): (16.93, 34.57),                   # bounds 67.72, 151.00
    ('P1 delaunay', 'default'): (14.62, 47.05),             # bounds 58.48, 202.16
    ('P1 delaunay', 'patch'): (14.62, 47.05),               # bounds 58.48, 202.16
    ('P1 delaunay', 'coo'): (14.62, 47.05),                 # bounds 58.48, 202.16
    ('P1 renumbered', 'default'): (15.63, 57.59),           # bounds 57.28, 242.32
    ('P1 renumbered', 'patch'): (14.32, 54.10),             # bounds 57.28, 242.32
    ('P1 renumbered', 'coo'): (14.32, 54.60),               # bounds 57.28, 242.32
    ('P1 mixed', 'default'): (14.32, 57.46),                # bounds 57.28, 253.20
    ('P1 mixed', 'patch'): (14.32, 59.30),                  # bounds 57.28, 253.20
    ('P1 mixed', 'coo'): (14.32, 59.30),                    # bounds 57.28, 253.20
    ('P2 curved', 'default'): (22.41, 1352.67),             # bounds 89.64, 5456.84
    ('P2 curved', 'coo'): (22.41, 1352.67),                 # bounds 89.64, 5456.84
    ('P2 delaunay', 'default'): (33.87, 1160.14),           # bounds 135.48, 4637.76
    ('P2 delaunay', 'coo'): (33.87, 1160.14),               # bounds 135.48, 4637.76
    ('P2 renumbered', 'default'): (34.19, 1259.65),         # bounds 136.76, 5057.48
    ('P2 renumbered', 'coo'): (34.19, 1259.65),             # bounds 136.76, 5057.48
    ('P2 mixed', 'default'): (34.19, 1259.65),              # bounds 136.76, 5021.16
    ('P2 mixed', 'coo'): (34.19, 1259.65),                  # bounds 136.76, 5021.16
    ('P4 curved', 'default'): (32.96, 21237.10),            # bounds 133.44, 84947.36
    ('P4 curved', 'coo'): (32.96, 21237.10),                # bounds 133.44, 84947.36
    ('P4 delaunay', 'default'): (34.64, 16511.47),          # bounds 135.64, 66024.32
    ('P4 delaunay', 'coo'): (34.64, 16511.47),              # bounds 135.64, 66024.32
    ('P4 renumbered', 'default'): (17.70, 19293.58),        # bounds 70.80, 77163.44
    ('P4 renumbered', 'coo'): (17.70, 19293.58),            # bounds 70.80, 77163.44
    ('P4 mixed', 'default'): (16.22, 19133.43),             # bounds 64.12, 76449.32
    ('P4 mixed', 'coo'): (16.22, 19133.43),                 # bounds 64.12, 76449.32
    ('Q1 curved', 'default'): (20.83, 34.82),               # bounds 88.56, 135.28
    ('Q1 curved', 'coo'): (20.83, 34.56),                   # bounds 88.56, 135.28
    ('Q1 renumbered', 'default'): (23.39, 37.48),           # bounds 93.56, 164.76
    ('Q1 renumbered', 'coo'): (23.39, 37.48),               # bounds 93.56, 164.76
    ('Q1 mixed', 'default'): (20.83, 34.90),                # bounds 78.12, 136.96
    ('Q1 mixed', 'coo'): (20.83, 34.69),                    # bounds 78.12, 136.96
    ('Q2 curved', 'default'): (17.27, 43.23),               # bounds 69.08, 203.80
    ('Q2 curved', 'coo'): (17.27, 43.23),                   # bounds 69.08, 203.80
    ('Q2 renumbered', 'default'): (17.99, 45.13),           # bounds 71.96, 193.84
    ('Q2 renumbered', 'coo'): (17.99, 45.13),               # bounds 71.96, 193.84
    ('Q2 mixed', 'default'): (17.99, 39.26),                # bounds 69.48, 158.76
    ('Q2 mixed', 'coo'): (17.99, 39.26),                    # bounds 69.48, 158.76
}

ROUTES = {'P1': ('default', 'patch', 'coo')}
CONVERGENCE = [(n, r) for n, c in xc.CASES.items() for r in ROUTES.get(c['et'], ('default',))]
PATCH_RUNS = [(n, r) for n in xc.patch_names() for r in ROUTES.get(n.split()[0], ('default', 'coo'))]

_ORACLE = {}


def _oracle_U(fep, name, level, m):
    """The oracle's U on the mesh the device made, once per case (the routes share it, unchanged)."""
    if name not in _ORACLE:
        U = oracle_level(fep, name, level, m)[2]
        U.setflags(write=False)
        _ORACLE[name] = U
    return _ORACLE[name]


def _context(fep, monkeypatch, elem, coord, tabs, route):
    if route == 'default':
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    ctx = fep.MeshContext(elem, coord, *tabs)
    t = ctx.element_type.name
    assert_route(ctx, route if route != 'default' else ('node' if t == 'P1' else 'patch'))
    ctx.set_materials(xc.SHEAR, xc.BULK, 0.1, ELASTIC_C)
    return ctx


def _gpu_level(fep, monkeypatch, name, level, route):
    """(mesh, K, U, f) of one level through the product."""
    c = xc.CASES[name]
    m = xc.mesh(fep, c['kind'], c['et'], level, device=DEV)
    xc.check_mesh(c, level, m)
    ctx = _context(fep, monkeypatch, m['elem'], m['coord'], xc.tables(fep, c), route)
    try:
        r = ctx.step(np.zeros(ctx.n_dof), want=('K',))
        assert r['n_smooth'] == 0 and r['n_apex'] == 0
        K = r['K'].copy()
    finally:
        ctx.close()
    f = None
    if c['load'] == 'pressure':
        edges, t, (hat, dhat, wf) = xc.wall_traction(m, c['et'])
        f = fep.load_traction(edges, m['coord'], t, hat, dhat, wf, device=DEV)
    return m, K, xc.solve(K, m, c['load'], f), f


@pytest.mark.parametrize('name,route', CONVERGENCE)
def test_convergence(fep, monkeypatch, name, route):
    """The two finest levels of the case: the order rule on the GPU's own errors, and U of the finest level against the
    oracle's on the same mesh."""
    c = xc.CASES[name]
    errs = []
    for level in c['levels'][-2:]:
        m, K, U, _ = _gpu_level(fep, monkeypatch, name, level, route)
        errs.append(xc.errors(K, m, U))
    o_max, o_en = xc.orders(errs)[0]
    d = relerr(U, _oracle_U(fep, name, c['levels'][-1], m))
    print(f"('{name}', '{route}'): ({d:.1e}, {o_max:.2f}, {o_en:.2f}),   # bound {xc.bound(name):.1e}")
    least_max, least_en = xc.rule(name)
    assert o_max >= least_max and o_en >= least_en, (name, route, o_max, o_en)
    assert d <= xc.bound(name), (name, route, d)


def test_device_solver_reaches_the_lu_solution(fep, monkeypatch):
    """P2 ring with the pressure, level 3, solved on the device with the multigrid-preconditioned CG at rtol 1e-13."""
    newton = import_module('fem-elastoplasticity_amd.newton')
    name, level = 'P2 ring, pressure', 3
    c = xc.CASES[name]
    m, K, U, f = _gpu_level(fep, monkeypatch, name, level, 'default')
    free, rhs, lift = xc.lifted_rhs(K, m, c['load'], f)
    ctx = _context(fep, monkeypatch, m['elem'], m['coord'], xc.tables(fep, c), 'default')
    ops = newton.make_ops(ctx, free, 'amg', 1e-13)
    try:
        Kd = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']
        assert np.array_equal(ops.host(Kd), K.data)
        ops.setup_amg(Kd, m['coord'])
        x = ops.host(ops.solve(Kd, ops.vec(rhs)))
    finally:
        ops.close()
        ctx.close()
    assert np.isfinite(x).all() and ops.solver.last['state'] == 1
    d = relerr(x + lift, U)
    print(f'device solve against LU: {d:.1e} after {ops.pcg_iters[-1]} iterations')
    assert d <= 1e-9
    assert xc.errors(K, m, x + lift)[0] <= 2 * 1.4e-3                          # and the Lame solution to the level's error (8e-4 .. 1.4e-3)


@pytest.mark.parametrize('name,route', PATCH_RUNS)
def test_patch(fep, monkeypatch, name, route):
    """step(U_lin, want=('E', 'F')): the strain at every point against the constant, the force at every interior DOF against
    zero, as ratios to ElemRef's u S_E and u S_F."""
    elem, coord, inner = xc.patch_mesh(fep, name, device=DEV)
    assert inner.any() and not inner.all()
    tabs = xc.patch_tables(fep, name)
    ctx = _context(fep, monkeypatch, elem, coord, tabs, route)
    try:
        r = ctx.step(xc.linear(coord), want=('E', 'F'))
        assert r['n_smooth'] == 0 and r['n_apex'] == 0
        E, F = r['E'].copy(), r['F'].copy()
    finally:
        ctx.close()
    r_e, r_f = xc.patch_ratios(elem, coord, tabs, inner, E, F)
    print(f"('{name}', '{route}'): ({r_e:.2f}, {r_f:.2f}),   # bounds {4 * xc.PATCH[name][0]:.2f}, {4 * xc.PATCH[name][1]:.2f}")
    assert r_e <= 4 * xc.PATCH[name][0] and r_f <= 4 * xc.PATCH[name][1], (name, route, r_e, r_f)
    assert np.abs(F[xc.dof_mask(~inner)]).max() > 1e-3 * max(np.abs(xc.linear_stress())) * np.ptp(coord[0]) / elem.shape[1]

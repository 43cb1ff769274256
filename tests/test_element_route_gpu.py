"""
The element route (element_kernel in its patch form + fixup_kernel, and its COO form) against the element-by-element
float64 reference (tests/elem_ref.py), entry by entry, for every element type.

Three decoupled stages, so that a last-bit difference in the strain can never flip a branch:
  1. E of the kernel against the reference strain, per point:             |dE|  <= C_E u S_E
  2. s, ds, ind_p (and the accepted ep) of the kernel against the oracle's return map applied to the KERNEL's E
  3. K and F of the kernel against the reference assembly of the KERNEL's ds and s, per entry:
                                                                              |dK_ij| <= C_K u S_ij,  |dF_i| <= C_F u S_F,i
(u = 2^-53; S_* = elem_ref's error scales).  Every case also pins the K,F-only, K-only and F-only steps and assemble(ds, s)
bitwise to the full-output step.

Bounds: measured worst ratios (MI355X, every case of this module, both forms) are written beside each bound; the bounds are
at most 10x those.
"""
import re

import zlib

import numpy as np
import pytest

import meshes
from conftest import dp_materials, load_golden, relerr_points
from elem_ref import ElemRef, ratio, reverse_elements
from footprint import scrub
from meshes import named as _mesh
from oracle import fep_oracle as orc
from routes import assert_route

pytestmark = pytest.mark.gpu

# bounds on |delta| / (u S), per type; measured worst over every case of the module, both forms, in the comments
C_E = {'P1': 6, 'P2': 8, 'Q1': 8, 'Q2': 8, 'P4': 8}           # measured 2.75, 3.83, 3.79, 3.73, 3.37
C_K = {'P1': 10, 'P2': 16, 'Q1': 12, 'Q2': 16, 'P4': 24}      # measured 4.55, 7.63, 5.87, 7.29, 11.23
C_F = {'P1': 8, 'P2': 12, 'Q1': 10, 'Q2': 10, 'P4': 12}       # measured 3.52, 5.70, 4.77, 4.71, 5.79
# the P1 node route under the same P1 bounds (test_p1_node_route_gpu.py, against the record form): measured E 3.13, K 4.73, F 5.13;
# against the exact form on the widened scale, bounds C_K + C_RECORD, C_F + C_RECORD: measured K 4.65, F 4.66
C_RECORD = 4                   # the P1 record form against the exact form on the widened scale (test_elem_ref.py)
TOL_PT_EACH = 1e-12            # stage 2, per point against its own largest entry (test_parity_gpu.py)
TOL_PT_WIDE = 5e-12            # ... with materials spanning decades (test_return_map_random_materials_wide_ranges)

# patch plan shape per type (fep_api.hip setup_patch, fep_kernels.hip.h ElemCfg): elements per workgroup, run length
EB = {'P1': 64, 'P2': 56, 'Q1': 64, 'Q2': 24, 'P4': 16}
RUN = {'P1': 32, 'P2': 14, 'Q1': 16, 'Q2': 12, 'P4': 8}
PLAN = re.compile(r'\[fep\] patch plan: (\d+) patches of <= (\d+) elements, \d+ items \(<= \d+ per patch\), (\d+) open blocks '
                  r'of \d+, (\d+) partials \(([\d.]+) per element\), (\d+) open nodes')
ROUTES = {'P1': ('patch', 'coo'), 'P2': ('default', 'coo'), 'Q1': ('default', 'coo'), 'Q2': ('default', 'coo'),
          'P4': ('default', 'coo')}


def _structured_cases(t):
    """(nx, ny, dropped trailing elements): strip length (elements per cell row) and n_e at 0, +1 and -1 modulo the run
    length and the elements per workgroup.  The triangles' strips hold 2 nx elements, so their strip residues are 0, +2,
    -2; the odd element counts come from dropping the last element."""
    run, eb = RUN[t], EB[t]
    if t in ('Q1', 'Q2'):
        return [(eb, 10, 0), (eb + 1, eb + 1, 0), (eb - 1, eb + 1, 0)]
    h = eb // 2
    return [(h, 10, 0), (h + 1, h + 1, 0), (h - 1, h + 1, 0), (h + 1, h + 1, 1), (h, 10, 1)]


def _cases():
    out = []
    for t in ('P1', 'P2', 'Q1', 'Q2', 'P4'):
        for r in ROUTES[t]:
            for nx, ny, k in _structured_cases(t):
                out.append((t, r, f'structured_{nx}x{ny}-{k}'))
            for name in ('strip1', 'strip2', 'renumbered', 'mixed', 'curved', 'aniso', 'delaunay'):
                if name == 'delaunay' and t in ('Q1', 'Q2'):
                    continue
                out.append((t, r, name))
    return out


def _state(kind, coord, h, n_int, rng):
    """Displacement, previous plastic strain, materials, e0 and accept for `kind`: all three branches populated."""
    x, y = coord
    xn, yn = 10 * (x - x.min()) / np.ptp(x), 10 * (y - y.min()) / np.ptp(y)      # switches on [0, 10]^2, strains ~1e-4
    U = np.array([2.0e-4 * y * (xn / 10) + 1.0e-4 * x * (yn > 5), -1.2e-4 * y * (xn < 5) + 1.6e-4 * y * (xn >= 5)])
    U += rng.normal(0, 1e-4 * h, size=U.shape)                     # i.i.d. strain noise of ~1e-4 per element
    Ep = rng.normal(0, 5e-6, size=(4, n_int))
    mats = dp_materials(n_int)
    e0 = None
    if kind == 'wide':                                              # per point, spanning decades
        sh = 10 ** rng.uniform(4, 8, n_int)
        mats = (sh, sh * 10 ** rng.uniform(-0.5, 1, n_int), rng.uniform(0.05, 0.9, n_int), sh * 10 ** rng.uniform(-5.5, -3, n_int))
    elif kind == 'tsx':
        e0 = load_golden('tsx')['init_strain'].ravel() * 0.1
    return U, Ep, mats, e0, kind == 'accept'


def _run_case(fep, monkeypatch, capfd, t, route, elem, coord, kind, h, rng, structured_ppe=None, keep=None):
    """One case on `route`: patch | coo (FEP_ROUTE), default (FEP_ROUTE unset, must come out as the patch form) or node (P1,
    FEP_ROUTE unset, must come out as the node route: test_p1_node_route_gpu.py).  Returns the plan line's figures (node:
    p1_node_cases.parse_lib's), None on the COO form; `keep` (a dict) receives the full-output step."""
    n_e = elem.shape[1]
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    monkeypatch.setenv('FEP_VERBOSE', '1')
    if n_e < 100_000:
        monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    else:
        monkeypatch.delenv('FEP_VALIDATE_PLAN', raising=False)
    capfd.readouterr()
    ctx = fep.MeshContext(elem, coord)
    err = capfd.readouterr().err
    plan = PLAN.findall(err)
    assert_route(ctx, 'patch' if route == 'default' else route)
    assert len(plan) == (0 if route in ('coo', 'node') else 1), plan
    n_int = ctx.n_int
    U, Ep, mats, e0, accept = _state(kind, coord, h, n_int, rng)
    ctx.set_materials(*mats)
    kw = {} if e0 is None else {'e0': e0}
    ep = Ep.copy()                                                  # pageable, updated in place on accept
    # scrub between the forms: none may pass its pin with what the call before left in the context's device buffers
    if accept:
        scrub(ctx, U, Ep, kw)
    full = ctx.step(U, ep, apply_plastic_strain=accept, want=('E', 's', 'ds', 'ind_p', 'K', 'F'), **kw)
    scrub(ctx, U, Ep, kw)
    kf = ctx.step(U, Ep.copy(), want=('K', 'F'), **kw)
    scrub(ctx, U, Ep, kw)
    k_only = ctx.step(U, Ep.copy(), want=('K',), **kw)
    scrub(ctx, U, Ep, kw)
    f_only = ctx.step(U, Ep.copy(), want=('F',), **kw)
    scrub(ctx, U, Ep, kw)
    K2, F2 = ctx.assemble(full['ds'], full['s'])
    pattern = ctx.pattern()
    ctx.close()
    assert np.array_equal(kf['K'].data, full['K'].data) and np.array_equal(kf['F'], full['F'])
    assert np.array_equal(k_only['K'].data, full['K'].data) and np.array_equal(f_only['F'], full['F'])
    assert np.array_equal(K2.data, full['K'].data) and np.array_equal(F2, full['F'])
    ref = ElemRef(elem, coord, fep.element_tables(t), pattern=pattern)
    # 1. strain
    E, S_E = ref.strain(U)
    r_E = ratio(full['E'], E, S_E)
    assert r_E <= C_E[t], ('E', r_E)
    # 2. return map on the kernel's strain
    wide = kind == 'wide'
    o = orc.return_map(full['E'], Ep.copy(), *mats, accept, e0=None if e0 is None else e0.reshape(4, 1), tsx=e0 is not None)
    assert np.array_equal(full['ind_p'], o['ind_p'])
    assert (full['n_smooth'], full['n_apex']) == (o['n_smooth'], o['n_apex'])
    assert full['n_smooth'] + full['n_apex'] == int(full['ind_p'].sum())
    tol = TOL_PT_WIDE if wide else TOL_PT_EACH
    assert relerr_points(full['s'], o['s']) <= tol and relerr_points(full['ds'], o['ds']) <= tol
    if accept:
        assert relerr_points(ep, o['ep']) <= tol
    else:
        assert np.array_equal(ep, Ep)
    if n_int >= 200:                                                # all three branches
        assert o['n_smooth'] > 0 and o['n_apex'] > 0 and o['n_smooth'] + o['n_apex'] < n_int, (o['n_smooth'], o['n_apex'])
    # 3. assembly of the kernel's ds and s
    if keep is not None:
        keep['full'] = full
    if route == 'node':
        # the node route sums the terms of the 48-byte record (elem_ref's module docstring): against the record form on
        # its plain scale with the element route's bounds, against the exact form on the widened scale with C + C_RECORD
        import p1_node_cases
        rec = ElemRef(elem, coord, fep.element_tables(t), pattern=pattern, record=True)
        K, S_K, F, S_F = rec.assemble(full['ds'], full['s'])
        r_K, r_F = ratio(full['K'].data, K, S_K), ratio(full['F'], F, S_F)
        Kx, W_K, Fx, W_F = ref.assemble(full['ds'], full['s'], widened=True)
        x_K, x_F = ratio(full['K'].data, Kx, W_K), ratio(full['F'], Fx, W_F)
        print(f'[ratios] {t} node n_e={n_e} E {r_E:.2f} K {r_K:.2f} F {r_F:.2f}; exact form, widened scale: K {x_K:.2f} F {x_F:.2f}')
        assert r_K <= C_K[t], ('K', r_K)
        assert r_F <= C_F[t], ('F', r_F)
        assert x_K <= C_K[t] + C_RECORD, ('K, exact form', x_K)
        assert x_F <= C_F[t] + C_RECORD, ('F, exact form', x_F)
        return p1_node_cases.parse_lib(err)
    K, S_K, F, S_F = ref.assemble(full['ds'], full['s'])
    r_K = ratio(full['K'].data, K, S_K)
    r_F = ratio(full['F'], F, S_F)
    assert r_K <= C_K[t], ('K', r_K)
    assert r_F <= C_F[t], ('F', r_F)
    print(f'[ratios] {t} {route} n_e={n_e} E {r_E:.2f} K {r_K:.2f} F {r_F:.2f}')
    if plan:
        n_patch, eb, n_open, n_part, ppe, n_fopen = plan[0]
        return dict(n_patch=int(n_patch), eb=int(eb), n_open=int(n_open), ppe=float(ppe), n_fopen=int(n_fopen))
    return None


@pytest.mark.parametrize('t,route,name', _cases())
def test_element_route_vs_reference_per_entry(fep, monkeypatch, capfd, t, route, name):
    rng = np.random.default_rng(zlib.crc32(f'{t} {name}'.encode()))      # the same case on both forms
    elem, coord, h, kind = _mesh(t, name, rng)
    plan = _run_case(fep, monkeypatch, capfd, t, route, elem, coord, kind, h, rng)
    if plan is None:
        return
    # each case reaches what it exists for
    assert plan['eb'] == EB[t]
    n_e = elem.shape[1]
    if name.startswith('structured'):
        assert plan['n_patch'] >= n_e / EB[t]
    if name in ('renumbered', 'delaunay', 'mixed', 'curved', 'strip2') or name.startswith('structured'):
        assert plan['n_open'] > 0
    if name in ('renumbered', 'delaunay'):
        # randomly numbered: patches without locality, more partials per element than the structured mesh of the type
        st = meshes.square(t, {'P1': 24, 'P2': 14, 'Q1': 24, 'Q2': 12, 'P4': 8}[t])
        capfd.readouterr()
        c2 = fep.MeshContext(*st)
        ppe_st = float(PLAN.findall(capfd.readouterr().err)[0][4])
        c2.close()
        assert plan['ppe'] > ppe_st, (plan['ppe'], ppe_st)
    if name == 'mixed':
        assert (ElemRef(elem, coord, fep.element_tables(t)).det() < 0).mean() > 0.3


# whole meshes at the benchmark's scale, default route, branches i.i.d. per point
@pytest.mark.parametrize('t,nx,ny', [('Q1', 1000, 1000), ('Q2', 500, 500), ('P4', 274, 274), ('P2', 708, 708)])
def test_element_route_whole_large_mesh(fep, monkeypatch, capfd, t, nx, ny):
    rng = np.random.default_rng(nx)
    elem, coord = meshes.rect(t, nx, ny)
    assert elem.shape[1] >= 150_000
    plan = _run_case(fep, monkeypatch, capfd, t, 'default', elem, coord, 'plain', 10 / nx, rng)
    assert plan['n_open'] > 0 and plan['n_patch'] >= elem.shape[1] / EB[t]


@pytest.mark.parametrize('t', ['P1', 'P2', 'Q1', 'Q2', 'P4'])
@pytest.mark.parametrize('route', ['patch', 'coo'])
def test_assemble_reads_the_upper_triangle_of_ds(fep, monkeypatch, t, route):
    """include/fep.h: ds must be symmetric, only rows 0, 1, 2, 4, 5, 8 are read.  Garbage in rows 3, 6, 7 gives K bit for bit
    equal to the symmetric ds's."""
    if route == 'patch' and t != 'P1':
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    rng = np.random.default_rng(6)
    elem, coord = meshes.square(t, {'P1': 9, 'P2': 6, 'Q1': 9, 'Q2': 5, 'P4': 4}[t])
    ctx = fep.MeshContext(elem, coord)
    assert_route(ctx, route)
    n = ctx.n_int
    A = rng.normal(size=(3, 3, n))
    ds = (A + A.transpose(1, 0, 2)).reshape(9, n)
    bad = ds.copy()
    bad[[3, 6, 7]] = rng.normal(size=(3, n)) * 1e3
    K1, _ = ctx.assemble(ds)
    K2, _ = ctx.assemble(bad)
    ctx.close()
    assert np.array_equal(K1.data, K2.data)
    ref = ElemRef(elem, coord, fep.element_tables(t), pattern=(K1.indptr, K1.indices))
    K, S_K, _, _ = ref.assemble(ds)
    assert ratio(K1.data, K, S_K) <= C_K[t]

"""
Parity of the HIP path (through the C ABI, libfep_hip.so) with
  (i)  golden vectors recorded from the reference itself (tests/golden/*.npz), and
  (ii) the oracle (oracle/fep_oracle.py) on seeded inputs,
plus size-independent properties at the benchmark's full size.

Tolerances (fp64): stresses / tangents / plastic strain 1e-13 relative to the array's max
(the reference's own 4x4 BLAS product `dev @ E_tr` has an unspecified summation order, so
bit-equality is not defined); geometry (dphi, weight) and all index arrays bit-exact;
K, F 1e-12 (different but fixed summation order over elements).
"""
import numpy as np
import pytest
import scipy.sparse as ssp

from conftest import dp_materials, load_golden, relerr, relerr_points, relerr_rows
from fan_mesh import fan_mesh
from footprint import scrub
from meshes import rect as rect_mesh_of, square as square_mesh_of
from oracle import fep_oracle as orc
from routes import assert_route

pytestmark = pytest.mark.gpu

ELS = ('P1', 'P2', 'Q1', 'Q2')
NQ = {'P1': 1, 'P2': 7, 'Q1': 4, 'Q2': 9, 'P4': 12}
TOL_PT = 1e-13
TOL_K = 1e-12
# per integration point / per matrix row (conftest.relerr_points, relerr_rows): every point against ITS OWN largest
# entry, every row of K against its own largest entry; the stress of a smooth point is a difference of two terms of
# the trial stress's size (DP:720), hence the extra decade
TOL_PT_EACH = 1e-12
TOL_K_EACH = 1e-11


def tables(mod, t):
    g = load_golden('tables')
    k = f'{mod}_{t}_'
    return g[k + 'dhatp1'], g[k + 'dhatp2'], g[k + 'wf']


# ---- a2 -------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['dp_none', 'dp_ep', 'dp_ep_accept', 'tsx_ep', 'tsx_ep_accept'])
@pytest.mark.parametrize('order', ['C', 'F'])
def test_return_map_vs_reference_golden(fep, case, order):
    g = load_golden('retmap')
    tsx = case.startswith('tsx')
    accept = case.endswith('accept')
    ep_in = None if case == 'dp_none' else g['Ep'].copy()
    E = np.array(g['E'], order=order)                     # the driver passes an F-ordered array (DP:1043)
    E_before = E.copy()
    if tsx:
        r = fep.tsx_tunnel.construct_constitutive_problem(E, g['e0'], ep_in, g['shear'], g['bulk'], g['eta'], g['c'], accept)
    else:
        r = fep.plasticity2d_dp.construct_constitutive_problem(E, ep_in, g['shear'], g['bulk'], g['eta'], g['c'], accept)
    assert np.array_equal(E, E_before)
    assert r['s'].shape == (4, E.shape[1]) and r['ds'].shape == (9, E.shape[1]) and r['ind_p'].dtype == np.bool_
    assert np.array_equal(r['ind_p'], g[case + '_ind_p'])
    assert relerr(r['s'], g[case + '_s']) <= TOL_PT
    assert relerr(r['ds'], g[case + '_ds']) <= TOL_PT
    assert relerr_points(r['s'], g[case + '_s']) <= TOL_PT_EACH and relerr_points(r['ds'], g[case + '_ds']) <= TOL_PT_EACH
    if accept:
        assert relerr(r['ep'], g[case + '_ep']) <= TOL_PT
        assert r['ep'] is ep_in                                        # C4 aliasing
        assert relerr(ep_in, g[case + '_ep_prev_after']) <= TOL_PT
    else:
        assert not r['ep'].any() and r['ep'].shape == (4, E.shape[1])
        if ep_in is not None:
            assert np.array_equal(ep_in, g['Ep'])                      # untouched without accept
    assert (r['lambda_final'] is None) == bool(g[case + '_lambda_is_none'])
    # the counts the reference logs (DP:730)
    ref = orc.return_map(g['E'], None if ep_in is None else g['Ep'].copy(), g['shear'], g['bulk'], g['eta'], g['c'],
                         False, e0=g['e0'] if tsx else None, tsx=tsx)
    assert (r['n_smooth'], r['n_apex']) == (ref['n_smooth'], ref['n_apex'])


def test_return_map_all_elastic_quirks(fep):
    g = load_golden('retmap')
    sh, bu, eta, c = dp_materials(64)
    r = fep.construct_constitutive_problem(g['Eel'], np.zeros((4, 64)), sh, bu, eta, c, True)
    assert relerr(r['s'], g['dp_elastic_s']) <= TOL_PT and relerr(r['ds'], g['dp_elastic_ds']) <= TOL_PT
    assert r['lambda_final'] is None and not r['ep'].any()
    ep_in = g['tsx_elastic_ep_in'].copy()
    r = fep.construct_constitutive_problem_tsx(g['Eel'], np.zeros((4, 1)), ep_in, sh, bu, eta, c, True)
    assert relerr(r['s'], g['tsx_elastic_s']) <= TOL_PT
    assert np.array_equal(r['ep'], g['tsx_elastic_ep']) and r['ep'] is not ep_in     # TSX:1103 early-out
    assert np.array_equal(r['lambda_final'], g['tsx_elastic_lambda'])
    assert np.array_equal(ep_in, g['tsx_elastic_ep_in'])


def test_return_map_edge_sizes(fep):
    sh, bu, eta, c = dp_materials(0)
    r = fep.construct_constitutive_problem(np.zeros((3, 0)), None, sh, bu, eta, c)
    assert r['s'].shape == (4, 0) and r['ds'].shape == (9, 0) and r['n_smooth'] == 0
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 257, 1000):          # ragged tails of the 256-lane blocks
        sh, bu, eta, c = dp_materials(n)
        E = rng.normal(0, 3e-4, size=(3, n))
        ep = rng.normal(0, 1e-5, size=(4, n))
        a = fep.construct_constitutive_problem(E, ep.copy(), sh, bu, eta, c, True)
        b = orc.return_map(E, ep.copy(), sh, bu, eta, c, True)
        assert np.array_equal(a['ind_p'], b['ind_p'])
        assert relerr(a['s'], b['s']) <= TOL_PT and relerr(a['ds'], b['ds']) <= TOL_PT and relerr(a['ep'], b['ep']) <= TOL_PT


def test_return_map_large_random_vs_oracle(fep):
    rng = np.random.default_rng(99)
    n = 200_000
    sh, bu, eta, c = dp_materials(n)
    sh *= rng.uniform(0.5, 2, n); bu *= rng.uniform(0.5, 2, n); eta *= rng.uniform(0.5, 1.5, n); c *= rng.uniform(0.5, 2, n)
    E = rng.normal(0, 2e-4, size=(3, n))
    E[:, : n // 50] += 4e-4                        # a band of apex points (oracle is fine up to ~20k)
    ep = rng.normal(0, 2e-5, size=(4, n))
    a = fep.construct_constitutive_problem(E, ep.copy(), sh, bu, eta, c, True)
    b = orc.return_map(E, ep.copy(), sh, bu, eta, c, True)
    assert b['n_apex'] > 1000 and b['n_smooth'] > 10000
    assert (a['n_smooth'], a['n_apex']) == (b['n_smooth'], b['n_apex'])
    assert np.array_equal(a['ind_p'], b['ind_p'])
    assert relerr(a['s'], b['s']) <= TOL_PT and relerr(a['ds'], b['ds']) <= TOL_PT and relerr(a['ep'], b['ep']) <= TOL_PT
    # properties: yield consistency after a smooth return, apex stress, symmetric tangent
    s, ds = a['s'], a['ds']
    i_s = np.logical_and(a['ind_p'], np.abs(ds).sum(axis=0) > 0)
    i_a = np.logical_and(a['ind_p'], ~i_s)
    p = (s[0] + s[1] + s[3]) / 3
    dev = s - p * np.array([[1], [1], [0], [1]])
    rho = np.sqrt(dev[0] ** 2 + dev[1] ** 2 + 2 * dev[2] ** 2 + dev[3] ** 2)
    f = rho / np.sqrt(2) + eta * p - c
    assert np.abs(f[i_s]).max() <= 1e-9 * c.max()
    assert np.allclose(s[0][i_a], (c / eta)[i_a], rtol=1e-15) and not s[2][i_a].any()
    assert np.array_equal(ds[1], ds[3]) and np.array_equal(ds[2], ds[6]) and np.array_equal(ds[5], ds[7])


# ---- a6 -------------------------------------------------------------------------------
@pytest.mark.parametrize('t', ELS)
def test_elastic_setup_vs_reference_golden(fep, t):
    g = load_golden('setup_dp')
    d1, d2, wf = tables('dp', t)
    elem = g[f'{t}_elements'].copy()
    K, B, w, iD, jD, D = fep.get_elastic_stiffness_matrix(elem, g[f'{t}_coordinates'], g[f'{t}_shear'], g[f'{t}_bulk'],
                                                          d1, d2, wf)
    assert np.array_equal(elem, g[f'{t}_elements'])                   # inputs untouched (DP flavour)
    assert w.shape == g[f'{t}_weight'].shape and np.array_equal(w, g[f'{t}_weight'])      # bit-exact geometry
    assert np.array_equal(iD, g[f'{t}_iD']) and np.array_equal(jD, g[f'{t}_jD'])
    for name, M in (('B', B), ('D', D)):
        assert M.format == 'csr' and tuple(M.shape) == tuple(g[f'{t}_{name}_shape'])
        assert np.array_equal(M.indptr, g[f'{t}_{name}_indptr'])
        assert np.array_equal(M.indices, g[f'{t}_{name}_indices'])    # bit-exact indexing
        assert np.array_equal(M.data, g[f'{t}_{name}_data'])          # and bit-exact values
    assert relerr(K.toarray(), g[f'{t}_K']) <= TOL_K
    # our pattern is a superset of the reference's value-dependent one
    assert not np.logical_and(g[f'{t}_K'] != 0, K.toarray() == 0).any()
    assert K.has_sorted_indices


# ---- a1..a5 ---------------------------------------------------------------------------
def _set_route(fep, monkeypatch, route, types):
    """FEP_ROUTE for `route` (unset for the default one: a value the session was started with must not leak in), then a
    context on a tiny mesh of every type in `types` must run that route: a switch the library ignores fails here."""
    if route in ('node', 'default'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    for t in types:
        m = fep.square_mesh(2, t, 10)
        ctx = fep.MeshContext(m['elements'], m['coordinates'])
        assert_route(ctx, 'patch' if route == 'default' else route)
        ctx.close()


@pytest.fixture(params=['node', 'patch', 'coo'])
def p1_route(request, monkeypatch, fep):
    """P1 routes: the node-centric fast path (default: one fused kernel per K,F-only step, two kernels otherwise) and, as
    independent cross-checks, the element route every other type runs — FEP_ROUTE=patch: K_e summed in LDS, FEP_ROUTE=coo:
    K_e through HBM.  (The measured-slower variants of the node route live in the -DFEP_ABLATION build only.)"""
    _set_route(fep, monkeypatch, request.param, ('P1',))
    return request.param


def test_p1_routes_agree_and_match_reference(fep, p1_route):
    test_hot_path_vs_reference_golden(fep, 'P1', True)
    test_hot_path_vs_reference_golden(fep, 'P1', False)
    test_hot_path_mid_size_vs_oracle(fep, 'P1', 60)


def _p1_case(fep, name):
    rng = np.random.default_rng(12)
    if name in ('rows', 'random'):
        from scipy.spatial import Delaunay
        M = 40
        g = np.stack(np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing='xy')).reshape(2, -1).astype(float)
        inner = (g[0] > 0) & (g[0] < M) & (g[1] > 0) & (g[1] < M)
        g[:, inner] += rng.uniform(-0.35, 0.35, size=(2, int(inner.sum())))
        coord = g * (10.0 / M)
        if name == 'random':
            coord = coord[:, rng.permutation(coord.shape[1])]
        elem = Delaunay(coord.T).simplices.T.astype(np.int64)
        if name == 'random':
            elem = elem[:, rng.permutation(elem.shape[1])]
    else:
        N = {'square150': 150, 'square7': 7, 'hetero': 90, 'tsx': 64}[name]
        mesh = fep.square_mesh(N, 'P1', 10)
        elem, coord = mesh['elements'], mesh['coordinates'].copy()
        inner = np.logical_and.reduce([coord[0] > 0, coord[0] < 10, coord[1] > 0, coord[1] < 10])
        coord[:, inner] += rng.uniform(-0.1, 0.1, size=(2, inner.sum())) * (10 / N)
    n = elem.shape[1]
    mats = dp_materials(n)
    if name == 'hetero':
        mats = [v * rng.uniform(0.8, 1.25, n) for v in mats]
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    U += rng.normal(0, 3e-6, size=U.shape)
    Ep = rng.normal(0, 5e-6, size=(4, n))
    e0 = np.array([-3e-5, 2e-5, 0.0, -4e-5]) if name == 'tsx' else None
    return elem, coord, mats, U, Ep, e0


@pytest.mark.parametrize('name', ['square150', 'square7', 'hetero', 'tsx', 'rows', 'random'])
def test_p1_fused_step_is_bitwise_the_two_kernel_route(fep, monkeypatch, name):
    """A non-accepting P1 step runs as ONE kernel (return map inside the assembly kernel's staging phase, s / ds never
    in HBM unless asked for).  Bit for bit the two-kernel route: K, F with and without the point outputs, s, ds, ind_p,
    strain, counters — structured and Delaunay meshes (run-compressed and list tables), per-point materials, e0."""
    elem, coord, mats, U, Ep, e0 = _p1_case(fep, name)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(*mats)
    ep = Ep.copy()
    kw = {} if e0 is None else {'e0': e0}
    full = ctx.step(U, ep, want=('E', 's', 'ds', 'ind_p', 'K', 'F'), **kw)        # point outputs wanted: two kernels
    scrub(ctx, U, Ep, kw)                     # between the forms: none passes with what the one before left on the device
    kf = ctx.step(U, ep, want=('K', 'F'), **kw)                                    # the one-kernel step
    scrub(ctx, U, Ep, kw)
    k_only = ctx.step(U, ep, want=('K',), **kw)
    scrub(ctx, U, Ep, kw)
    f_only = ctx.step(U, None, want=('F',), **kw)
    scrub(ctx, U, Ep, kw)
    f_zero_ep = ctx.step(U, np.zeros_like(Ep), want=('s', 'F'), **kw)              # two kernels, the state f_only ran on
    assert np.array_equal(ep, Ep)
    scrub(ctx, U, Ep, kw)
    K2, F2 = ctx.assemble(full['ds'], full['s'])                                   # assembly kernel alone on the stored ds / s
    ctx.close()
    assert full['n_smooth'] > 0 and full['n_apex'] > 0
    assert np.array_equal(full['K'].data, kf['K'].data) and np.array_equal(full['F'], kf['F'])
    assert np.array_equal(full['K'].data, k_only['K'].data) and np.array_equal(f_only['F'], f_zero_ep['F'])
    assert np.array_equal(K2.data, full['K'].data) and np.array_equal(F2, full['F'])


def test_p1_mesh_with_a_node_of_no_element(fep, p1_route):
    """A node that belongs to no element has no block in K and no lane that writes its force: F must still come back
    as zero there on every route (the reference's B^T product gives 0), not as uninitialised memory."""
    mesh = fep.square_mesh(12, 'P1', 10)
    elem, coord = mesh['elements'], mesh['coordinates']
    n_n = coord.shape[1]
    coord = np.concatenate([coord[:, :50], [[3.3], [4.4]], coord[:, 50:], [[20.0], [20.0]]], axis=1)   # orphans: id 50 and the last
    elem = np.where(elem >= 50, elem + 1, elem)
    n = elem.shape[1]
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(*dp_materials(n))
    F_poison = ctx.step(1e3 * U, None, want=('F',))['F']                       # leaves other values in freed device memory
    r = ctx.step(U, np.zeros((4, n)), want=('s', 'ds', 'K', 'F'))
    assert r['F'][2 * 50] == 0 and r['F'][2 * 50 + 1] == 0 and r['F'][-1] == 0 and r['F'][-2] == 0
    d1, d2, wf = fep.element_tables('P1')
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, *dp_materials(n)[:2], d1, d2, wf)
    sh, bu, eta, c = dp_materials(n)
    E, cp, K_t, F = orc.hot_path(U, np.zeros((4, n)), dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=sh,
                                                          bulk=bu, eta=eta, c=c))
    assert relerr(r['F'], F) <= TOL_K and np.abs((r['K'] - K_t).data).max() <= TOL_K * np.abs(K_t.data).max()
    assert r['K'].shape == (2 * (n_n + 2), 2 * (n_n + 2))
    K2, F2 = ctx.assemble(r['ds'], r['s'])
    assert np.array_equal(F2, r['F'])
    # transform: the weighted mean over no element is 0/0 = NaN, as the reference's F1 / F2 (DP:812); finite elsewhere
    qn = ctx.transform(r['s'][1])
    assert np.isnan(qn[50]) and np.isnan(qn[-1]) and np.isfinite(np.delete(qn, [50, qn.size - 1])).all()
    ctx.close()


@pytest.fixture(params=['patch', 'coo'])
def gen_route(request, monkeypatch, fep):
    """P2 / Q1 / Q2 (and P4): the element route in its patch form (default: K_e stays in LDS) and, as the independent
    cross-check, with the K_e round trip through HBM (FEP_ROUTE=coo)."""
    _set_route(fep, monkeypatch, 'default' if request.param == 'patch' else 'coo', ('P2', 'Q1', 'Q2'))
    return request.param


def test_route_switches_are_read_at_every_context_creation(fep, monkeypatch):
    """FEP_ROUTE is read by each fep_ctx_create, not once per process: in one process a context made with the switch
    set runs the switched route and the next one, made without it, the default route again (both ways, P2 and P1)."""
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    for t, route, default in (('P2', 'coo', 'patch'), ('P1', 'patch', 'node'), ('P2', 'coo', 'patch')):
        m = fep.square_mesh(3, t, 10)
        for r in (route, default):
            if r == default:
                monkeypatch.delenv('FEP_ROUTE', raising=False)
            else:
                monkeypatch.setenv('FEP_ROUTE', r)
            ctx = fep.MeshContext(m['elements'], m['coordinates'])
            assert_route(ctx, r)
            ctx.close()


def _patch_cases(fep):
    rng = np.random.default_rng(77)
    out = {}
    for t, n in (('P2', 37), ('Q1', 45), ('Q2', 23), ('P1', 52)):
        m = fep.square_mesh(n, t, 10)
        out[f'square_{t}'] = (m['elements'], m['coordinates'])
    g = load_golden('tsx')
    out['tsx_P1'] = (g['elem'], g['coord'])
    out['tsx_P2'] = (g['p2_elem'], g['p2_coord'])
    out['tsx_P4'] = (g['p4_elem'], g['p4_coord'])
    m = fep.square_mesh(14, 'P2', 10)                                       # randomly numbered elements and nodes: patches
    perm = rng.permutation(m['coordinates'].shape[1])                       # without locality, many partials per block
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    out['shuffled_P2'] = (inv[m['elements'][:, rng.permutation(m['elements'].shape[1])]], m['coordinates'][:, perm])
    m = fep.square_mesh(12, 'Q2', 10)                                       # two nodes of no element
    co = m['coordinates']
    out['orphans_Q2'] = (np.where(m['elements'] >= 50, m['elements'] + 1, m['elements']),
                         np.concatenate([co[:, :50], [[3.3], [4.4]], co[:, 50:], [[20.0], [20.0]]], axis=1))
    m = fep.square_mesh(1, 'P2', 10)                                        # a single patch: nothing open
    out['one_cell_P2'] = (m['elements'], m['coordinates'])
    for t, k in (('P1', 16), ('P1', 255), ('P2', 85)):                      # one node of k elements (tests/fan_mesh.py):
        elem, coord = fan_mesh(k, t, shuffle=k % 2 == 1)                    # P1's element route, a row of 256 blocks
        out[f'fan{k}_{t}'] = (elem, 5 + 2.5 * coord)                        # (the displacement below expects [0, 10]^2)
    return out


@pytest.mark.parametrize('name', ['square_P2', 'square_Q1', 'square_Q2', 'square_P1', 'tsx_P1', 'tsx_P2', 'tsx_P4', 'shuffled_P2',
                                  'orphans_Q2', 'one_cell_P2', 'fan16_P1', 'fan255_P1', 'fan85_P2'])
def test_patch_route_against_the_coo_route(fep, monkeypatch, name):
    """Element route, patch form (K_e blocks summed inside the workgroup's LDS, partials only for node pairs on a patch
    boundary) against the COO form (every K_e block through HBM, one flat sum per CSR block): the point outputs are the same
    kernel code (bit-identical), K and F differ by the association of the sums only (<= 1e-13 of the array maximum, every
    row of K <= 1e-12 of its own maximum); step and assemble_tangent agree bit for bit on each route; run-to-run bitwise
    reproducible.  The plan is replayed against the symbolic phase (FEP_VALIDATE_PLAN)."""
    elem, coord = _patch_cases(fep)[name]
    n_p = elem.shape[0]
    t = {3: 'P1', 6: 'P2', 4: 'Q1', 8: 'Q2', 15: 'P4'}[n_p]
    n = elem.shape[1] * NQ[t]
    rng = np.random.default_rng(5)
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    U += rng.normal(0, 3e-6, size=U.shape)
    Ep = rng.normal(0, 5e-6, size=(4, n))
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    res = {}
    routes = ('coo', 'patch')
    for route in routes:
        monkeypatch.setenv('FEP_ROUTE', route)                                # (P1 too: its node route is not what is compared here)
        ctx = fep.MeshContext(elem, coord)
        assert_route(ctx, route)
        ctx.set_materials(*dp_materials(n))
        F_poison = ctx.step(1e3 * U, None, want=('K', 'F'))                   # other values in the scratch buffers
        r = ctx.step(U, Ep.copy(), want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
        r2 = ctx.step(U, Ep.copy(), want=('K', 'F'))                          # K,F-only call: same values
        assert np.array_equal(r2['K'].data, r['K'].data) and np.array_equal(r2['F'], r['F'])
        ep = Ep.copy()
        acc = ctx.step(U, ep, apply_plastic_strain=True, want=('K', 'F'))
        assert np.array_equal(acc['K'].data, r['K'].data) and np.array_equal(acc['F'], r['F'])
        K2, F2 = ctx.assemble(r['ds'], r['s'])
        assert np.array_equal(K2.data, r['K'].data) and np.array_equal(F2, r['F'])
        _, F3 = ctx.assemble(None, r['s'])
        K3, _ = ctx.assemble(r['ds'], None)
        assert np.array_equal(F3, r['F']) and np.array_equal(K3.data, r['K'].data)
        res[route] = (r, ep)
        ctx.close()
    a = res['coo'][0]
    for route in routes[1:]:
        b = res[route][0]
        assert (a['n_smooth'] > 0 or n < 100) and (a['n_smooth'], a['n_apex']) == (b['n_smooth'], b['n_apex'])
        for k in ('E', 's', 'ds', 'ind_p'):
            assert np.array_equal(a[k], b[k]), (route, k)
        assert np.array_equal(res['coo'][1], res[route][1])
        assert relerr(b['K'].data, a['K'].data) <= 1e-13 and relerr(b['F'], a['F']) <= 1e-13
        assert relerr_rows(b['K'], a['K']) <= 1e-12
        if name == 'orphans_Q2':
            assert b['F'][2 * 50] == 0 and b['F'][2 * 50 + 1] == 0 and b['F'][-1] == 0 and b['F'][-2] == 0


@pytest.mark.parametrize('t,N', [('P2', 24), ('Q1', 40), ('Q2', 20)])
def test_generic_routes_agree_and_match_reference(fep, gen_route, t, N):
    test_hot_path_vs_reference_golden(fep, t, True)
    test_hot_path_vs_reference_golden(fep, t, False)
    test_hot_path_mid_size_vs_oracle(fep, t, N)


@pytest.mark.parametrize('t', ELS)
@pytest.mark.parametrize('accept', [False, True])
def test_hot_path_vs_reference_golden(fep, t, accept):
    g = load_golden('hotpath_dp')
    d1, d2, wf = tables('dp', t)
    elem, coord = g[f'{t}_elements'], g[f'{t}_coordinates']
    n_int = elem.shape[1] * NQ[t]
    sh, bu, eta, c = dp_materials(n_int)
    ctx = fep.MeshContext(elem, coord, d1, d2, wf)
    ctx.set_materials(sh, bu, eta, c)
    tag = f'{t}_acc{int(accept)}_'
    ep = g[f'{t}_Ep_old'].copy()
    r = ctx.step(g[f'{t}_U'], ep, apply_plastic_strain=accept, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    assert relerr(r['E'], g[tag + 'E']) <= 1e-14
    assert np.array_equal(r['ind_p'], g[tag + 'ind_p'])
    assert relerr(r['s'], g[tag + 's']) <= TOL_PT and relerr(r['ds'], g[tag + 'ds']) <= TOL_PT
    assert relerr_points(r['s'], g[tag + 's']) <= TOL_PT_EACH and relerr_points(r['ds'], g[tag + 'ds']) <= TOL_PT_EACH
    assert relerr(r['K'].toarray(), g[tag + 'K_t']) <= TOL_K
    assert relerr_rows(r['K'].toarray(), g[tag + 'K_t']) <= TOL_K_EACH
    assert relerr(r['F'], g[tag + 'F']) <= TOL_K
    if accept:
        assert relerr(ep, g[tag + 'ep']) <= TOL_PT
    else:
        assert np.array_equal(ep, g[f'{t}_Ep_old'])
    # unfused route (drop-in for the inline DP:1047-1058): same K, F from the returned ds, s
    K2, F2 = fep.assemble_tangent(ctx, r['ds'], r['s'])
    assert np.array_equal(K2.data, r['K'].data) and np.array_equal(F2, r['F'])
    # run-to-run bitwise reproducible (no atomics in the value path)
    r2 = ctx.step(g[f'{t}_U'], g[f'{t}_Ep_old'].copy(), apply_plastic_strain=accept, want=('K', 'F', 's'))
    assert np.array_equal(r2['K'].data, r['K'].data) and np.array_equal(r2['F'], r['F'])
    ctx.close()


# ---- config 3: tsx-tunnel CSV dumps ------------------------------------------------------
def _tsx_ctx(fep, t, coord, elem):
    d1, d2, wf = tables('tsx', t) if t != 'P1' else tables('dp', 'P1')
    n_int = elem.shape[1] * NQ[t]
    G = 60000 / (2 * (1 + 0.2)) * np.ones(n_int)
    Kb = 60000 / (3 * (1 - 2 * 0.2)) * np.ones(n_int)
    K, B, w, iD, jD, D = fep.tsx_tunnel.get_elastic_stiffness_matrix(elem, coord, G, Kb, d1, d2, wf)
    Q = np.ones(coord.shape, dtype=bool)
    Q[0, np.abs(coord[0]) > 49.99] = 0
    Q[1, np.abs(coord[1]) > 49.99] = 0
    return K, B, w, Q


def test_tsx_p1_tangent_vs_k_tangent_qq_csv(fep):
    g = load_golden('tsx')
    K, B, w, Q = _tsx_ctx(fep, 'P1', g['coord'], g['elem'])
    qf = Q.flatten(order='F')
    Kqq = K[qf][:, qf].toarray()
    ref = ssp.coo_matrix((g['p1_Kqq_val'], (g['p1_Kqq_row'], g['p1_Kqq_col'])), shape=(908, 908)).toarray()
    assert relerr(Kqq, ref) <= TOL_K
    csv = ssp.coo_matrix((g['kqq_val'], (g['kqq_row'], g['kqq_col'])), shape=(908, 908)).toarray()
    assert not np.logical_and(csv != 0, Kqq == 0).any()                    # CSV pattern is covered
    assert np.abs(Kqq - csv).max() <= 1e-4 * np.abs(csv).max()             # MATLAB dump, un-rounded coordinates


def test_tsx_p2_load_vs_f0q_csv_and_p4(fep):
    g = load_golden('tsx')
    K, B, w, Q = _tsx_ctx(fep, 'P2', g['p2_coord'], g['p2_elem'])
    s0 = np.array([-45.0, -11.0, 0.0, -60.0]).reshape((-1, 1)) * np.ones((1, w.size))
    _, F0 = fep.assemble_tangent(K, None, s0)                              # TSX:1737
    F0 = F0.reshape((2, -1), order='F')
    assert relerr(F0, g['p2_F0']) <= TOL_K
    assert np.abs(F0.T[Q.T] - g['f0q']).max() <= 2e-4 * np.abs(g['f0q']).max()
    assert relerr(K.diagonal(), g['p2_K_diag']) <= TOL_K
    K4, B4, w4, Q4 = _tsx_ctx(fep, 'P4', g['p4_coord'], g['p4_elem'])
    assert relerr(K4.diagonal(), g['p4_K_diag']) <= 1e-11
    assert abs(np.sqrt((K4.data ** 2).sum()) - g['p4_K_frob']) <= 1e-11 * g['p4_K_frob']
    assert abs(w4.sum() - g['p4_weight_sum']) <= 1e-13 * g['p4_weight_sum']


def test_tsx_p1_replay_state_vs_reference(fep):
    """Hot path on the reference's converged TSX displacement (step 17, 3 plastic points)."""
    g = load_golden('tsx')
    coord, elem = g['coord'], g['elem']
    n_int = elem.shape[1]
    G = 60000 / (2 * (1 + 0.2)) * np.ones(n_int)
    Kb = 60000 / (3 * (1 - 2 * 0.2)) * np.ones(n_int)
    fr = 49 * np.pi / 180
    eta = 3 * np.tan(fr) / np.sqrt(9 + 12 * np.tan(fr) ** 2) * np.ones(n_int)
    c = 3 * 18.7 / np.sqrt(9 + 12 * np.tan(fr) ** 2) * np.ones(n_int)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(G, Kb, eta, c)
    r = ctx.step(g['p1_U_final'], np.zeros((4, n_int)), e0=1.0 * g['init_strain'], want=('ind_p', 's', 'K', 'F'))
    assert int(r['ind_p'].sum()) == int(g['p1_nplast'][-1]) == 3
    d1, d2, wf = tables('dp', 'P1')
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, G, Kb, d1, d2, wf)
    E, cp, K_t, F = orc.hot_path(g['p1_U_final'], np.zeros((4, n_int)),
                                 dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=G, bulk=Kb, eta=eta, c=c),
                                 e0=1.0 * g['init_strain'], tsx=True)
    assert np.array_equal(r['ind_p'], cp['ind_p'])
    assert relerr(r['K'].toarray(), K_t.toarray()) <= TOL_K and relerr(r['F'], F) <= TOL_K
    # converged state: residual on the free DOFs vanishes (fq.csv is ~1e-15)
    Q = np.ones(coord.shape, dtype=bool)
    Q[0, np.abs(coord[0]) > 49.99] = 0
    Q[1, np.abs(coord[1]) > 49.99] = 0
    assert np.abs(r['F'][Q.flatten(order='F')]).max() <= 1e-9 * np.abs(r['F']).max()


# ---- config 1: Elasticity2D P1 K ----------------------------------------------------------
@pytest.mark.parametrize('level,nnz,trace,frob', [(1, 7680, 4.215902547065e+08, 2.054604152327e+07),
                                                 (3, 117120, 6.745444075305e+09, 8.396141008266e+07)])
def test_el_p1_K_pins(fep, level, nnz, trace, frob):
    g = load_golden('el_p1')
    d1, d2, wf = tables('dp', 'P1')
    elem1 = g[f'l{level}_elements_1based'].astype(np.int64)
    coord = g[f'l{level}_coordinates']
    n_int = elem1.shape[1]
    G = 206900 / (2 * (1 + 0.29)) * np.ones(n_int)
    Kb = 206900 / (3 * (1 - 2 * 0.29)) * np.ones(n_int)
    K, w = fep.elasticity2d.get_elastic_stiffness_matrix(elem1, coord, G, Kb, d1, d2, wf)
    assert elem1.min() == 0                                       # shifted in place like EL:389
    Kz = K.copy()
    Kz.data[np.abs(Kz.data) < 1e-9 * np.abs(Kz.data).max()] = 0   # SciPy drops exact zeros (C9)
    Kz.eliminate_zeros()
    assert Kz.nnz == nnz
    assert abs(K.diagonal().sum() - trace) <= 1e-12 * trace
    assert abs(np.sqrt((K.data ** 2).sum()) - frob) <= 1e-12 * frob
    assert abs(w.sum() - 75.0) <= 1e-12 * 75
    assert relerr(K @ np.cos(np.arange(K.shape[0]) * 0.37), g[f'l{level}_Kx']) <= TOL_K


# ---- mid size vs oracle, every element type ------------------------------------------------
@pytest.mark.parametrize('t,N', [('P1', 60), ('P2', 24), ('Q1', 40), ('Q2', 20), ('P4', 10)])
def test_hot_path_mid_size_vs_oracle(fep, t, N, heterogeneous=False):
    rng = np.random.default_rng(5)
    elem, coord = square_mesh_of(t, N)                   # (P4: the P1 square raised by create_midpoints_P4)
    inner = np.logical_and.reduce([coord[0] > 0, coord[0] < 10, coord[1] > 0, coord[1] < 10])
    coord[:, inner] += rng.uniform(-0.1, 0.1, size=(2, inner.sum())) * (10 / N) / {'P2': 2, 'Q2': 2, 'P4': 4}.get(t, 1)
    d1, d2, wf = fep.element_tables(t)
    n_int = elem.shape[1] * NQ[t]
    sh, bu, eta, c = dp_materials(n_int)
    if heterogeneous:                 # per-point parameters (the kernels' array path; constants take a fast path)
        sh, bu, eta, c = [v * rng.uniform(0.8, 1.25, n_int) for v in (sh, bu, eta, c)]
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    U += rng.normal(0, 3e-6, size=U.shape)
    Ep = rng.normal(0, 5e-6, size=(4, n_int))
    ctx = fep.MeshContext(elem, coord, d1, d2, wf)
    ctx.set_materials(sh, bu, eta, c)
    ep = Ep.copy()
    r = ctx.step(U, ep, apply_plastic_strain=True, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, sh, bu, d1, d2, wf)
    ep_o = Ep.copy()
    E, cp, K_t, F = orc.hot_path(U, ep_o, dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=sh, bulk=bu,
                                                eta=eta, c=c), apply_plastic_strain=True)
    assert 0 < cp['n_smooth'] and 0 < cp['n_apex'] < 20000 and cp['n_smooth'] + cp['n_apex'] < n_int
    assert (r['n_smooth'], r['n_apex']) == (cp['n_smooth'], cp['n_apex'])
    assert np.array_equal(r['ind_p'], cp['ind_p'])
    assert relerr(r['E'], E) <= 1e-13
    assert relerr(r['s'], cp['s']) <= TOL_PT and relerr(r['ds'], cp['ds']) <= TOL_PT and relerr(ep, ep_o) <= TOL_PT
    assert relerr_points(r['s'], cp['s']) <= TOL_PT_EACH and relerr_points(r['ds'], cp['ds']) <= TOL_PT_EACH
    diff = (r['K'] - K_t)
    assert np.abs(diff.data).max() <= TOL_K * np.abs(K_t.data).max()
    assert relerr_rows(r['K'], K_t) <= TOL_K_EACH
    assert relerr(r['F'], F) <= TOL_K


@pytest.mark.parametrize('t,N', [('P1', 60), ('P2', 20), ('Q1', 30), ('Q2', 12), ('P4', 8)])
def test_heterogeneous_materials_vs_oracle(fep, t, N):
    test_hot_path_mid_size_vs_oracle(fep, t, N, heterogeneous=True)


def test_constant_materials_fast_path_is_bitwise_the_array_path(fep):
    """Materials constant over the mesh (the reference's demos) are passed to the kernels as scalars, the four arrays are not
    read; any other set of arrays takes the array path.  Same values bit for bit: the second context differs from the first
    in the cohesion of the LAST element's points only, so every other point, and every row / force entry of a node outside
    that element, must come out identical."""
    mesh = fep.square_mesh(30, 'P2', 10)
    elem = mesh['elements']
    n_int = elem.shape[1] * 7
    x, y = mesh['coordinates']
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    res = []
    for perturbed in (False, True):
        mats = [v.copy() for v in dp_materials(n_int)]
        if perturbed:
            mats[3][-7:] *= 1.5
        ctx = fep.MeshContext(elem, mesh['coordinates'])
        ctx.set_materials(*mats)
        res.append(ctx.step(U, np.zeros((4, n_int)), want=('s', 'ds', 'K', 'F')))
        ctx.close()
    assert res[0]['n_smooth'] > 0
    for k in ('s', 'ds'):
        assert np.array_equal(res[0][k][:, :-7], res[1][k][:, :-7])
    outside = np.ones(mesh['coordinates'].shape[1], dtype=bool)
    outside[elem[:, -1]] = False
    rows = np.repeat(outside, 2)
    assert np.array_equal(res[0]['F'][rows], res[1]['F'][rows])
    K0, K1 = res[0]['K'].tocsr(), res[1]['K'].tocsr()
    assert np.array_equal(K0[rows].data, K1[rows].data)


# ---- full benchmark size: properties (the reference cannot run here: DP:714 needs n_apex^2 memory) ----
def test_full_size_p1_properties(fep):
    N = 708                                                   # 1 002 528 P1 elements (config 4)
    mesh = fep.square_mesh(N, 'P1', 10)
    elem, coord = mesh['elements'], mesh['coordinates']
    n_e = elem.shape[1]
    assert n_e == 1002528
    sh, bu, eta, c = dp_materials(n_e)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(sh, bu, eta, c)
    _, _, w, det = ctx.geometry()
    assert abs(w.sum() - 100.0) <= 1e-9                       # sum of weights = area
    assert (det > 0).all()
    # (1) all elastic: K_tangent == K_elast, F == K_elast U
    rng = np.random.default_rng(1)
    U0 = rng.normal(0, 1e-9, size=(2, coord.shape[1]))
    r0 = ctx.step(U0, want=('K', 'F', 'ind_p'))
    assert not r0['ind_p'].any()
    Kel = ctx.step(np.zeros_like(U0), want=('K',))['K']
    assert np.array_equal(r0['K'].data, Kel.data)
    assert relerr(r0['F'], Kel @ U0.reshape(-1, order='F')) <= 1e-10
    assert np.abs(Kel - Kel.T).data.max() <= 1e-12 * np.abs(Kel.data).max()     # symmetry
    rigid = np.tile([1.0, 0.0], coord.shape[1])
    assert np.abs(Kel @ rigid).max() <= 1e-9 * np.abs(Kel.data).max()           # translations in the kernel
    # (2) mixed state: sampled elements against the oracle's per-point map + symmetric tangent
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    U += rng.normal(0, 2e-8, size=U.shape)
    r = ctx.step(U, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    assert r['n_smooth'] > 1e5 and r['n_apex'] > 1e4 and r['n_smooth'] + r['n_apex'] < n_e
    sel = rng.choice(n_e, 4000, replace=False)
    o = orc.return_map(r['E'][:, sel], None, sh[sel], bu[sel], eta[sel], c[sel])
    assert np.array_equal(o['ind_p'], r['ind_p'][sel])
    assert relerr(r['s'][:, sel], o['s']) <= TOL_PT and relerr(r['ds'][:, sel], o['ds']) <= TOL_PT
    Kt = r['K']
    assert np.abs(Kt - Kt.T).data.max() <= 1e-12 * np.abs(Kt.data).max()
    assert np.abs(Kt @ rigid).max() <= 1e-9 * np.abs(Kt.data).max()
    # F is linear in s: F(s) from the unfused route equals the fused one bit for bit
    _, F2 = ctx.assemble(None, r['s'])
    assert np.array_equal(F2, r['F'])
    # (3) the WHOLE result against the oracle at full size (the reference itself cannot run this state: 574 k apex points make
    # its n_apex x n_apex temporary, DP:714; the oracle restates the same path without it): every point, every row of K
    d1t, d2t, wft = fep.element_tables('P1')
    Ko, Bo, wo, iDo, jDo, Do = orc.elastic_setup(elem, coord, sh, bu, d1t, d2t, wft)
    Eo, cpo, Kto, Fo = orc.hot_path(U, np.zeros((4, n_e)), dict(K_elast=Ko, B=Bo, D_elast=Do, weight=wo, iD=iDo, jD=jDo,
                                                                 shear=sh, bulk=bu, eta=eta, c=c))
    assert (cpo['n_smooth'], cpo['n_apex']) == (r['n_smooth'], r['n_apex']) and np.array_equal(r['ind_p'], cpo['ind_p'])
    assert relerr(r['E'], Eo) <= 1e-13
    assert relerr(r['s'], cpo['s']) <= TOL_PT and relerr(r['ds'], cpo['ds']) <= TOL_PT
    assert relerr_points(r['s'], cpo['s']) <= TOL_PT_EACH and relerr_points(r['ds'], cpo['ds']) <= TOL_PT_EACH
    assert np.abs((Kt - Kto).data).max() <= TOL_K * np.abs(Kto.data).max()
    # every row against the larger of its own and K_elast's largest entry: the oracle (like the reference, DP:1050) forms
    # K_elast + B^T (D_p - D_elast) B, so a row whose points all sit at the apex is a difference of two numbers of K_elast's
    # size there (1e-9 of round-off where the kernels' B^T D_p B gives the exact zero); with 574 k apex points such rows exist
    dK = abs(Kt - Kto).tocsr()
    d_row = np.asarray(dK.max(axis=1).todense()).ravel()
    s_row = np.maximum(np.asarray(abs(Kto).max(axis=1).todense()).ravel(), np.asarray(abs(Ko).max(axis=1).todense()).ravel())
    assert (d_row <= TOL_K_EACH * s_row).all()
    assert relerr(r['F'], np.asarray(Fo).ravel()) <= TOL_K
    del Ko, Bo, Do, Kto
    # strain of sampled elements against a direct evaluation
    d1, d2, wgt, _ = ctx.geometry()
    nodes = elem[:, sel]
    ux, uy = U[0][nodes], U[1][nodes]
    E_dir = np.array([(d1[:, sel] * ux).sum(0), (d2[:, sel] * uy).sum(0), (d2[:, sel] * ux + d1[:, sel] * uy).sum(0)])
    assert relerr(r['E'][:, sel], E_dir) <= 1e-13
    ctx.close()


def test_misaligned_device_vectors_are_refused(fep):
    """The kernels move U, F and the CSR values as 16-byte pairs: an odd-double offset must come back as an error code,
    never reach a kernel."""
    import torch
    mesh = fep.square_mesh(8, 'P1', 10)
    ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'])
    ctx.set_materials(*[v[0] for v in dp_materials(1)])
    dev = torch.device('cuda', 0)
    buf = torch.zeros(ctx.n_dof + 2, dtype=torch.float64, device=dev)
    F = torch.zeros(ctx.n_dof + 2, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ctx.step_dev(st, buf.data_ptr(), f_out=F.data_ptr())                                   # aligned: fine
    with pytest.raises(fep.FepError, match='invalid argument'):
        ctx.step_dev(st, buf.data_ptr() + 8, f_out=F.data_ptr())
    with pytest.raises(fep.FepError, match='invalid argument'):
        ctx.step_dev(st, buf.data_ptr(), f_out=F.data_ptr() + 8)
    torch.cuda.synchronize()
    ctx.close()


def test_error_codes(fep):
    elem = np.array([[0], [1], [5]])                      # node id out of range
    coord = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(IndexError):
        fep.MeshContext(elem, coord)
    import ctypes as C
    l = fep.lib()
    h = C.c_void_p()
    el32 = np.array([[0], [1], [7]], dtype=np.int32)
    d1, d2, wf = fep.element_tables('P1')
    rc = l.fep_ctx_create(C.byref(h), 0, 1, 1, 3, el32.ctypes.data, coord.ctypes.data, d1.ctypes.data, d2.ctypes.data,
                          wf.ctypes.data)
    assert rc == -5 and not h                             # FEP_ERANGE, no context
    assert l.fep_ctx_create(C.byref(h), 0, 9, 1, 3, el32.ctypes.data, coord.ctypes.data, d1.ctypes.data, d2.ctypes.data,
                            wf.ctypes.data) == -1        # unknown element type
    ctx = fep.MeshContext(np.array([[0], [1], [2]]), coord)
    with pytest.raises(fep.FepError):                     # materials not set -> FEP_ESTATE
        ctx.step(np.zeros(6))


# ---- P4 (15 nodes, 12 points; TSX only) and ragged sizes ---------------------------------------------
def test_p4_hot_path_vs_oracle_on_tsx_mesh(fep):
    g = load_golden('tsx')
    coord, elem = g['p4_coord'], g['p4_elem']
    d1, d2, wf = tables('tsx', 'P4')
    n_int = elem.shape[1] * 12
    G = 60000 / (2 * (1 + 0.2)) * np.ones(n_int)
    Kb = 60000 / (3 * (1 - 2 * 0.2)) * np.ones(n_int)
    fr = 49 * np.pi / 180
    eta = 3 * np.tan(fr) / np.sqrt(9 + 12 * np.tan(fr) ** 2) * np.ones(n_int)
    c = 3 * 18.7 / np.sqrt(9 + 12 * np.tan(fr) ** 2) * np.ones(n_int)
    rng = np.random.default_rng(8)
    x, y = coord
    U = np.array([4e-4 * x + 1e-4 * y, -6e-4 * y]) + rng.normal(0, 2e-5, size=coord.shape)
    e0 = g['init_strain']
    ctx = fep.MeshContext(elem, coord, d1, d2, wf)
    ctx.set_materials(G, Kb, eta, c)
    ep = np.zeros((4, n_int))
    r = ctx.step(U, ep, e0=e0, apply_plastic_strain=True, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, G, Kb, d1, d2, wf)
    ep_o = np.zeros((4, n_int))
    E, cp, K_t, F = orc.hot_path(U, ep_o, dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=G, bulk=Kb,
                                                eta=eta, c=c), apply_plastic_strain=True, e0=e0, tsx=True)
    assert cp['n_smooth'] > 0 and cp['n_smooth'] + cp['n_apex'] < n_int
    assert (r['n_smooth'], r['n_apex']) == (cp['n_smooth'], cp['n_apex'])
    assert np.array_equal(r['ind_p'], cp['ind_p'])
    # P4 tolerances are one decade above the other element types': the degree-4 shape-function derivatives on this mesh
    # (element sizes 0.1 ... 10, coordinates up to 50) span four decades and the strain sums 15 node terms of mixed
    # sign, so E itself agrees to 1e-12 only (different but fixed summation order: LDS-staged pairs here, a sparse
    # product in the oracle); s, ds inherit that, K sums 12 points x 15 x 15 such products.
    assert relerr(r['E'], E) <= 1e-12
    assert relerr(r['s'], cp['s']) <= 1e-12 and relerr(r['ds'], cp['ds']) <= 1e-12 and relerr(ep, ep_o) <= 1e-12
    assert np.abs((r['K'] - K_t).data).max() <= 1e-11 * np.abs(K_t.data).max()
    assert relerr(r['F'], F) <= 1e-11


@pytest.mark.parametrize('t,nx,ny', [('P1', 1, 1), ('P1', 3, 2), ('Q1', 1, 1), ('Q1', 5, 3), ('P2', 1, 1), ('P2', 3, 3), ('Q2', 2, 2),
                                     ('P4', 1, 1), ('P4', 3, 2)])
def test_tiny_and_ragged_meshes(fep, t, nx, ny):
    """Meshes far smaller than a workgroup tile, element counts that are not multiples of any block size."""
    if t in ('P1', 'Q1', 'P4'):
        elem, coord = rect_mesh_of(t, nx, ny, 2.0, 3.0)
    else:
        elem, coord = square_mesh_of(t, nx, 2.0)
    d1, d2, wf = fep.element_tables(t)
    n_int = elem.shape[1] * NQ[t]
    sh, bu, eta, c = dp_materials(n_int)
    rng = np.random.default_rng(nx * 7 + ny)
    U = rng.normal(0, 3e-4, size=coord.shape)
    ctx = fep.MeshContext(elem, coord, d1, d2, wf)
    ctx.set_materials(sh, bu, eta, c)
    r = ctx.step(U, None, want=('s', 'ds', 'ind_p', 'K', 'F'))
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, sh, bu, d1, d2, wf)
    E, cp, K_t, F = orc.hot_path(U, None, dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=sh, bulk=bu,
                                               eta=eta, c=c))
    assert np.array_equal(r['ind_p'], cp['ind_p'])
    assert relerr(r['s'], cp['s']) <= TOL_PT and relerr(r['ds'], cp['ds']) <= TOL_PT
    assert relerr(r['K'].toarray(), K_t.toarray()) <= TOL_K and relerr(r['F'], F) <= TOL_K


def test_p2_one_million_points_divergence_stress(fep):
    """BASELINE configs[4] in miniature on one GPU: P2, branches i.i.d. per point (worst-case divergence inside
    a wave); sampled points against the oracle's map, global invariants on K and F."""
    N = 270                                                   # 145 800 P2 elements, 1 020 600 points
    mesh = fep.square_mesh(N, 'P2', 10)
    elem, coord = mesh['elements'], mesh['coordinates']
    n_e = elem.shape[1]
    n_int = n_e * 7
    sh, bu, eta, c = dp_materials(n_int)
    rng = np.random.default_rng(17)
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10), -1.2e-4 * y]) + rng.normal(0, 2.5e-6, size=coord.shape)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(sh, bu, eta, c)
    r = ctx.step(U, None, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    n_el = n_int - r['n_smooth'] - r['n_apex']
    assert min(n_el, r['n_smooth'], r['n_apex']) > 0.1 * n_int          # all three branches heavily populated
    # neighbouring points differ in branch most of the time (divergence really happens inside waves)
    br = r['ind_p'].astype(np.int8) + (np.abs(r['ds']).sum(axis=0) == 0)
    assert (np.diff(br[:100000]) != 0).mean() > 0.3
    sel = rng.choice(n_int, 5000, replace=False)
    o = orc.return_map(r['E'][:, sel], None, sh[sel], bu[sel], eta[sel], c[sel])
    assert np.array_equal(o['ind_p'], r['ind_p'][sel])
    assert relerr(r['s'][:, sel], o['s']) <= TOL_PT and relerr(r['ds'][:, sel], o['ds']) <= TOL_PT
    K = r['K']
    assert np.abs(K - K.T).data.max() <= 1e-12 * np.abs(K.data).max()
    rigid = np.tile([0.0, 1.0], coord.shape[1])
    assert np.abs(K @ rigid).max() <= 1e-9 * np.abs(K.data).max()
    K2, F2 = ctx.assemble(r['ds'], r['s'])
    assert np.array_equal(K2.data, K.data) and np.array_equal(F2, r['F'])
    # sum of nodal forces = 0 for a self-equilibrated stress field integrated over the whole body (B^T s sums to zero
    # against rigid translations)
    assert abs(r['F'][0::2].sum()) <= 1e-9 * np.abs(r['F']).sum() and abs(r['F'][1::2].sum()) <= 1e-9 * np.abs(r['F']).sum()
    ctx.close()


@pytest.mark.parametrize('numbering', ['rows', 'random'])
def test_unstructured_delaunay_mesh_vs_oracle(fep, p1_route, numbering):
    """General connectivity: Delaunay triangulation of jittered points (node degrees 4..10, arbitrary orientation —
    the reference takes |det|), nodes and elements in generator order or randomly renumbered."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(4)
    M = 36
    g = np.stack(np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing='xy')).reshape(2, -1).astype(float)
    inner = (g[0] > 0) & (g[0] < M) & (g[1] > 0) & (g[1] < M)
    g[:, inner] += rng.uniform(-0.35, 0.35, size=(2, int(inner.sum())))
    coord = g * (10.0 / M)
    if numbering == 'random':
        coord = coord[:, rng.permutation(coord.shape[1])]
    elem = Delaunay(coord.T).simplices.T.astype(np.int64)
    if numbering == 'random':
        elem = elem[:, rng.permutation(elem.shape[1])]
        elem = np.where(rng.random(elem.shape[1]) < 0.5, elem, elem[[0, 2, 1]])       # mixed orientations
    n_e = elem.shape[1]
    deg = np.bincount(elem.ravel())
    assert deg.min() >= 1 and deg.max() >= 8
    d1, d2, wf = fep.element_tables('P1')
    sh, bu, eta, c = dp_materials(n_e)
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    Ep = rng.normal(0, 5e-6, size=(4, n_e))
    ctx = fep.MeshContext(elem, coord, d1, d2, wf)
    ctx.set_materials(sh, bu, eta, c)
    ep = Ep.copy()
    r = ctx.step(U, ep, apply_plastic_strain=True, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, sh, bu, d1, d2, wf)
    ep_o = Ep.copy()
    E, cp, K_t, F = orc.hot_path(U, ep_o, dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=sh, bulk=bu,
                                                eta=eta, c=c), apply_plastic_strain=True)
    assert cp['n_smooth'] > 0 and cp['n_apex'] > 0
    assert (r['n_smooth'], r['n_apex']) == (cp['n_smooth'], cp['n_apex']) and np.array_equal(r['ind_p'], cp['ind_p'])
    assert relerr(r['s'], cp['s']) <= TOL_PT and relerr(r['ds'], cp['ds']) <= TOL_PT and relerr(ep, ep_o) <= TOL_PT
    assert np.abs((r['K'] - K_t).data).max() <= TOL_K * np.abs(K_t.data).max()
    assert relerr(r['F'], F) <= TOL_K
    ctx.close()


def test_config5_full_size_p2_properties(fep):
    """BASELINE configs[4] at its full size on ONE GPU: 3 998 792 P2 elements = 27 991 544 integration points,
    branches i.i.d. per point.  The oracle cannot run this (and the reference even less); checked are the sampled
    points against the oracle's map and size-independent properties of K and F (symmetry and the rigid translations
    through products, the force balance, the fused against the unfused route)."""
    N = 1414
    mesh = fep.square_mesh(N, 'P2', 10)
    elem, coord = mesh['elements'], mesh['coordinates']
    n_e = elem.shape[1]
    n_int = n_e * 7
    assert (n_e, n_int, coord.shape[1]) == (3998792, 27991544, 8003241)
    sh, bu, eta, c = dp_materials(1)
    rng = np.random.default_rng(23)
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10), -1.2e-4 * y]) + rng.normal(0, 2.5e-6 * 270 / N, size=coord.shape)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(sh[0], bu[0], eta[0], c[0])
    r = ctx.step(U, None, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    n_el = n_int - r['n_smooth'] - r['n_apex']
    assert min(n_el, r['n_smooth'], r['n_apex']) > 0.1 * n_int
    assert (np.diff(r['ind_p'][:200000].astype(np.int8)) != 0).mean() > 0.2      # divergence inside waves
    sel = rng.choice(n_int, 5000, replace=False)
    one = np.ones(sel.size)
    o = orc.return_map(r['E'][:, sel], None, sh[0] * one, bu[0] * one, eta[0] * one, c[0] * one)
    assert np.array_equal(o['ind_p'], r['ind_p'][sel])
    assert relerr(r['s'][:, sel], o['s']) <= TOL_PT and relerr(r['ds'][:, sel], o['ds']) <= TOL_PT
    K, F = r['K'], r['F']
    assert K.nnz == ctx.nnz == 367979364
    kmax = np.abs(K.data).max()
    u, v = rng.normal(size=ctx.n_dof), rng.normal(size=ctx.n_dof)
    Ku, Kv = K @ u, K @ v
    assert abs(v @ Ku - u @ Kv) <= 1e-11 * (np.abs(v) @ np.abs(Ku))             # symmetry
    for t in ([1.0, 0.0], [0.0, 1.0]):
        assert np.abs(K @ np.tile(t, coord.shape[1])).max() <= 1e-9 * kmax          # translations in the kernel
    assert abs(F[0::2].sum()) <= 1e-9 * np.abs(F).sum() and abs(F[1::2].sum()) <= 1e-9 * np.abs(F).sum()
    K2, F2 = ctx.assemble(r['ds'], r['s'])
    assert np.array_equal(K2.data, K.data) and np.array_equal(F2, F)
    ctx.close()
    # a contiguous 1 % slab of the elements (14 cell rows) as a mesh of its own, whole against the oracle: the slab's point
    # data must be the full-size run's (same elements, same nodes' displacements), and its K / F the oracle's.  Rows of
    # nodes interior to the slab (every element of the node inside it) are rows of the full-size K as well.
    rows = 14
    e0, e1 = 700 * 2 * N, (700 + rows) * 2 * N                               # elements of cell rows 700 .. 713
    sub_nodes = np.unique(elem[:, e0:e1])
    sub_elem = np.searchsorted(sub_nodes, elem[:, e0:e1])
    sub_coord = np.ascontiguousarray(coord[:, sub_nodes])
    n_sub = (e1 - e0) * 7
    sub = fep.MeshContext(sub_elem, sub_coord)
    sub.set_materials(sh[0], bu[0], eta[0], c[0])
    rs = sub.step(U[:, sub_nodes], None, want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    sl = slice(e0 * 7, e1 * 7)
    assert np.array_equal(rs['ind_p'], r['ind_p'][sl])
    assert np.array_equal(rs['s'], r['s'][:, sl]) and np.array_equal(rs['ds'], r['ds'][:, sl])   # same kernel code on the same inputs
    d1t, d2t, wft = fep.element_tables('P2')
    one = np.ones(n_sub)
    Ko, Bo, wo, iDo, jDo, Do = orc.elastic_setup(sub_elem, sub_coord, sh[0] * one, bu[0] * one, d1t, d2t, wft)
    Eo, cpo, Kto, Fo = orc.hot_path(U[:, sub_nodes], np.zeros((4, n_sub)), dict(K_elast=Ko, B=Bo, D_elast=Do, weight=wo, iD=iDo,
                                                                                jD=jDo, shear=sh[0] * one, bulk=bu[0] * one,
                                                                                eta=eta[0] * one, c=c[0] * one))
    assert np.array_equal(rs['ind_p'], cpo['ind_p']) and min(cpo['n_smooth'], cpo['n_apex']) > 0.1 * n_sub
    # one decade on top of the usual bounds: at h = 10 / 2828 the strain B U is a sum of terms ~300 times its own size, and
    # the oracle's sparse product and the kernel sum them in different orders (measured 1.1e-13 on s); the return map on the
    # KERNEL's strain is checked to the usual 1e-13 on the sampled points above
    assert relerr(rs['E'], Eo) <= 1e-12
    assert relerr(rs['s'], cpo['s']) <= 10 * TOL_PT and relerr(rs['ds'], cpo['ds']) <= 10 * TOL_PT
    # every point against ITS OWN largest entry: with the oracle's map on the kernel's strain (a point of small stress sees the
    # strain's round-off magnified by max|s| / |s_point|, which is the conditioning of B U, not of the path under test)
    ok = orc.return_map(rs['E'], None, sh[0] * one, bu[0] * one, eta[0] * one, c[0] * one)
    assert np.array_equal(ok['ind_p'], rs['ind_p'])
    assert relerr_points(rs['s'], ok['s']) <= TOL_PT_EACH and relerr_points(rs['ds'], ok['ds']) <= TOL_PT_EACH
    assert np.abs((rs['K'] - Kto).data).max() <= TOL_K * np.abs(Kto.data).max() and relerr_rows(rs['K'], Kto) <= TOL_K_EACH
    assert relerr(rs['F'], np.asarray(Fo).ravel()) <= TOL_K
    # interior rows of the slab against the same rows of the full-size K (different patches, different partial sums)
    inner = np.ones(sub_nodes.size, dtype=bool)
    edge_nodes = np.unique(np.concatenate([elem[:, e0 - 2 * N:e0].ravel(), elem[:, e1:e1 + 2 * N].ravel()]))
    inner[np.searchsorted(sub_nodes, np.intersect1d(sub_nodes, edge_nodes))] = False
    loc = np.flatnonzero(inner)
    dofs_l = (2 * loc[:, None] + np.arange(2)[None, :]).ravel()
    dofs_g = (2 * sub_nodes[loc][:, None] + np.arange(2)[None, :]).ravel()
    Kl = rs['K'][dofs_l].tocoo()
    Kg = K[dofs_g].tocoo()
    sub_dofs = (2 * sub_nodes[:, None] + np.arange(2)[None, :]).ravel()
    assert np.array_equal(sub_dofs[Kl.col], Kg.col) and np.array_equal(Kl.row, Kg.row)      # same pattern, same order
    assert np.abs(Kl.data - Kg.data).max() <= 1e-13 * kmax
    assert np.abs(rs['F'][dofs_l] - F[dofs_g]).max() <= 1e-13 * np.abs(F).max()
    sub.close()


@pytest.mark.parametrize('t,N', [('P1', 24), ('P2', 8), ('Q1', 12), ('Q2', 6), ('P4', 4)])
def test_tangent_is_the_derivative_of_the_internal_force(fep, t, N):
    """End to end without any checker: K_tangent(U) v equals the central difference of F(U + h v) (the Newton
    linearisation DP:1050 / DP:1058 is consistent), on a state with all three branches."""
    rng = np.random.default_rng(8)
    elem, coord = square_mesh_of(t, N)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(*[v[0] for v in dp_materials(1)])
    x, y = coord
    U = np.array([2.0e-4 * y * (x / 10) + 1.0e-4 * x * (y > 5), -1.2e-4 * y * (x < 5) + 1.6e-4 * y * (x >= 5)])
    U = U.reshape(-1, order='F')
    Ep = rng.normal(0, 5e-6, size=(4, ctx.n_int))
    r = ctx.step(U, Ep, want=('K', 'F', 'ind_p'))
    assert r['n_smooth'] > 0 and r['n_apex'] > 0 and r['n_smooth'] + r['n_apex'] < ctx.n_int
    v = rng.normal(size=ctx.n_dof)
    h = 1e-9 * np.abs(U).max()
    Fp = ctx.step(U + h * v, Ep, want=('F', 'ind_p'))
    Fm = ctx.step(U - h * v, Ep, want=('F', 'ind_p'))
    same = np.array_equal(Fp['ind_p'], r['ind_p']) and np.array_equal(Fm['ind_p'], r['ind_p'])
    dF = (Fp['F'] - Fm['F']) / (2 * h)
    Kv = r['K'] @ v
    # points that change branch inside +-h contribute a kink; they are rare and bounded
    tol = 1e-6 if same else 1e-3
    assert np.abs(dF - Kv).max() <= tol * np.abs(Kv).max()
    ctx.close()


def test_gpu_ds_is_the_consistent_tangent_of_gpu_s(fep):
    """The kernel's `ds` against central differences of the kernel's own `s` (no oracle involved)."""
    rng = np.random.default_rng(3)
    n = 20000
    sh, bu, eta, c = dp_materials(n)
    e = rng.normal(0, 3e-4, size=(3, n))
    e[0:2] += rng.normal(1e-4, 2e-4, size=(1, n))
    ep = rng.normal(0, 2e-5, size=(4, n))
    cc = fep.plasticity2d_dp.construct_constitutive_problem
    r = cc(e, ep.copy(), sh, bu, eta, c)
    assert min((~r['ind_p']).sum(), r['n_smooth'], r['n_apex']) > 2000
    h = 1e-9
    fd = np.zeros((9, n))
    for j in range(3):
        de = np.zeros((3, n))
        de[j] = h
        sp, sm = cc(e + de, ep.copy(), sh, bu, eta, c)['s'], cc(e - de, ep.copy(), sh, bu, eta, c)['s']
        for i in range(3):
            fd[3 * i + j] = (sp[i] - sm[i]) / (2 * h)
    assert np.abs(fd - r['ds']).max() <= 1e-7 * np.abs(r['ds']).max()


# ---- special values and wide parameter ranges of the return map --------------------------------------
def test_return_map_special_values_vs_oracle(fep):
    """Zero strain, points exactly on the switching surfaces, pure volumetric / pure deviatoric strains,
    very small and very large magnitudes.  Branch decisions must be identical (strict > / <= as DP:693-699)."""
    sh0, bu0, eta0, c0 = [v[0] for v in dp_materials(1)]
    rows = []
    rows.append((0.0, 0.0, 0.0))                                    # zero strain: elastic, rho = 0
    rows.append((1e-300, -1e-300, 1e-300))                          # denormal-range products
    rows.append((5e-4, 5e-4, 0.0))                                  # pure volumetric tension: apex with rho = 0 (C6 corner)
    rows.append((-5e-4, -5e-4, 0.0))                                # pure volumetric compression: elastic
    rows.append((3e-4, -3e-4, 0.0))                                 # pure deviatoric
    rows.append((0.0, 0.0, 7e-4))                                   # pure shear
    for sc in (1e-12, 1e-9, 1e-6, 1e-3, 1e-1, 1e2):                 # magnitudes over 14 decades
        rows.append((1.3 * sc, -0.4 * sc, 0.9 * sc))
        rows.append((-1.1 * sc, -0.7 * sc, 0.2 * sc))
    E = np.array(rows).T.copy()
    n = E.shape[1]
    sh, bu, eta, c = sh0 * np.ones(n), bu0 * np.ones(n), eta0 * np.ones(n), c0 * np.ones(n)
    # a point tuned to sit on crit1 == 0 as closely as fp64 allows, and one on crit2 == 0
    from scipy.optimize import brentq

    def crit(g, which):
        r = orc.return_map(np.array([[0.0], [0.0], [g]]), None, sh[:1], bu[:1], eta[:1], c[:1])
        return (1.0 if r['ind_p'][0] else -1.0) if which == 1 else 0.0
    g1 = brentq(lambda g: crit(g, 1), 1e-6, 1e-2, xtol=1e-22, rtol=8.9e-16)
    E = np.concatenate([E, np.array([[0.0, 0.0], [0.0, 0.0], [g1, np.nextafter(g1, 1.0)]])], axis=1)
    n = E.shape[1]
    sh, bu, eta, c = sh0 * np.ones(n), bu0 * np.ones(n), eta0 * np.ones(n), c0 * np.ones(n)
    ep = np.zeros((4, n))
    with np.errstate(all='ignore'):
        o = orc.return_map(E, ep.copy(), sh, bu, eta, c, True)
    a = fep.construct_constitutive_problem(E, ep.copy(), sh, bu, eta, c, True)
    assert np.array_equal(a['ind_p'], o['ind_p'])
    fin = np.isfinite(o['s']).all(axis=0) & np.isfinite(o['ds']).all(axis=0)
    assert fin.sum() >= n - 1                                        # only the rho = 0 apex corner may be non-finite
    assert relerr(a['s'][:, fin], o['s'][:, fin]) <= TOL_PT and relerr(a['ds'][:, fin], o['ds'][:, fin]) <= TOL_PT
    assert np.array_equal(np.isnan(a['ds']), np.isnan(o['ds'])) and np.array_equal(np.isnan(a['s']), np.isnan(o['s']))
    assert relerr(a['ep'][:, fin], o['ep'][:, fin]) <= TOL_PT


def test_return_map_random_materials_wide_ranges(fep):
    rng = np.random.default_rng(2025)
    n = 50_000
    sh = 10 ** rng.uniform(2, 9, n)
    bu = sh * 10 ** rng.uniform(-1, 2, n)
    eta = rng.uniform(0.01, 0.9, n)
    c = 10 ** rng.uniform(-2, 5, n)
    scale = c / sh                                                   # strains around the yield strain of each point
    E = rng.normal(0, 1, size=(3, n)) * scale * 10 ** rng.uniform(-2, 1.5, n)
    ep = rng.normal(0, 0.1, size=(4, n)) * scale
    a = fep.construct_constitutive_problem(E, ep.copy(), sh, bu, eta, c, True)
    o = orc.return_map(E, ep.copy(), sh, bu, eta, c, True)
    assert 0.1 * n < o['n_smooth'] and 0.02 * n < o['n_apex'] < 20000
    assert np.array_equal(a['ind_p'], o['ind_p'])
    # per-point relative error (the arrays span 10 decades, so a global max norm would hide small points)
    for key in ('s', 'ds', 'ep'):
        ref = o[key]
        den = np.abs(ref).max(axis=0) + 1e-300
        assert (np.abs(a[key] - ref).max(axis=0) / den).max() <= 5e-12, key

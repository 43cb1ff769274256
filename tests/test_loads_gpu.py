"""
External loads on the GPU (fep_load_volume_*, fep_load_traction_*) and the Elasticity2D flavour end to end, against the
reference's own vectors (tests/golden/el_loads.npz, make_golden_el.py) and tests/loads_ref.py.

Bounds (u = 2^-53, loads_ref.bound):
  volume vector, per entry      |got - ref| <= 2 (m + 2) u * sum |terms|      m = (element, point) terms of the node: two
                                differently ordered float64 sums of the same two-rounding products;
  traction vector, per entry    |got - ref| <= 2 (m + 6) u * sum |terms|      m = edge points at the node; the four extra
                                roundings are the two squares, their sum and the root of the arc length (and, against the
                                closed form, the tabulated 1 / sqrt(3));
  totals                        derived in test_totals_*;
  driver                        U to 1e-10 of the field's maximum, energy to 1e-10 relative (tests/test_newton_gpu.py's).
Every test prints the worst ratio to its bound before it asserts.
"""
import decimal

import numpy as np
import pytest
import scipy.sparse as ssp

import loads_ref
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

CONST_V = np.array([[0.0], [-1.0]])
CONST_T = np.array([[0.0], [450.0]])


def _hatp(fep, t):
    return fep.get_local_basis_volume(t, fep.get_quadrature_volume(t)[0])[0]


def _volume_cases(fep):
    """(name, element type, elements 0-based, coordinates, weight, f_V_int, reference f_V) for every element type, a
    constant and a random field each."""
    g, md, tx = load_golden('el_loads'), load_golden('mesh_dp'), load_golden('tsx')
    out = []
    for t in ('P1', 'Q1', 'Q2'):
        tag = f'{t}_l1_'
        elem = g[tag + 'elements'] - 1
        n_int = g[tag + 'weight'].size
        out.append((t + ' const', t, elem, g[tag + 'coordinates'], g[tag + 'weight'], CONST_V * np.ones((1, n_int)), g[tag + 'f_V']))
        out.append((t + ' random', t, elem, g[tag + 'jig_coordinates'], g[tag + 'jig_weight'], g[tag + 'jig_f_V_int'],
                    g[tag + 'jig_f_V']))
    for t, tag, elem, coord in (('P2', 'P2sq_', md['P2_n4_elements'], md['P2_n4_coordinates']),
                                ('P4', 'P4tx_', tx['p4_elem'], tx['p4_coord'])):
        n_int = g[tag + 'weight'].size
        out.append((t + ' const', t, elem, coord, g[tag + 'weight'], CONST_V * np.ones((1, n_int)), g[tag + 'f_V_const']))
        out.append((t + ' random', t, elem, coord, g[tag + 'weight'], g[tag + 'f_V_int'], g[tag + 'f_V_rand']))
    return out


def _assert_within(name, got, ref, m, sabs, extra):
    lim = loads_ref.bound(m, sabs, extra)
    d = np.abs(np.asarray(got) - np.asarray(ref))
    worst = float((d / np.where(lim > 0, lim, 1.0)).max())
    print(f'{name}: worst |delta| / bound = {worst:.3f} over {d.size} entries')
    assert d.shape == lim.shape and np.all(d <= lim), (name, worst, np.argwhere(d > lim)[:5])


def test_volume_vector_every_element_type_per_entry(fep):
    for name, t, elem, coord, w, f, ref in _volume_cases(fep):
        ctx = fep.MeshContext(elem, coord)
        got = ctx.load_volume(f_v_int=f, hatp=_hatp(fep, t), weight=w)
        _, sabs, m = loads_ref.volume(elem, coord.shape[1], f, _hatp(fep, t), w)
        assert got.shape == ref.shape == (2, coord.shape[1])
        _assert_within(name, got, ref, m, sabs, 2)                  # every entry, none left out
        ctx.close()


def test_volume_uniform_equals_field_and_calls_are_bit_identical(fep):
    import torch
    for name, t, elem, coord, w, f, ref in _volume_cases(fep):
        if 'const' not in name:
            continue
        n_n = coord.shape[1]
        coord2 = np.concatenate((coord, [[-3.0], [-3.0]]), axis=1)              # one node that belongs to no element
        ctx = fep.MeshContext(elem, coord2)
        a = ctx.load_volume(f_v_int=f)                                          # default hatp, the context's own weight
        b = ctx.load_volume(f_v_int=f)
        c = ctx.load_volume(uniform=(0.0, -1.0))
        assert a.tobytes() == b.tobytes() == c.tobytes(), name
        assert np.all(a[:, n_n] == 0) and not np.isnan(a).any(), name           # 0, not the NaN of transform
        assert np.array_equal(a, ctx.load_volume(f_v_int=f, hatp=_hatp(fep, t)))
        r = ctx.load_volume(uniform=(0.37, -9.81))
        fr = np.array([[0.37], [-9.81]]) * np.ones((1, ctx.n_int))
        assert r.tobytes() == ctx.load_volume(f_v_int=fr).tobytes(), name
        # device form: direct, then captured in a graph and replayed
        dev = torch.device('cuda', 0)
        fd = torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
        out = torch.full((ctx.n_dof,), float('nan'), dtype=torch.float64, device=dev)
        out_u = torch.full((ctx.n_dof,), float('nan'), dtype=torch.float64, device=dev)

        def launch():
            st = torch.cuda.current_stream().cuda_stream
            ctx.load_volume_dev(st, out.data_ptr(), f_v_int=fd.data_ptr())
            ctx.load_volume_dev(st, out_u.data_ptr(), uniform=(0.37, -9.81))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            launch()
        torch.cuda.synchronize()
        want = np.ascontiguousarray(r.T).ravel()                                # interleaved (x, y) per node
        assert out.cpu().numpy().tobytes() == want.tobytes() == out_u.cpu().numpy().tobytes(), name
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            launch()
        out.fill_(float('nan'))
        out_u.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes() == out_u.cpu().numpy().tobytes(), name
        del gr
        ctx.close()


def test_load_entry_points_validate(fep):
    g = load_golden('el_loads')
    ctx = fep.MeshContext(g['P1_l1_elements'] - 1, g['P1_l1_coordinates'])
    l = fep.lib()
    h = np.ones((3, 1))
    out = np.zeros(ctx.n_dof)
    p = lambda a: a.ctypes.data                                                 # noqa: E731
    assert l.fep_load_volume_host(None, p(h), None, 0.0, 0.0, None, p(out)) == -1
    assert l.fep_load_volume_host(ctx.handle, None, None, 0.0, 0.0, None, p(out)) == -1
    assert l.fep_load_volume_host(ctx.handle, p(h), None, 0.0, 0.0, None, None) == -1
    assert l.fep_load_volume_dev(ctx.handle, None, p(h), None, 0.0, 0.0, None, None) == -1
    with pytest.raises(ValueError):
        ctx.load_volume()
    with pytest.raises(ValueError):
        ctx.load_volume(f_v_int=np.zeros((2, ctx.n_int)), uniform=(0, 1))
    ctx.close()
    # traction: sizes and ids
    ed = np.array([[0], [1]], dtype=np.int32)
    xy = np.array([[0.0, 1.0], [0.0, 0.0]])
    hs, dh, wf = fep.surface_tables('P1')
    t = np.ones((2, 1))
    out4 = np.zeros(4)
    bad_hi, bad_lo = np.array([[0], [2]], dtype=np.int32), np.array([[-1], [1]], dtype=np.int32)

    def args(n_n, n_e, e):
        return (0, n_n, n_e, 2, 1, p(e), p(xy), p(hs), p(dh), p(wf), p(t), p(out4))
    assert l.fep_load_traction_host(*args(2, 1, ed)) == 0
    assert out4.tolist() == [0.5, 0.5, 0.5, 0.5]                                # t L / 2, L = 1
    assert l.fep_load_traction_host(*args(-1, 1, ed)) == -1
    assert l.fep_load_traction_host(*args(2, -1, ed)) == -1
    assert l.fep_load_traction_host(0, 2, 1, 2, 1, None, p(xy), p(hs), p(dh), p(wf), p(t), p(out4)) == -1
    assert l.fep_load_traction_host(*args(2, 1, bad_hi)) == -5
    assert l.fep_load_traction_host(*args(2, 1, bad_lo)) == -5
    with pytest.raises(fep.FepError):
        fep.load_traction(np.array([[0], [7]]), xy, t, hs, dh, wf)


def _traction_golden_cases(fep):
    g = load_golden('el_loads')
    out = []
    for t in ('P1', 'Q1', 'Q2'):
        n_pts = g[f'{t}_l1_ft_int_var'].shape[1]
        out.append((t, t, g[f'{t}_l1_neumann_nodes'], g[f'{t}_l1_coordinates'], CONST_T * np.ones((1, n_pts)), g[f'{t}_l1_f_t'],
                    g[f'{t}_l1_ft_int_var'], g[f'{t}_l1_f_t_var']))
    out.append(('P2 square', 'P2', g['P2sq_edges'], load_golden('mesh_dp')['P2_n4_coordinates'], CONST_T * np.ones((1, 8)),
                g['P2sq_f_t_const'], g['P2sq_ft_int_var'], g['P2sq_f_t_var']))
    return out


def test_traction_vector_vs_reference_and_last_point_quirk(fep):
    for name, t, edges, coord, tc, ref_c, tv, ref_v in _traction_golden_cases(fep):
        xi_s, wf_s = fep.get_quadrature_surface(t)
        hatp_s, dhatp1_s = fep.get_local_basis_surface(t, xi_s)
        h, dh, wf = fep.surface_tables(t)
        got = fep.load_traction(edges.astype(np.int64), coord, tc, h, dh, wf)
        _, sabs, m = loads_ref.traction(edges, coord, tc, h, dh, wf)
        _assert_within(name + ' const', got, ref_c, m, sabs, 6)
        assert np.all(got[:, m == 0] == 0)
        assert got.tobytes() == fep.load_traction(edges.astype(np.int64), coord, tc, h, dh, wf).tobytes()
        # the reference's signature and quirk: the last point's value everywhere (EL:352-353)
        w = fep.elasticity2d.get_vector_traction(edges, coord, tv, hatp_s, dhatp1_s, wf_s)
        assert isinstance(w, ssp.csc_matrix) and w.shape == (2, coord.shape[1])
        last = np.repeat(tv[:, -1:], tv.shape[1], axis=1)
        _, sabs, m = loads_ref.traction(edges, coord, last, h, dh, wf)
        _assert_within(name + ' last-point quirk', w.toarray(), ref_v, m, sabs, 6)
        assert w.nnz == 2 * int((m > 0).sum())
        # the library itself honours a value per point: a non-constant field differs from the quirk
        per_point = fep.load_traction(edges.astype(np.int64), coord, tv, h, dh, wf)
        _, sabs_v, m_v = loads_ref.traction(edges, coord, tv, h, dh, wf)
        _assert_within(name + ' per point', per_point, loads_ref.traction(edges, coord, tv, h, dh, wf)[0], m_v, sabs_v, 6)
        assert np.abs(per_point - ref_v).max() > 1.0


def _exact_length(p, q):
    """sqrt(|q - p|^2) of two float points, rounded once from 60 digits."""
    with decimal.localcontext() as c:
        c.prec = 60
        dx, dy = decimal.Decimal(float(q[0])) - decimal.Decimal(float(p[0])), decimal.Decimal(float(q[1])) - decimal.Decimal(float(p[1]))
        return (dx * dx + dy * dy).sqrt()


@pytest.mark.parametrize('direction', ['vertical', '30 degrees'])
@pytest.mark.parametrize('n_p_s', [2, 3])
def test_traction_on_sloping_strips_vs_closed_form(fep, direction, n_p_s):
    """Ground the reference does not cover (its Jacobian is |dx/dxi|): a uniform traction on a straight strip of 6 edges.
    Two-node edges: t L / 2 per end node; three-node edges with the middle node at the midpoint: t L / 6, t L / 6, 4 t L / 6.
    All coordinates are multiples of 2^-9 (exact in binary, exact midpoints); each edge length is taken from the float end
    points with 60 digits, so the closed form carries one rounding per edge and node.
    The cancellation inside j_c = sum_a x_a dhat_a of a three-node edge (the reference's formula, kept so that its horizontal
    edges are reproduced to the bits of its own Jacobian) is not in this bound: its absolute error grows with the distance of
    the edge from the origin, up to (n_p_s + 1) u sum_a |x_a dhat_a|.  tests/loads_exact.py, traction_bound, carries that term
    and tests/test_loads_shapes_gpu.py applies it to curved and high-order edges anywhere.  The strips here are centred at the
    origin, |x| <= 3 edge lengths; for two-node edges on this lattice j_c is exact anywhere."""
    step = {'vertical': (0.0, 0.5), '30 degrees': (round(np.sqrt(3) / 4 * 256) / 256, 0.25)}[direction]
    n_e = 6
    k = np.arange(2 * n_e + 1) - n_e
    coord = np.array([k * step[0] / 2, k * step[1] / 2])                     # lattice of end and middle nodes
    coord = np.concatenate((coord, [[9.0, -1.0], [9.0, 3.0]]), axis=1)       # two unloaded nodes
    e = np.arange(n_e)
    edges = np.array([2 * e, 2 * e + 2]) if n_p_s == 2 else np.array([2 * e, 2 * e + 2, 2 * e + 1])
    t = 'P1' if n_p_s == 2 else 'Q2'
    h, dh, wf = fep.surface_tables(t)
    trac = (-3.0, 7.5)
    t_int = np.array([[trac[0]], [trac[1]]]) * np.ones((1, n_e * wf.size))
    got = fep.load_traction(edges, coord, t_int, h, dh, wf)
    _, sabs, m = loads_ref.traction(edges, coord, t_int, h, dh, wf)
    want = np.zeros((2, coord.shape[1]), dtype=object) + decimal.Decimal(0)
    with decimal.localcontext() as c:
        c.prec = 60
        for j in range(n_e):
            L = _exact_length(coord[:, edges[0, j]], coord[:, edges[1, j]])
            shares = (L / 2, L / 2) if n_p_s == 2 else (L / 6, L / 6, 4 * L / 6)
            for a, sh in enumerate(shares):
                for comp in range(2):
                    want[comp, edges[a, j]] += decimal.Decimal(trac[comp]) * sh
    want = np.array([[float(v) for v in row] for row in want])
    if direction == '30 degrees':
        ang = np.degrees(np.arctan2(step[1], step[0]))
        assert abs(ang - 30) < 0.1
    _assert_within(f'{direction}, {n_p_s}-node edges', got, want, m, sabs, 6)
    assert np.all(got[:, -2:] == 0)


def test_totals_of_the_demo_loads(fep):
    """sum f_V = force * area = -75, sum f_t = traction * length = 4500 on the demo meshes, with bounds from the roundings
    that enter (n = entries summed, L / h = size over lattice step):
      * every entry of f against its exact value: (m + 2) u sum|terms| (volume), (m + 6) u sum|terms| (traction);
      * the float64 sum of n entries formed here: n u sum |f|;
      * the exact sum of all terms is force * sum_k w_k * sum_a hatp[a, q]: the tabulated partition of unity is 1 to
        (n_p + 2) u; the weights |det J| wf come from Jacobian entries sum_a x_a dhat_a, n_p products of coordinates up to L
        that cancel down to ~ h / 2, i.e. relative error up to 2 (n_p + 2) u L / h each, two entries per product and two
        products in the determinant: 8 (n_p + 2) u (L / h) on the area; the same with n_p_s on the length."""
    u = loads_ref.U
    for t in ('P1', 'Q1', 'Q2'):
        mesh = fep.assemble_mesh_el(1, t, 10, 5)
        elem, coord = mesh['elements'] - 1, mesh['coordinates']
        ctx = fep.MeshContext(elem, coord)
        n_p = ctx.n_p
        h_lat = 10 / (np.unique(coord[0]).size - 1)
        f = ctx.load_volume(uniform=(0.0, -1.0))
        w = ctx.geometry()[2].ravel()
        _, sabs, m = loads_ref.volume(elem, ctx.n_n, CONST_V * np.ones((1, ctx.n_int)), _hatp(fep, t), w)
        lim = u * (((m + 2) * sabs[1]).sum() + ctx.n_n * np.abs(f[1]).sum()) + (n_p + 2) * u * 75 + 8 * (n_p + 2) * u * (10 / h_lat) * 75
        print(f'{t}: sum f_V + 75 = {f[1].sum() + 75:.3e}, bound {lim:.3e}')
        assert abs(f[1].sum() + 75) <= lim and np.all(f[0] == 0)
        hs, dh, wf = fep.surface_tables(t)
        edges = mesh['neumann_nodes'].astype(np.int64)
        t_int = CONST_T * np.ones((1, edges.shape[1] * wf.size))
        ft = fep.load_traction(edges, coord, t_int, hs, dh, wf)
        _, sabs, m = loads_ref.traction(edges, coord, t_int, hs, dh, wf)
        n_b = int((m > 0).sum())
        n_p_s = edges.shape[0]
        lim = u * (((m + 6) * sabs[1]).sum() + n_b * np.abs(ft[1]).sum()) + (n_p_s + 2) * u * 4500 + 8 * (n_p_s + 2) * u * (10 / h_lat) * 4500
        print(f'{t}: sum f_t - 4500 = {ft[1].sum() - 4500:.3e}, bound {lim:.3e}')
        assert abs(ft[1].sum() - 4500) <= lim and np.all(ft[0] == 0)
        ctx.close()


@pytest.mark.parametrize('solver', ['direct', 'pcg', 'amg'])
@pytest.mark.parametrize('t', ['P1', 'Q1', 'Q2'])
def test_solve_elasticity2d_level1_vs_reference(fep, t, solver):
    g = load_golden('el_loads')
    r = fep.solve_elasticity2d(t, level=1, linear_solver=solver)
    eu, ee = relerr(r['U'], g[f'{t}_l1_u']), abs(r['energy'] - float(g[f'{t}_l1_energy'])) / abs(float(g[f'{t}_l1_energy']))
    print(f'{t} {solver}: U {eu:.2e}, energy {ee:.2e} ({r["energy"]!r}), iterations {r["iterations"]}')
    assert r['U'].shape == g[f'{t}_l1_u'].shape and eu <= 1e-10
    assert ee <= 1e-10
    assert relerr(r['f_V'], g[f'{t}_l1_f_V']) <= 1e-13 and relerr(r['f_t'], g[f'{t}_l1_f_t']) <= 1e-13
    assert r['K'].shape == (r['U'].size, r['U'].size)
    assert (r['iterations'] is None) == (solver == 'direct')


def test_elasticity_fem_p1_level3_is_baseline_config_0(fep, capsys):
    g = load_golden('el_loads')
    r = fep.elasticity2d.elasticity_fem(fep.LagrangeElementType.P1, 3, False)
    printed = capsys.readouterr().out.strip().splitlines()[-1]
    assert printed.startswith('Stored energy: ')
    e_ref = 2694.589229927946                                                   # the reference's own printout
    assert float(g['P1_l3_energy']) == e_ref
    print(f'energy {r["energy"]!r}, iterations {r["iterations"]}')
    assert abs(float(printed.split(':')[1]) - e_ref) <= 1e-10 * e_ref
    assert relerr(r['U'], g['P1_l3_u']) <= 1e-10


def test_get_vector_volume_called_as_the_reference_driver_calls_it(fep):
    """EL:1094-1127 line by line with the library's names: the mesh's 1-based elements are shifted by the K routine and
    get_vector_volume finds the context of that call through the identity of `weight`."""
    el = fep.elasticity2d
    g = load_golden('el_loads')
    for t in ('P1', 'Q1', 'Q2'):
        element_type = el.LagrangeElementType[t]
        mesh = el.assemble_mesh(1, element_type, 10, 5)
        xi, wf = el.get_quadrature_volume(element_type)
        hatp, dhatp1, dhatp2 = el.get_local_basis_volume(element_type, xi)
        n_int = mesh['elements'].shape[1] * wf.size
        shear = 206900 / (2 * (1 + 0.29)) * np.ones(n_int)
        bulk = 206900 / (3 * (1 - 2 * 0.29)) * np.ones(n_int)
        K, weight = el.get_elastic_stiffness_matrix(mesh['elements'], mesh['coordinates'], shear, bulk, dhatp1, dhatp2, wf)
        assert type(weight) is np.ndarray and weight.shape == (1, n_int) and mesh['elements'].min() == 0
        f_V_int = np.dot(np.array([[0, -1]]).transpose(), np.ones((1, n_int)))
        f_V = el.get_vector_volume(mesh['elements'], mesh['coordinates'], f_V_int, hatp, weight)
        n_n = mesh['coordinates'].shape[1]
        assert isinstance(f_V, ssp.csc_matrix) and f_V.shape == (2, n_n) and f_V.nnz == 2 * n_n
        assert f_V.reshape((-1, 1), order='F').shape == (2 * n_n, 1)
        hot = importlib_hotpath(fep)
        assert hot._context_for(mesh['elements'], n_n, weight) is K.fep_ctx      # found, not rebuilt
        ref, sabs, m = loads_ref.volume(mesh['elements'], n_n, f_V_int, hatp, weight)
        _assert_within(t + ' driver call', f_V.toarray(), ref, m, sabs, 2)
        assert relerr(f_V.toarray(), g[f'{t}_l1_f_V']) <= 1e-13
        # a copy of the weights is unknown to the registry: a context is built from elements / coordinates; same bits
        w2 = weight.copy()
        assert hot._context_for(mesh['elements'], n_n, w2) is None
        f2 = el.get_vector_volume(mesh['elements'], mesh['coordinates'], f_V_int, hatp, w2)
        assert f2.toarray().tobytes() == f_V.toarray().tobytes()
        # the caller's weights are honoured, as the reference honours them
        f3 = el.get_vector_volume(mesh['elements'], mesh['coordinates'], f_V_int, hatp, 2 * weight)
        assert np.array_equal(f3.toarray(), 2 * f_V.toarray())
        weight *= 2                                                              # in place: same object, new values
        f4 = el.get_vector_volume(mesh['elements'], mesh['coordinates'], f_V_int, hatp, weight)
        assert np.array_equal(f4.toarray(), f3.toarray())


def importlib_hotpath(fep):
    import importlib
    return importlib.import_module(fep.__name__ + '.hotpath')

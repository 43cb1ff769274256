"""
The high-precision load reference (tests/loads_exact.py) on the host, before a GPU is involved: its edge tables against the
library's, the float64 restatement tests/loads_ref.py inside the new bounds on every case of tests/load_cases.py (so inputs
and bounds are satisfiable), the recorded reason for the new traction bound (the old one fails on the curved P4 wall), the
pressure-total bound on the restatement, and the exact reference against the sloping-strip closed forms.
Every test prints the worst ratio to its bound before it asserts.
"""
import decimal

import numpy as np
import pytest

import load_cases as lc
import loads_exact as lx
import loads_ref

U = lx.U


def test_edge_tables_reproduce_the_library_p2_tables(fep):
    """The convention (row a = node a of (-1, +1, 0), row 0 is 1 at xi = -1; leggauss' two points are -+ 1 / sqrt 3, weights 1)
    pinned to fep.surface_tables('P2'), whose entries carry the roundings of x (x - 1) / 2 etc.: 2 u per entry."""
    h, dh, wf = lx.edge_tables((-1, 1, 0), 2)
    H, DH, WF = fep.surface_tables('P2')
    print('worst table differences in u:', np.abs(h - H).max() / U, np.abs(dh - DH).max() / U, np.abs(wf - WF).max() / U)
    assert h.shape == H.shape and dh.shape == DH.shape and wf.shape == WF.shape
    assert np.all(np.abs(h - H) <= 2 * U) and np.all(np.abs(dh - DH) <= 2 * U) and np.all(np.abs(wf - WF) <= 2 * U)
    hl, dl, wl = lx.edge_tables((-1, 1), 1)
    HL, DL, WL = fep.surface_tables('P1')
    assert np.array_equal(hl, HL) and np.array_equal(dl, DL) and np.array_equal(wl, WL)


@pytest.mark.parametrize('n_p_s,n_q', [(2, 1), (2, 8), (3, 2), (3, 5), (4, 5), (5, 2), (5, 5), (5, 8)])
def test_edge_tables_are_a_lagrange_basis(n_p_s, n_q):
    """Kronecker property at the nodes (exact: rational arithmetic), partition of unity and zero derivative sum at the Gauss
    points to the rounding of the entries (u sum_a |entry|), weights summing to 2."""
    from fractions import Fraction
    nodes = [Fraction(v) for v in lc.NODES[n_p_s]]
    for i, x in enumerate(nodes):
        v, _ = lx._lagrange(nodes, x)
        assert v == [int(j == i) for j in range(n_p_s)]
    h, dh, wf = lx.edge_tables(lc.NODES[n_p_s], n_q)
    assert h.shape == dh.shape == (n_p_s, n_q) and wf.shape == (n_q,)
    assert np.all(np.abs(h.sum(axis=0) - 1) <= (n_p_s + 1) * U * np.abs(h).sum(axis=0))
    assert np.all(np.abs(dh.sum(axis=0)) <= (n_p_s + 1) * U * np.abs(dh).sum(axis=0))
    assert np.abs(h).sum(axis=0).max() <= n_p_s + 2                         # what pressure_total_bound leans on
    assert abs(wf.sum() - 2) <= 2 * n_q * U
    assert lx.gauss_defect(lc.NODES[n_p_s], dh, wf).max() <= 8 * n_q * U * np.abs(dh).max()


@pytest.mark.parametrize('name', lc.TRACTION_NAMES)
def test_restatement_within_traction_bound_of_exact(fep, name):
    case = lc.traction_case(fep, name)
    f, lim, m = lc.exact(case)
    ref, sabs, m_ref = loads_ref.traction(*case.args())
    assert np.array_equal(m, m_ref) and f.shape == (2, case.n_n)
    assert np.all(f[:, m == 0] == 0) and np.all(lim[:, m == 0] == 0) and np.all(lim[:, m > 0] >= 0)
    lc.within(name + ' loads_ref.traction', ref, f, lim)
    if case.pressure is not None and case.closed:
        b = lc.pressure_total_bound(case, ref)
        tot = np.abs(ref.sum(axis=1))
        print(f'{name}: |sum f| = {tot}, bound {b}, sum |f| = {np.abs(ref).sum(axis=1)}')
        assert np.all(tot <= b)
        assert np.all(b <= 1e-11 * np.abs(ref).sum(axis=1))                 # and the bound says something
    if case.sorted_edges is not None:
        srt, _, _ = loads_ref.traction(case.sorted_edges, case.coord, case.sorted_t, case.h, case.dh, case.wf)
        assert np.all(np.abs(srt - ref) <= 2 * lim)


def test_old_bound_fails_on_the_curved_p4_wall(fep):
    """The recorded reason for traction_bound: on the tunnel wall projected onto TSX_HOLE, refined twice, as P4 edges, the
    float64 restatement loads_ref.traction misses the exact vector by more than loads_ref.bound(m, sabs, 6), the bound of
    tests/test_loads_gpu.py, which has no term for the cancellation inside j_c.  Measured worst |delta| / old bound
    (random traction / pressure): 2-point 5.9 / 5.4, 5-point 9.0 / 6.2, 8-point 2.5 / 2.1; against traction_bound the same
    vectors sit at 0.035 to 0.072."""
    for n_q, low in ((2, 4.0), (5, 4.0), (8, 1.5)):
        for kind in ('random', 'pressure'):
            case = lc.traction_case(fep, f'tunnel wall level 2 P4, {n_q}-point, {kind}, shuffled')
            f, lim, m = lc.exact(case)
            ref, sabs, m_ref = loads_ref.traction(*case.args())
            old = loads_ref.bound(m_ref, sabs, 6)
            d = np.abs(ref - f)
            r_old = float((d / np.where(old > 0, old, 1.0)).max())
            r_new = float((d / np.where(lim > 0, lim, 1.0)).max())
            print(f'{case.name}: worst |delta| / old bound = {r_old:.2f}, / traction_bound = {r_new:.3f}')
            assert r_old > low and r_new <= 1


@pytest.mark.parametrize('name', lc.VOLUME_NAMES)
def test_restatement_within_volume_bound_of_exact(fep, name):
    t, elem, coord, f_rand = lc.volume_mesh(fep, name)
    n_n = coord.shape[1]
    w = lc.host_weight(fep, t, elem, coord)
    assert w.min() > 0
    h = lc.hatp(fep, t)
    for kind, f in (('random', f_rand), ('uniform', lc.uniform_field(w.size))):
        ex, lim, m = lc.exact_volume(elem, n_n, f, h, w)
        ref, sabs, m_ref = loads_ref.volume(elem, n_n, f, h, w)
        assert np.array_equal(m, m_ref) and m.min() > 0
        lc.within(f'{name} {kind} loads_ref.volume (largest m = {m.max()})', ref, ex, lim)
    if name == 'fan 255 P1':
        assert m.max() == 255


# ---- the exact reference against closed forms ------------------------------------------------------------------------------
def _strip(direction, n_p_s):
    """The strips of test_loads_gpu.test_traction_on_sloping_strips_vs_closed_form, same numbers."""
    step = {'vertical': (0.0, 0.5), '30 degrees': (round(np.sqrt(3) / 4 * 256) / 256, 0.25)}[direction]
    n_e = 6
    k = np.arange(2 * n_e + 1) - n_e
    coord = np.array([k * step[0] / 2, k * step[1] / 2])
    coord = np.concatenate((coord, [[9.0, -1.0], [9.0, 3.0]]), axis=1)
    e = np.arange(n_e)
    edges = np.array([2 * e, 2 * e + 2]) if n_p_s == 2 else np.array([2 * e, 2 * e + 2, 2 * e + 1])
    return edges, coord


@pytest.mark.parametrize('direction', ['vertical', '30 degrees'])
@pytest.mark.parametrize('n_p_s', [2, 3])
def test_traction_exact_vs_sloping_strip_closed_form(fep, direction, n_p_s):
    """Uniform traction on a straight strip of 6 edges: t L / 2 per end node of a two-node edge; t L (1/6, 1/6, 4/6) on a
    three-node edge with its middle node at the midpoint.  L from the float end points at 60 digits.
    Two-node edges (midpoint rule, entries 1/2, -1/2, 1/2, weight 2: exact in binary): the formula IS the closed form, so
    traction_exact equals it to the one rounding of each side, 2 u |value|.
    Three-node edges: the closed form holds for the exact 2-point Gauss rule; the library's float64 tables are inputs that
    differ from it entry by entry.  With dh, ddh the differences of fep.surface_tables('Q2') from the tables at
    +- 1 / sqrt 3 evaluated with 60 digits, the formula moves to first order by at most
        sum over the terms of  |wf t| [ |dh| J + |h| (B_1 + B_2) ],     B_c = sum_a |x_{c,a} ddh_a|
    (|J(j + dj) - J(j)| <= |dj_1| + |dj_2|), plus one rounding on each side; the second order is covered by a factor 1 + 1e-9."""
    edges, coord = _strip(direction, n_p_s)
    n_e = edges.shape[1]
    h, dh, wf = fep.surface_tables('P1' if n_p_s == 2 else 'Q2')
    trac = (-3.0, 7.5)
    t_int = np.array([[trac[0]], [trac[1]]]) * np.ones((1, n_e * wf.size))
    got = lx.traction_exact(edges, coord, t_int, h, dh, wf)
    want = np.zeros((2, coord.shape[1]), dtype=object) + decimal.Decimal(0)
    with decimal.localcontext() as c:
        c.prec = 60
        D = decimal.Decimal
        for j in range(n_e):
            p, q = coord[:, edges[0, j]], coord[:, edges[1, j]]
            dx, dy = D(float(q[0])) - D(float(p[0])), D(float(q[1])) - D(float(p[1]))
            L = (dx * dx + dy * dy).sqrt()
            shares = (L / 2, L / 2) if n_p_s == 2 else (L / 6, L / 6, 4 * L / 6)
            for a, sh in enumerate(shares):
                for comp in range(2):
                    want[comp, edges[a, j]] += D(trac[comp]) * sh
        if n_p_s == 3:                                                      # the tables at the exact Gauss points
            g = 1 / D(3).sqrt()
            xs = (-g, g)
            h_x = [[x * (x - 1) / 2 for x in xs], [x * (x + 1) / 2 for x in xs], [(x + 1) * (1 - x) for x in xs]]
            d_x = [[x - D('0.5') for x in xs], [x + D('0.5') for x in xs], [-2 * x for x in xs]]
            e_h = np.array([[float(abs(D(float(h[a, q])) - h_x[a][q])) for q in range(2)] for a in range(3)])
            e_d = np.array([[float(abs(D(float(dh[a, q])) - d_x[a][q])) for q in range(2)] for a in range(3)])
    want = np.array([[float(v) for v in row] for row in want])
    lim = U * (np.abs(want) + np.abs(got))
    if n_p_s == 3:
        assert e_h.max() <= 4 * U and e_d.max() <= 4 * U                     # the tables are as good as their arithmetic
        J, _ = lx.jacobian_sizes(edges, coord, dh, wf)
        nodes = np.repeat(edges[:, :, None], 2, axis=2).ravel()
        B = sum(np.abs(coord[c][edges][:, :, None] * e_d[:, None, :]).sum(axis=0) for c in range(2))     # (n_e, n_q)
        for comp in range(2):
            wt = np.abs(wf[None, :] * t_int[comp].reshape(n_e, 2))
            terms = e_h[:, None, :] * (wt * J)[None] + np.abs(h)[:, None, :] * (wt * B)[None]
            lim[comp] += (1 + 1e-9) * np.bincount(nodes, weights=terms.ravel(), minlength=coord.shape[1])
    lc.within(f'traction_exact on the {direction} strip, {n_p_s}-node edges', got, want, lim)
    assert np.all(got[:, -2:] == 0) and np.abs(got).max() > 1

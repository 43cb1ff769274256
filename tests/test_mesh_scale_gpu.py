"""
The mesh kernels (fep_mesh_*: numbering, enrichment, uniform and marked refinement, corner codes) and the state transfer
behind them at the sizes where their prefix sums change shape: one scan tile | two at 1024 entries, two scan levels | three
at 1024^2 (scale_cases.py).  The small strips are held to the NumPy twin bit for bit AND to the twin-free checkers of
scale_cases.py; the million-element strips and the jittered square, where the twin takes minutes, to the checkers and the
closed forms alone.  On the integer strips every check is an exact equality.
"""
import functools

import numpy as np
import pytest

import scale_cases as sc

pytestmark = pytest.mark.gpu

DEV = 0
ERANGE, ESTATE = -5, -6                                       # include/fep.h
LARGEST = sc.LARGE_SIZES[-1]


@functools.lru_cache(maxsize=1)
def _strip(n):
    """(coord, elem, edge table) of strip(n); one mesh is kept, so tests of the same size that follow each other share it."""
    coord, elem = sc.strip(n)
    return coord, elem, sc.edge_table(elem)


@functools.lru_cache(maxsize=1)
def _square():
    coord, elem = sc.jittered_square()
    assert elem.shape[1] == 1051250
    return coord, elem, sc.edge_table(elem)


def _same(a, b, what=''):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.shape(a[k]) == np.shape(b[k]) and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _same_bytes(dev, host, what):
    """A device-resident output (int32 / uint8 / float64 tensor) against the host form's array (which widens the integers)."""
    d = dev.cpu().numpy()
    assert d.shape == host.shape and np.array_equal(d, host) and host.astype(d.dtype).tobytes() == d.tobytes(), what


def _strip_info(n):
    n_n, n_e, n_edges, n_bnd = sc.strip_counts(n)
    return dict(n_e=n_e, n_n=n_n, n_edges=n_edges, n_boundary_edges=n_bnd, n_nonmanifold=0, n_inconsistent=0, n_degenerate=0)


def _marked_round(fep, m, coord, elem, t, marked, exact, sweeps=None):
    """mark + refine_marked + child_corners of the DeviceMesh m, checked; -> (mark's counts, (coord, elem, parent), corners)."""
    got = m.mark(marked)
    c, e, p = m.refine_marked()
    corners = m.child_corners()
    assert (e.shape[1], c.shape[1] - coord.shape[1]) == (got['n_child'], got['n_new_nodes'])
    split = sc.check_children(coord, elem, c, e, p, corners, exact=exact, t=t)
    state = sc.check_marks(coord, elem, marked, split, p, corners, t=t)
    assert sc.closure_counts(state, t) == (got['n_child'], got['n_new_nodes']), got
    assert got['n_marked_elements'] == int(state.any(axis=0).sum())
    if sweeps is not None:
        assert 0 < got['n_sweeps'] <= sweeps, got
    return got, (c, e, p), corners


# ---- a. one scan tile | two ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sc.SMALL_SIZES)
def test_tile_edge_small(fep, n):
    coord, elem, t = _strip(n)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        assert m.info == _strip_info(n)
        sc.check_info(m.info, elem)
        p2, p4 = m.enrich('P2'), m.enrich('P4')
        cu, eu = m.refine()
        sc.check_p2(p2, coord, elem, t=t)
        sc.check_p4(p4, coord, elem, t=t)
        assert sc.check_children(coord, elem, cu, eu, *sc.uniform_codes(n), exact=True, t=t).all()
        _same(p2, fep.create_midpoints_P2(coord, elem), 'P2')
        _same(p4, fep.create_midpoints_P4(coord, elem), 'P4')
        for d, h in zip((cu, eu), fep.refine_uniform(coord, elem)):
            assert d.shape == h.shape and d.dtype == h.dtype and d.tobytes() == h.tobytes()
        for kind in ('none', 'all', 'random'):
            marked = sc.marking(kind, n)
            got, dev, corners = _marked_round(fep, m, coord, elem, t, marked, True, sweeps=sc.max_sweeps())
            for d, h in zip(dev, fep.refine_marked(coord, elem, marked)):
                assert d.shape == h.shape and d.dtype == h.dtype and d.tobytes() == h.tobytes(), kind
            hc = fep.child_corners(coord, elem, marked)
            assert corners.shape == hc.shape and corners.dtype == hc.dtype and corners.tobytes() == hc.tobytes(), kind
            if kind == 'all':
                assert dev[0].tobytes() == cu.tobytes()


# ---- b. two scan levels | three -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sc.LARGE_SIZES)
def test_tile_edge_large_p2_and_refine(fep, n):
    coord, elem, t = _strip(n)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        assert m.info == _strip_info(n)
        p2 = m.enrich('P2')
        cu, eu = m.refine()
        if n == LARGEST:
            for d, key in zip(m.enrich_dev('P2'), ('elem_ext', 'coord_ext', 'surf', 'elem_ed', 'edge_el')):
                _same_bytes(d, p2[key], key)
            for d, h in zip(m.refine_dev(), (cu, eu)):
                _same_bytes(d, h, 'refine_dev')
    sc.check_p2(p2, coord, elem, t=t)
    assert sc.check_children(coord, elem, cu, eu, *sc.uniform_codes(n), exact=True, t=t).all()


@pytest.mark.parametrize('n', sc.LARGE_SIZES)
def test_tile_edge_large_p4(fep, n):
    coord, elem, t = _strip(n)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        p4 = m.enrich('P4')
        if n == LARGEST:
            for d, key in zip(m.enrich_dev('P4'), ('elem_ext', 'coord_ext', 'surf')):
                _same_bytes(d, p4[key], key)
    sc.check_p4(p4, coord, elem, t=t)


@pytest.mark.parametrize('n,kind', [(n, kind) for n in sc.LARGE_SIZES for kind in ('all', 'random', 'first', 'last')])
def test_tile_edge_large_marked(fep, n, kind):
    coord, elem, t = _strip(n)
    marked = sc.marking(kind, n)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        # the strip's closure ends after two propagation steps: more sweeps than that allows, and the geometry is not the strip's
        got, dev, corners = _marked_round(fep, m, coord, elem, t, marked, True, sweeps=sc.max_sweeps())
        if n == LARGEST:
            for d, h in zip(m.refine_marked_dev(), dev):
                _same_bytes(d, h, 'refine_marked_dev')
            _same_bytes(m.child_corners_dev(), corners, 'child_corners_dev')
    if kind == 'all':
        assert (got['n_child'], got['n_new_nodes'], got['n_marked_elements']) == (4 * n, 2 * n + 1, n)
    if kind in ('first', 'last'):                                # the marked triangle, its neighbours, their cell partners
        assert got['n_marked_elements'] <= 4 and got['n_new_nodes'] <= 5


# ---- c. degree-6 nodes, no exact arithmetic -------------------------------------------------------------------------------------
def test_jittered_square_numbering(fep):
    coord, elem, t = _square()
    with fep.DeviceMesh(coord, elem, DEV) as m:
        sc.check_info(m.info, elem)
        N = sc.JITTER_N
        assert (m.info['n_edges'], m.info['n_boundary_edges']) == (3 * N * N + 2 * N, 4 * N)
        p2 = m.enrich('P2')
        cu, eu = m.refine()
    sc.check_p2(p2, coord, elem, t=t)
    assert sc.check_children(coord, elem, cu, eu, *sc.uniform_codes(elem.shape[1]), t=t).all()


@pytest.mark.parametrize('kind', ['random', 'disc'])
def test_jittered_square_marked(fep, kind):
    coord, elem, t = _square()
    marked = sc.marking(kind, elem.shape[1], coord=coord, elem=elem)
    assert 0 < marked.sum() < marked.size
    with fep.DeviceMesh(coord, elem, DEV) as m:
        got, dev, corners = _marked_round(fep, m, coord, elem, t, marked, False)
    print(f'jittered square {kind}: {got}')


# ---- d. the counters --------------------------------------------------------------------------------------------------------
def _refused_calls_write_nothing(fep, m):
    """Every writing entry point on a refused mesh: FEP_ESTATE, the canaries untouched; the Python forms raise."""
    lib, ptr = fep.lib(), fep._lib.ptr
    n_e, n_n, n_edges, n_bnd = (m.info[k] for k in ('n_e', 'n_n', 'n_edges', 'n_boundary_edges'))
    ext = np.full((15, n_e), -7, dtype=np.int32)
    cx = np.full((2, n_n + 3 * n_e + 3 * n_edges), -7.0)
    surf = np.full((5, max(n_bnd, 1)), -7, dtype=np.int32)
    ed, el = np.full((3, n_e), -7, dtype=np.int32), np.full((2, max(n_edges, 1)), -7, dtype=np.int32)
    child, parent = np.full((3, 4 * n_e), -7, dtype=np.int32), np.full(4 * n_e, -7, dtype=np.int32)
    corners = np.full((3, 4 * n_e), 0xF9, dtype=np.uint8)
    out = np.full(4, -7, dtype=np.int64)
    marks = np.ones(n_e, dtype=np.uint8)
    assert lib.fep_mesh_enrich_host(m._h, 2, ptr(ext), ptr(cx), ptr(surf), ptr(ed), ptr(el)) == ESTATE
    assert lib.fep_mesh_enrich_host(m._h, 5, ptr(ext), ptr(cx), ptr(surf), None, None) == ESTATE
    assert lib.fep_mesh_refine_host(m._h, ptr(child), ptr(cx)) == ESTATE
    assert lib.fep_mesh_mark(m._h, None, ptr(marks), 0, out.ctypes.data_as(fep._lib.c_i64_p)) == ESTATE
    assert lib.fep_mesh_refine_marked_host(m._h, ptr(child), ptr(cx), ptr(parent)) == ESTATE
    assert lib.fep_mesh_child_corners_host(m._h, ptr(corners)) == ESTATE
    for a in (ext, surf, ed, el, child, parent, out):
        assert (a == -7).all()
    assert (cx == -7.0).all() and (corners == 0xF9).all()
    for call in (lambda: m.enrich('P2'), lambda: m.enrich('P4'), m.refine, lambda: m.mark(marks)):
        with pytest.raises(ValueError, match='edge-manifold'):
            call()


def test_counters_at_scale(fep):
    coord, elem, t = _strip(LARGEST)
    n_n = coord.shape[1]
    swapped = elem.copy()
    swapped[1, -1], swapped[2, -1] = elem[2, -1], elem[1, -1]
    a, b = t.edges[:, np.flatnonzero(t.mult == 2)[-1]]                                # the last interior edge
    third = np.concatenate([elem, [[a], [b], [n_n]]], axis=1)
    far = np.concatenate([coord, [[-5.0], [7.0]]], axis=1)
    repeated = elem.copy()
    repeated[1, -1] = repeated[0, -1]
    for name, co, el, counter in (('swapped', coord, swapped, 'n_inconsistent'), ('third', far, third, 'n_nonmanifold'),
                                  ('repeated', coord, repeated, 'n_degenerate')):
        with fep.DeviceMesh(co, el, DEV) as m:
            sc.check_info(m.info, el)
            others = {'n_inconsistent', 'n_nonmanifold', 'n_degenerate'} - {counter}
            assert m.info[counter] == 1 and all(m.info[k] == 0 for k in others), (name, m.info)
            _refused_calls_write_nothing(fep, m)
    beyond = elem.copy()
    beyond[2, -1] = n_n
    with pytest.raises(fep.FepError) as ei:
        fep.DeviceMesh(coord, beyond, DEV)
    assert ei.value.code == ERANGE
    with fep.DeviceMesh(coord, elem, DEV) as m:                                      # the unmodified mesh still passes
        assert m.info == _strip_info(LARGEST)
        sc.check_p2(m.enrich('P2'), coord, elem, t=t)


# ---- e. the chain through the state transfer ----------------------------------------------------------------------------------
def _shape_of_children(fep, t, corners):
    tab = fep.transfer_tables(t)
    code = corners.astype(np.int64)
    shape = tab['shape_of_code'][code[0] + 6 * code[1] + 36 * code[2]].astype(np.int64)
    assert (shape >= 0).all()
    return tab, shape


@pytest.mark.parametrize('mesh', ['strip', 'square'])
def test_chain_through_transfer(fep, mesh):
    import torch
    dev = torch.device('cuda', DEV)
    coord, elem, t = _strip(LARGEST) if mesh == 'strip' else _square()
    n_e = elem.shape[1]
    with fep.DeviceMesh(coord, elem, DEV) as m:
        got = m.mark(sc.marking('random', n_e))
        c_d, e_d, p_d = m.refine_marked_dev()
        k_d = m.child_corners_dev()
    elem_d = torch.from_numpy(elem.astype(np.int32)).to(dev)
    u = torch.from_numpy(np.ascontiguousarray(coord.T)).to(dev)
    # weights 0, 1/2 and 1: 0 u is 0, u / 2 is exact, so the one rounding is that of u_a / 2 + u_b / 2 = (u_a + u_b) / 2
    x_child = fep.transfer_nodes_dev('P1', elem_d, e_d, p_d, k_d, u, c_d.shape[1]).cpu().numpy()
    coord_c = c_d.cpu().numpy()
    assert x_child.shape == (coord_c.shape[1], 2) and np.array_equal(x_child, coord_c.T)
    parent, corners = p_d.cpu().numpy().astype(np.int64), k_d.cpu().numpy()
    assert parent.size == got['n_child']
    for et in ('P1', 'P2'):
        tab, shape = _shape_of_children(fep, et, corners)
        n_q = tab['near'].shape[1]
        point = np.arange(n_e * n_q)
        value = (point // n_q) + (point % n_q) / 16.0                                  # parent element + point / 16: exact
        q = np.ascontiguousarray(np.stack([value, -value]))
        q_child = fep.transfer_points_dev(et, p_d, k_d, torch.from_numpy(q).to(dev)).cpu().numpy()
        src = parent[:, None] * n_q + tab['near'][shape].astype(np.int64)               # (n_child, n_q)
        assert q_child.shape == (2, parent.size * n_q) and np.array_equal(q_child, q[:, src.ravel()]), et


# ---- f. P2 fields across a marked refinement ----------------------------------------------------------------------------------
def test_p2_polynomial_across_marked_refinement(fep):
    import torch
    n = sc.LARGE_SIZES[1]
    assert n == 524288
    coord, elem, t = _strip(n)
    with fep.DeviceMesh(coord, elem, DEV) as m:
        ext_p, x_p = m.enrich_dev('P2')[:2]
        m.mark(sc.marking('random', n))
        c_d, e_d, p_d = m.refine_marked_dev()
        k_d = m.child_corners_dev()
        with fep.DeviceMesh(c_d, e_d, DEV, on_device=True) as child:
            assert (child.info['n_nonmanifold'], child.info['n_inconsistent'], child.info['n_degenerate']) == (0, 0, 0)
            ext_c, x_c = child.enrich_dev('P2')[:2]

    def field(xy):
        x, y = xy
        return np.ascontiguousarray(np.stack([(x - 2 * y) ** 2, x * y], axis=1))

    xp, xc = x_p.cpu().numpy(), x_c.cpu().numpy()
    # Exactly.  Parent nodes are multiples of 1/2 and child nodes of 1/4 with |x| < 2^25, so both fields are multiples of 1/16
    # below 2^52 / 16 and exact doubles.  P2 weights at the child's nodes are multiples of 1/8 of magnitude <= 1 and the parent
    # values multiples of 1/4, so each of the 6 products and every partial sum is a multiple of 1/32 of magnitude at most
    # 6 max |u|: exact as long as 32 * 6 * max |u| < 2^53.  A sum without rounding is the quadratic's P2 interpolant, which
    # is the quadratic itself, so no fallback to the rounding bound of test_polynomials_are_reproduced is needed.
    assert np.abs(xp).max() < 2 ** 25 and np.array_equal(xp * 2, np.round(xp * 2)) and np.array_equal(xc * 4, np.round(xc * 4))
    u = field(xp)
    W = fep.transfer_tables('P2')['W']
    assert np.array_equal(W * 8, np.round(W * 8)) and np.abs(W).max() <= 1
    assert 32 * 6 * np.abs(u).max() < 2 ** 53
    got = fep.transfer_nodes_dev('P2', ext_p, ext_c, p_d, k_d, torch.from_numpy(u).to(x_p.device), xc.shape[1]).cpu().numpy()
    assert np.array_equal(got, field(xc))

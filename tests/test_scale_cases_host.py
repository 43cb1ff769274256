"""
The checkers of scale_cases.py on the CPU: they pass on the NumPy twin's output (strips at the tile edge, the unstructured
mesh, the tunnel), agree there with the twin-based checks of marked_cases.py, and reject every single mutation a wrong
numbering would produce.  A checker that accepts everything closes no gap.  Also the closed forms of strip(n) at all
fourteen sizes, against the edge table.
"""
import numpy as np
import pytest

import marked_cases as mc
import scale_cases as sc

fep = mc.fep


# ---- sizes and closed forms -------------------------------------------------------------------------------------------------
def test_sizes_sit_on_the_tile_edges():
    assert sc.SMALL_SIZES == [511, 512, 1021, 1022, 1023, 1024, 1025]
    assert sc.LARGE_SIZES == [524287, 524288, 1048573, 1048574, 1048575, 1048576, 1048577]
    for sizes, limit, below in ((sc.SMALL_SIZES, 1024, 1), (sc.LARGE_SIZES, 1024 ** 2, 2)):
        for name in ('n_n + 1', 'n_e + 1', 'n_edges + 1'):
            lengths = sorted(sc.scanned_lengths(n)[name] for n in sizes)
            at = max(v for v in lengths if v <= limit)
            past = min(v for v in lengths if v > limit)
            assert limit - at <= (1 if name == 'n_edges + 1' else 0) and past - at <= 2, (name, at, past)
            assert at >= limit - 1 and (name == 'n_edges + 1' or at == limit)
            assert (sc.scan_levels(at), sc.scan_levels(past)) == (below, below + 1)
    assert [sc.scan_levels(v) for v in (1, 1024, 1025, 1024 ** 2, 1024 ** 2 + 1)] == [1, 1, 2, 2, 3]
    assert sc.scanned_lengths(511)['n_edges + 1'] == 1024 and sc.scanned_lengths(524287)['n_edges + 1'] == 1024 ** 2
    assert sc.max_sweeps() == 8


@pytest.mark.parametrize('n', sc.SMALL_SIZES + sc.LARGE_SIZES)
def test_strip_closed_forms(n):
    coord, elem = sc.strip(n)
    n_n, n_e, n_edges, n_bnd = sc.strip_counts(n)
    assert coord.shape == (2, n_n) and elem.shape == (3, n_e) and np.array_equal(np.unique(elem), np.arange(n_n))
    assert np.array_equal(coord, np.round(coord))
    t = sc.edge_table(elem)
    assert t.mult.size == n_edges and int((t.mult == 1).sum()) == n_bnd and t.mult.max() == 2 and t.opposite[t.mult == 2].all()
    assert np.array_equal(t.edges[:, t.he], np.sort(np.stack([elem, elem[[1, 2, 0]]]), axis=0))
    assert (sc.doubled_areas(coord, elem) == 1).all()
    x, y = coord
    length = (x[elem[[1, 2, 0]]] - x[elem]) ** 2 + (y[elem[[1, 2, 0]]] - y[elem]) ** 2
    r = sc.reference_edge(coord, elem)
    assert np.array_equal(r, np.where(np.arange(n) % 2 == 0, 1, 2))                  # the diagonal, strictly longest
    assert np.array_equal(np.sort(length, axis=0), np.tile([[1.0], [1.0], [2.0]], (1, n)))
    partner = np.arange(n) ^ 1                                                       # ... shared with the cell partner
    has = partner < n
    assert np.array_equal(t.he[r, np.arange(n)][has], t.he[r[partner[has]], partner[has]])


# ---- the checkers pass where the twin is right --------------------------------------------------------------------------------
def _case(name):
    if name == 'unstructured':
        return mc.unstructured()
    if name == 'tunnel':
        return mc.tunnel()
    return sc.strip(int(name))


CASES = [str(n) for n in sc.SMALL_SIZES] + ['unstructured', 'tunnel']


def _marks(name, coord, elem):
    n_e = elem.shape[1]
    out = {k: sc.marking(k, n_e) for k in ('none', 'all', 'random', 'first', 'last')}
    if name == 'tunnel':
        out['near'] = mc.near_tunnel(None, coord, elem)
    return out


@pytest.mark.parametrize('name', CASES)
def test_checkers_pass_on_the_twin(name):
    coord, elem = _case(name)
    exact = name not in ('unstructured', 'tunnel')
    n_e, n_n = elem.shape[1], coord.shape[1]
    t = sc.edge_table(elem)
    n_edges, n_bnd, n_nm, n_inc, n_deg = mc.edge_counts(elem)
    info = dict(n_e=n_e, n_n=n_n, n_edges=n_edges, n_boundary_edges=n_bnd, n_nonmanifold=n_nm, n_inconsistent=n_inc, n_degenerate=n_deg)
    sc.check_info(info, elem)
    sc.check_p2(fep.create_midpoints_P2(coord, elem), coord, elem, t=t)
    p4 = fep.create_midpoints_P4(coord, elem)
    sc.check_p4(p4, coord, elem, ulps=0, t=t)
    sc.check_p4(p4, coord, elem, ulps=2, t=t)
    cu, eu = fep.refine_uniform(coord, elem)
    parent_u, corners_u = sc.uniform_codes(n_e)
    assert np.array_equal(corners_u, fep.uniform_corners(n_e)[0])
    split = sc.check_children(coord, elem, cu, eu, parent_u, corners_u, exact=exact, t=t)
    assert split.all()
    for kind, marked in _marks(name, coord, elem).items():
        c, e, p = fep.refine_marked(coord, elem, marked)
        corners = fep.child_corners(coord, elem, marked)
        split = sc.check_children(coord, elem, c, e, p, corners, exact=exact, t=t)
        state = sc.check_marks(coord, elem, marked, split, p, corners, t=t)
        assert sc.closure_counts(state, t) == (e.shape[1], c.shape[1] - n_n), kind
        mc.check_conforming(coord, elem, mc.marked_boundary_edges(coord, elem, c, e), c, e, p)
        if kind == 'all':
            assert state.all() and c.tobytes() == cu.tobytes()
        if kind == 'none':
            assert not state.any()
        if exact and kind in ('first', 'last'):                                      # the two-step closure of the strip
            assert state.any(axis=0).sum() <= 4


def test_counters_agree_with_the_twin_on_refused_meshes():
    coord, elem = sc.strip(13)
    swapped = elem.copy()
    swapped[1, -1], swapped[2, -1] = elem[2, -1], elem[1, -1]
    t = sc.edge_table(elem)
    a, b = t.edges[:, np.flatnonzero(t.mult == 2)[-1]]
    third = np.concatenate([elem, [[a], [b], [coord.shape[1]]]], axis=1)
    repeated = elem.copy()
    repeated[1, -1] = repeated[0, -1]
    for el, n_n in ((swapped, 15), (third, 16), (repeated, 15)):
        n_edges, n_bnd, n_nm, n_inc, n_deg = mc.edge_counts(el[:, (el[0] != el[1]) & (el[1] != el[2]) & (el[2] != el[0])])
        n_deg = int(((el[0] == el[1]) | (el[1] == el[2]) | (el[2] == el[0])).sum())
        if n_nm:                                   # the twin counts repeated directed edges; the header only interior edges of TWO elements
            n_inc = 0
        info = dict(n_e=el.shape[1], n_n=n_n, n_edges=n_edges, n_boundary_edges=n_bnd, n_nonmanifold=n_nm, n_inconsistent=n_inc,
                    n_degenerate=n_deg)
        assert n_nm + n_inc + n_deg == 1
        sc.check_info(info, el)
        for key in ('n_nonmanifold', 'n_inconsistent', 'n_degenerate', 'n_boundary_edges'):
            with pytest.raises(AssertionError):
                sc.check_info(dict(info, **{key: info[key] + 1}), el)


# ---- and fail where it is wrong -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['1025', 'unstructured'])
def good(request):
    coord, elem = _case(request.param)
    marked = sc.marking('random', elem.shape[1])
    c, e, p = fep.refine_marked(coord, elem, marked)
    return dict(coord=coord, elem=elem, marked=marked, t=sc.edge_table(elem), exact=request.param == '1025',
                p2=fep.create_midpoints_P2(coord, elem), p4=fep.create_midpoints_P4(coord, elem),
                child=(c, e, p), corners=fep.child_corners(coord, elem, marked))


def _copy(h):
    return {k: np.array(v, copy=True) for k, v in h.items()}


def _interior_element(g):
    """An element with as many interior edges as the mesh offers (the strip: two), past the middle of the mesh."""
    inside = (g['t'].mult[g['t'].he] == 2).sum(axis=0)
    most = np.flatnonzero(inside == inside.max())
    return int(most[most.size // 2])


def _rejected(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def _children(g, coord_c=None, elem_c=None, parent=None, corners=None):
    c, e, p = g['child']
    return sc.check_children(g['coord'], g['elem'], c if coord_c is None else coord_c, e if elem_c is None else elem_c,
                             p if parent is None else parent, g['corners'] if corners is None else corners, exact=g['exact'], t=g['t'])


def test_the_unmutated_outputs_pass(good):
    g = good
    sc.check_p2(g['p2'], g['coord'], g['elem'], t=g['t'])
    sc.check_p4(g['p4'], g['coord'], g['elem'], t=g['t'])
    split = _children(g)
    sc.check_marks(g['coord'], g['elem'], g['marked'], split, g['child'][2], g['corners'], t=g['t'])


def test_two_ids_swapped_in_one_element_are_rejected(good):
    g, i = good, _interior_element(good)
    h = _copy(g['p2'])
    h['elem_ext'][[3, 4], i] = h['elem_ext'][[4, 3], i]
    h['elem_ed'][[0, 1], i] = h['elem_ed'][[1, 0], i]
    _rejected(sc.check_p2, h, g['coord'], g['elem'], t=g['t'])
    for rows in ([3, 4], [6, 7], [6, 8]):                                             # midpoints; an edge's own pair; two edges' quarter points
        h = _copy(g['p4'])
        h['elem_ext'][rows, i] = h['elem_ext'][rows[::-1], i]
        _rejected(sc.check_p4, h, g['coord'], g['elem'], t=g['t'])
    h = _copy(g['p4'])                                                               # the pair swapped in BOTH elements of an edge
    edge = g['t'].he[int(np.argmax(g['t'].mult[g['t'].he[:, i]])), i]
    holds = np.argwhere(g['t'].he == edge)
    for k, j in holds:
        h['elem_ext'][[6 + 2 * k, 7 + 2 * k], j] = h['elem_ext'][[7 + 2 * k, 6 + 2 * k], j]
    assert len(holds) == 2
    _rejected(sc.check_p4, h, g['coord'], g['elem'], t=g['t'])


def test_a_midpoint_one_ulp_off_is_rejected(good):
    g = good
    n_n = g['coord'].shape[1]
    for key, check, col in (('p2', sc.check_p2, n_n + 17), ('p4', sc.check_p4, n_n + 17), ('p4', sc.check_p4, g['p4']['coord_ext'].shape[1] - 1)):
        for row in (0, 1):
            h = _copy(g[key])
            h['coord_ext'][row, col] = np.nextafter(h['coord_ext'][row, col], np.inf)
            h['coord_mid'] = h['coord_ext'][:, n_n:]
            _rejected(check, h, g['coord'], g['elem'], t=g['t'])
    c = g['child'][0].copy()
    c[1, -1] = np.nextafter(c[1, -1], -np.inf)
    _rejected(_children, g, coord_c=c)
    c = g['child'][0].copy()                                                         # an old node
    c[0, 3] = np.nextafter(c[0, 3], np.inf)
    _rejected(_children, g, coord_c=c)


def test_three_roundings_pass_the_ulp_bound_and_a_fourth_ulp_does_not():
    coord, elem = mc.unstructured()
    h = fep.create_midpoints_P4(coord, elem)
    n_n = coord.shape[1]
    big = int(np.argmax(np.abs(h['coord_ext'][0, n_n:]))) + n_n
    for ulp, ok in ((1, True), (4, False)):
        m = _copy(h)
        m['coord_ext'][0, big] += ulp * np.spacing(np.abs(coord).max()) * np.sign(m['coord_ext'][0, big])
        m['coord_mid'] = m['coord_ext'][:, n_n:]
        if ok:
            sc.check_p4(m, coord, elem, ulps=2)
        else:
            _rejected(sc.check_p4, m, coord, elem, ulps=2)


def test_a_child_with_two_vertices_exchanged_is_rejected(good):
    e = good['child'][1].copy()
    ch = e.shape[1] // 2
    e[[1, 2], ch] = e[[2, 1], ch]
    _rejected(_children, good, elem_c=e)
    corners = good['corners'].copy()                                                  # ... also when its codes follow it
    corners[[1, 2], ch] = corners[[2, 1], ch]
    _rejected(_children, good, elem_c=e, corners=corners)


def test_a_parent_entry_off_by_one_is_rejected(good):
    p0 = good['child'][2]
    last_of_a_family = int(np.flatnonzero(np.diff(p0) == 1)[p0.size // 8])
    for ch, step in ((last_of_a_family, 1), (last_of_a_family + 1, -1), (0, 1), (p0.size - 1, -1)):
        p = p0.copy()
        p[ch] += step
        _rejected(_children, good, parent=p)


def test_a_corner_code_3_for_4_is_rejected(good):
    corners = good['corners'].copy()
    k, ch = (int(v[0]) for v in np.nonzero(corners == 3))
    corners[k, ch] = 4
    _rejected(_children, good, corners=corners)
    corners = good['corners'].copy()
    k, ch = (int(v[-1]) for v in np.nonzero(corners == 4))
    corners[k, ch] = 3
    _rejected(_children, good, corners=corners)


def test_a_split_edge_left_out_of_the_closure_is_rejected(good):
    g = good
    split = _children(g)
    p = g['child'][2]
    sc.check_marks(g['coord'], g['elem'], g['marked'], split, p, g['corners'], t=g['t'])
    edge = g['t'].he[np.nonzero(split)][split.sum() // 2]
    less = split & (g['t'].he != edge)
    assert split.sum() - less.sum() in (1, 2)
    _rejected(sc.check_marks, g['coord'], g['elem'], g['marked'], less, p, g['corners'], t=g['t'])
    # and marks whose closure is smaller than what was split: one marked element fewer
    fewer = g['marked'].copy()
    fewer[np.flatnonzero(fewer)[0]] = False
    _rejected(sc.check_marks, g['coord'], g['elem'], fewer, split, p, g['corners'], t=g['t'])
    # counts derived from a closure that misses the edge differ from the mesh's
    assert sc.closure_counts(less, g['t']) != sc.closure_counts(split, g['t'])


def test_a_duplicated_surf_column_is_rejected(good):
    g = good
    for key, check in (('p2', sc.check_p2), ('p4', sc.check_p4)):
        h = _copy(g[key])
        h['surf'][:, 5] = h['surf'][:, 4]
        _rejected(check, h, g['coord'], g['elem'], t=g['t'])
        h = _copy(g[key])                                                            # the node row alone
        h['surf'][2, 5] = h['surf'][2, 4]
        _rejected(check, h, g['coord'], g['elem'], t=g['t'])
        h = _copy(g[key])                                                            # walked the other way
        h['surf'][[0, 1], 5] = h['surf'][[1, 0], 5]
        _rejected(check, h, g['coord'], g['elem'], t=g['t'])


def test_ids_shifted_from_some_element_on_are_rejected(good):
    """The signature of a wrong block sum: everything behind a tile edge moves by one."""
    g, i = good, _interior_element(good)
    h = _copy(g['p2'])
    h['elem_ext'][3:, i:] += 1
    h['elem_ed'][:, i:] += 1
    _rejected(sc.check_p2, h, g['coord'], g['elem'], t=g['t'])
    h = _copy(g['p4'])
    h['elem_ext'][3:, i:] += 1
    _rejected(sc.check_p4, h, g['coord'], g['elem'], t=g['t'])
    c, e, p = g['child']
    n_n = g['coord'].shape[1]
    shifted = e.copy()
    behind = np.zeros(e.shape, dtype=bool)
    behind[:, e.shape[1] // 2:] = True
    shifted[behind & (e >= n_n) & (e < c.shape[1] - 1)] += 1
    assert not np.array_equal(shifted, e)
    _rejected(_children, g, elem_c=shifted)
    for q in (np.concatenate([p[:p.size // 2], p[p.size // 2:] + 1]), np.concatenate([p[:p.size // 2], p[p.size // 2:] - 1])):
        _rejected(_children, g, parent=q)
    # children written one place further from some parent on (m_cbase off by one): one column repeated, the last one lost
    at = e.shape[1] // 2
    moved = np.concatenate([e[:, :at], e[:, at - 1:-1]], axis=1)
    _rejected(_children, g, elem_c=moved)

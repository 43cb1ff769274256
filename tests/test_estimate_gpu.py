"""
The recovered-stress error indicator on the GPU (fep_recover_stress_*, fep_estimate_*, fep_mark_bulk_*) against its NumPy
twin (fem-elastoplasticity_amd/estimate.py, itself held to a long-double reference by tests/test_estimate_host.py): every
array bit for bit (a NaN counts as a NaN whatever its sign bit: 0/0 is -NaN on the host and +NaN on the device), on the
shapes at which a lane, a workgroup or a tree level ends; the non-finite rules; the refusals; the device chain from the
step to the refined mesh; the tunnel driver.
"""
import ctypes as C
from contextlib import closing

import numpy as np
import pytest

import estimate_cases as ec
import exact_cases as xc
import fan_mesh

pytestmark = pytest.mark.gpu

DEV = 0
EINVAL, ESTATE = -1, -6                                       # include/fep.h
CANARY = -7.25


def same(a, b):
    """Bit for bit, NaNs as NaNs."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != 'f':
        assert a.tobytes() == b.tobytes()
        return
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (int(na.sum()), int(nb.sum()))
    assert a[~na].tobytes() == b[~nb].tobytes(), int((a[~na] != b[~nb]).sum())


def strip(n, seed=2):
    """n triangles in a row (n + 2 nodes): bottom nodes 0 .., top nodes behind them, jittered so that no two weights agree."""
    nc = n // 2 + 1
    rng = np.random.default_rng(seed + n)
    x = np.concatenate([np.arange(nc + 1), np.arange(nc + 1)]) + rng.uniform(-0.2, 0.2, 2 * nc + 2)
    y = np.concatenate([np.zeros(nc + 1), np.ones(nc + 1)]) + rng.uniform(-0.2, 0.2, 2 * nc + 2)
    c = np.arange(nc)
    b0, b1, t0, t1 = c, c + 1, nc + 1 + c, nc + 2 + c
    elem = np.stack([np.stack([b0, b1, t0]), np.stack([b1, t1, t0])], axis=2).reshape(3, -1)[:, :n]
    used = np.unique(elem)
    new = np.full(2 * nc + 2, -1)
    new[used] = np.arange(used.size)
    return np.ascontiguousarray(new[elem], dtype=np.int64), np.ascontiguousarray(np.stack([x, y])[:, used])


def one_element(fep, et):
    if et in ('Q1', 'Q2'):
        m = fep.rect_mesh(1, 1, et, 1.3, 0.8)
        return np.ascontiguousarray(m['elements'], dtype=np.int64), np.ascontiguousarray(m['coordinates'], dtype=np.float64)
    coord, elem = np.array([[0.0, 2.0, 0.5], [0.0, 0.3, 1.5]]), np.array([[0], [1], [2]], dtype=np.int64)
    if et == 'P1':
        return elem, coord
    h = fep.create_midpoints(et, coord, elem)
    return np.ascontiguousarray(h['elem_ext'], dtype=np.int64), np.ascontiguousarray(h['coord_ext'], dtype=np.float64)


def type_mesh(fep, et):
    if et in ('Q1', 'Q2'):
        m = fep.rect_mesh(3, 3, et, 1.0, 1.0)
        return np.ascontiguousarray(m['elements'], dtype=np.int64), np.ascontiguousarray(m['coordinates'], dtype=np.float64)
    m = xc.mesh(fep, 'ring', et, 1)
    return m['elem'], m['coord']


def materials(n_int, per_point, seed=4):
    """(shear, bulk, m3, m4): per point, or constant shear and bulk."""
    rng = np.random.default_rng(seed)
    one = np.ones(n_int)
    if per_point:
        return xc.SHEAR * rng.uniform(0.5, 2.0, n_int), xc.BULK * rng.uniform(0.5, 2.0, n_int), 0.1 * one, 1e9 * one
    return xc.SHEAR * one, xc.BULK * one, 0.1 * one, 1e9 * one


def tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', DEV))


def run_all_forms(fep, et, elem, coord, s, mats, model='dp'):
    """The twin's result, after holding the _host and the _dev forms of both calls to it."""
    import torch
    hatp = ec.hatp_of(fep, et)
    n_n = coord.shape[1]
    with closing(fep.MeshContext(elem, coord, *fep.element_tables(et), device=DEV)) as ctx:
        if model != 'dp':
            ctx.set_model(model)
        ctx.set_materials(*mats)
        w = np.asarray(ctx.geometry()[2], dtype=float).ravel()
        twin = fep.estimate_np(elem, w, mats[0], mats[1], hatp, s, n_n)
        host = ctx.estimate(s)
        same(ctx.recover_stress(s), twin['s_node'])
        same(host['s_node'], twin['s_node'])
        same(host['eta2'], twin['eta2'])
        assert (host['total'], host['max'], host['n_nonfinite']) == (twin['total'], twin['max'], twin['n_nonfinite'])
        s_d = tensor(s)
        eta2_d, st_d, sn_d = ctx.estimate_dev(s_d)
        eta2_again, no_stats, _ = ctx.estimate_dev(s_d, s_node=sn_d, stats=False)
        torch.cuda.synchronize(DEV)
        assert no_stats is None
        same(sn_d.cpu().numpy(), twin['s_node'])
        same(eta2_d.cpu().numpy(), twin['eta2'])
        same(eta2_again.cpu().numpy(), twin['eta2'])
        same(st_d.cpu().numpy(), np.array([twin['total'], twin['max'], float(twin['n_nonfinite']), float(elem.shape[1])]))
    return twin


def random_stress(n_int, seed=9):
    return np.random.default_rng(seed).normal(0.0, 50.0, (4, n_int))


@pytest.mark.parametrize('et', ['P1', 'P2', 'Q1', 'Q2', 'P4'])
def test_every_type_one_element_and_a_mesh(fep, et):
    n_q = fep.ELEMENT_SHAPE[fep.LagrangeElementType[et]][1]
    for elem, coord in (one_element(fep, et), type_mesh(fep, et)):
        n_int = elem.shape[1] * n_q
        twin = run_all_forms(fep, et, elem, coord, random_stress(n_int), materials(n_int, True))
        # (one P1 element recovers its own stress: eta2 = 0 exactly)
        assert twin['n_nonfinite'] == 0 and (twin['eta2'] >= 0).all() and (elem.shape[1] == 1 or twin['max'] > 0)


@pytest.mark.parametrize('n', [254, 255, 256, 257])
def test_p1_strips_at_the_lane_and_workgroup_edges(fep, n):
    """n_e = 254 .. 257 triangles on n_e + 2 nodes: the last lane of a workgroup and the first of the next, for elements
    (255, 256, 257) and for nodes (256, 257)."""
    elem, coord = strip(n)
    assert elem.shape == (3, n) and coord.shape == (2, n + 2)
    run_all_forms(fep, 'P1', elem, coord, random_stress(n), materials(n, True))


def test_long_incidence_list(fep):
    """The hub of fan_mesh(250): 250 elements around one node."""
    elem, coord = fan_mesh.fan_mesh(250, 'P1')
    assert np.bincount(elem.ravel()).max() == 250
    run_all_forms(fep, 'P1', elem, coord, random_stress(elem.shape[1]), materials(elem.shape[1], True))


@pytest.mark.parametrize('et', ['P1', 'P2'])
def test_node_of_no_element(fep, et):
    elem, coord = type_mesh(fep, et)
    coord = np.ascontiguousarray(np.concatenate([coord, [[9.0], [9.0]]], axis=1))
    n_int = elem.shape[1] * fep.ELEMENT_SHAPE[fep.LagrangeElementType[et]][1]
    twin = run_all_forms(fep, et, elem, coord, random_stress(n_int), materials(n_int, False))
    assert np.isnan(twin['s_node'][:, -1]).all() and twin['n_nonfinite'] == 0


@pytest.mark.parametrize('et', ['P1', 'Q2'])
def test_per_point_and_constant_materials_give_the_same_bytes(fep, et):
    """Constant shear and bulk: once with all four parameters constant (the kernels take the constants), once with a
    varying fourth parameter (they read the arrays)."""
    elem, coord = type_mesh(fep, et)
    n_int = elem.shape[1] * fep.ELEMENT_SHAPE[fep.LagrangeElementType[et]][1]
    s = random_stress(n_int)
    const = materials(n_int, False)
    varying = const[:3] + (const[3] * np.linspace(1.0, 2.0, n_int),)
    a = run_all_forms(fep, et, elem, coord, s, const)
    b = run_all_forms(fep, et, elem, coord, s, varying)
    assert a['eta2'].tobytes() == b['eta2'].tobytes()


def test_plane_stress_context(fep):
    """The indicator does not depend on the context's model: a 'vmps' context, s33 = 0."""
    elem, coord = type_mesh(fep, 'P2')
    n_int = elem.shape[1] * 7
    s = random_stress(n_int)
    s[3] = 0.0
    mats = materials(n_int, True)
    a = run_all_forms(fep, 'P2', elem, coord, s, mats, model='vmps')
    b = run_all_forms(fep, 'P2', elem, coord, s, mats)
    assert a['eta2'].tobytes() == b['eta2'].tobytes()


# ---- marking ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def twin_marks(fep):
    return {(n, th): fep.mark_bulk(ec.value_set(n), th) for n in ec.MARK_SIZES for th in ec.THETAS}


@pytest.mark.parametrize('n', ec.MARK_SIZES)
def test_mark_bulk_dev_against_the_twin(fep, twin_marks, n):
    """65 537 values reach the third tree level (65 537 -> 257 -> 2 -> 1)."""
    import torch
    v = ec.value_set(n)
    v_d = tensor(v)
    for th in ec.THETAS:
        want_marked, want_out = twin_marks[(n, th)]
        marked_d, out_d = fep.mark_bulk(v_d, th)
        torch.cuda.synchronize(DEV)
        assert marked_d.dtype == torch.uint8
        same(marked_d.cpu().numpy().view(np.bool_), want_marked)
        same(out_d.cpu().numpy(), want_out)
        marked_h, out_h = fep.mark_bulk(v, th, device=DEV)
        same(marked_h, want_marked)
        same(out_h, want_out)


def test_mark_bulk_special_values(fep):
    for v in (np.full(300, 0.7), np.zeros(300), np.zeros(0)):
        for device in (None, DEV):
            marked, out = fep.mark_bulk(v, 0.3, device=device)
            assert marked.all() == (v.size == 0 or v[0] > 0) and marked.shape == v.shape
            if not (v > 0).any():
                assert np.array_equal(out, [np.inf, 0.0, 0.0, 0.0]) and not marked.any()
    v = ec.value_set(257)
    v[3], v[200], v[17] = np.nan, np.inf, -np.inf
    want_marked, want_out = fep.mark_bulk(v, 0.5)
    marked, out = fep.mark_bulk(v, 0.5, device=DEV)
    same(marked, want_marked)
    same(out, want_out)
    assert not marked[[3, 200, 17]].any() and marked.any()


def test_refusals_write_nothing(fep):
    import torch
    l = fep.lib()
    v_d = tensor(ec.value_set(300))
    marked = torch.full((300,), 9, dtype=torch.uint8, device=v_d.device)
    out = torch.full((4,), CANARY, dtype=torch.float64, device=v_d.device)
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    for n, eta2, theta, mk, o in ((300, p(v_d), 0.0, p(marked), p(out)), (300, p(v_d), 1.5, p(marked), p(out)),
                                  (300, p(v_d), float('nan'), p(marked), p(out)), (-1, p(v_d), 0.5, p(marked), p(out)),
                                  (300, None, 0.5, p(marked), p(out)), (300, p(v_d), 0.5, None, p(out)),
                                  (300, p(v_d), 0.5, p(marked), None)):
        assert l.fep_mark_bulk_dev(DEV, None, n, eta2, theta, mk, o) == EINVAL
    host = np.full(4, CANARY)
    assert l.fep_mark_bulk_host(DEV, 300, None, 0.5, None, fep._lib.ptr(host)) == EINVAL
    torch.cuda.synchronize(DEV)
    assert (marked.cpu().numpy() == 9).all() and (out.cpu().numpy() == CANARY).all() and (host == CANARY).all()
    assert l.fep_mark_bulk_dev(DEV, None, 0, None, 0.5, None, p(out)) == 0              # n = 0 is legal
    torch.cuda.synchronize(DEV)
    assert np.array_equal(out.cpu().numpy(), [np.inf, 0.0, 0.0, 0.0])
    # the context calls: NULL pointers, a table missing where it is read, materials not set
    elem, coord = type_mesh(fep, 'P2')
    with closing(fep.MeshContext(elem, coord, *fep.element_tables('P2'), device=DEV)) as ctx:
        s, sn = tensor(random_stress(ctx.n_int)), torch.full((4, ctx.n_n), CANARY, dtype=torch.float64, device=v_d.device)
        eta2 = torch.full((ctx.n_e,), CANARY, dtype=torch.float64, device=v_d.device)
        h = fep._lib.ptr(ec.hatp_of(fep, 'P2'))
        assert l.fep_recover_stress_dev(ctx.handle, None, None, p(sn)) == EINVAL
        assert l.fep_recover_stress_dev(ctx.handle, None, p(s), None) == EINVAL
        assert l.fep_estimate_dev(ctx.handle, None, h, p(s), p(sn), p(eta2), p(out)) == ESTATE
        ctx.set_materials(*materials(ctx.n_int, False))
        assert l.fep_estimate_dev(ctx.handle, None, None, p(s), p(sn), p(eta2), p(out)) == EINVAL
        assert l.fep_estimate_dev(ctx.handle, None, h, p(s), p(sn), None, p(out)) == EINVAL
        assert l.fep_estimate_dev(None, None, h, p(s), p(sn), p(eta2), p(out)) == EINVAL
        torch.cuda.synchronize(DEV)
        assert (eta2.cpu().numpy() == CANARY).all() and (sn.cpu().numpy() == CANARY).all()
        assert np.array_equal(out.cpu().numpy(), [np.inf, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        fep.mark_bulk(v_d, 0.0)


def test_mark_bulk_in_a_stream_capture(fep, twin_marks):
    """The _dev form only enqueues.  On a stream without its scratch a capture is refused with FEP_ESTATE (no allocation under
    capture); after one call outside, the same call captures, and a replay marks the CURRENT contents of eta2 (theta is baked
    into the launches)."""
    import torch
    n = 65537
    v_d = tensor(ec.value_set(n))
    side = torch.cuda.Stream(DEV)
    refused = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        try:
            fep.mark_bulk(v_d, 0.5)
        except fep.FepError as e:
            refused = e.code
    assert refused == ESTATE
    with torch.cuda.stream(side):
        fep.mark_bulk(v_d, 0.5)                                                     # outside a capture: makes the scratch
    torch.cuda.synchronize(DEV)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        marked_d, out_d = fep.mark_bulk(v_d, 0.5)
    other = ec.value_set(n, seed=4)
    v_d.copy_(tensor(other))
    g2.replay()
    torch.cuda.synchronize(DEV)
    want_marked, want_out = fep.mark_bulk(other, 0.5)
    same(marked_d.cpu().numpy().view(np.bool_), want_marked)
    same(out_d.cpu().numpy(), want_out)
    assert not np.array_equal(want_marked, twin_marks[(n, 0.5)][0])


# ---- non-finite values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', [np.nan, np.inf])
def test_non_finite_stress_is_visible_contained_and_leaves_no_trace(fep, poison):
    import torch
    elem, coord = strip(257)
    s = random_stress(257)
    mats = materials(257, True)
    e_bad = 130
    touched = np.isin(elem, elem[:, e_bad]).any(axis=0)
    assert 3 <= touched.sum() < 10
    with closing(fep.MeshContext(elem, coord, *fep.element_tables('P1'), device=DEV)) as ctx:
        ctx.set_materials(*mats)
        w = np.asarray(ctx.geometry()[2], dtype=float).ravel()
        before = ctx.estimate(s)
        bad = s.copy()
        bad[2, e_bad] = poison
        got = ctx.estimate(bad)
        eta2_d, st_d, _ = ctx.estimate_dev(tensor(bad))
        marked_d, out_d = fep.mark_bulk(eta2_d, 0.5)
        torch.cuda.synchronize(DEV)
        after = ctx.estimate(s)
    twin = fep.estimate_np(elem, w, mats[0], mats[1], None, bad, coord.shape[1])
    assert np.array_equal(~np.isfinite(got['eta2']), touched)                       # visible, and nowhere else
    assert got['eta2'][~touched].tobytes() == before['eta2'][~touched].tobytes()    # contained
    assert got['n_nonfinite'] == int(touched.sum()) == int(st_d.cpu()[2])
    assert got['total'] == twin['total'] == fep.tree_sum(np.where(touched, 0.0, before['eta2'])) and got['max'] == twin['max']
    same(np.isfinite(got['eta2']), np.isfinite(twin['eta2']))
    want_marked, want_out = fep.mark_bulk(np.where(touched, 0.0, before['eta2']), 0.5)    # excluded from every sum, never marked
    same(marked_d.cpu().numpy().view(np.bool_), want_marked)
    same(out_d.cpu().numpy(), want_out)
    assert not want_marked[touched].any()
    for k in ('eta2', 's_node'):                                                    # no trace
        assert after[k].tobytes() == before[k].tobytes()
    assert (after['total'], after['max'], after['n_nonfinite']) == (before['total'], before['max'], 0)


# ---- the device chain -------------------------------------------------------------------------------------------------------
def test_device_chain_step_to_refined_mesh(fep):
    """step_dev -> estimate_dev -> mark_bulk on the device -> DeviceMesh.mark(on_device=True) -> refine_marked_dev on the
    Lame ring at level 2, no host array in between; against the same chain through host arrays and the NumPy refine_marked."""
    import torch
    m = xc.mesh(fep, 'ring', 'P1', 2, device=DEV)
    elem, coord = m['elem'], m['coord']
    curves = xc.ring_base(fep, range(6))[2]
    U = xc.flat(xc.lame(coord, m['centre']))
    with closing(fep.MeshContext(elem, coord, *fep.element_tables('P1'), device=DEV)) as ctx:
        ctx.set_materials(*materials(ctx.n_int, False))
        stream = torch.cuda.current_stream(DEV).cuda_stream
        u_d = tensor(U)
        s_d = torch.empty((4, ctx.n_int), dtype=torch.float64, device=u_d.device)
        ind_d = torch.empty(ctx.n_int, dtype=torch.uint8, device=u_d.device)
        ctx.step_dev(stream, u_d.data_ptr(), s=s_d.data_ptr(), ind_p=ind_d.data_ptr())       # an accepting call's outputs
        eta2_d, st_d, _ = ctx.estimate_dev(s_d)
        marked_d, out_d = fep.mark_bulk(eta2_d, 0.5)
        with fep.DeviceMesh(coord, elem, DEV) as dm:
            dm.set_curves(curves)
            info = dm.mark(marked_d, on_device=True)
            c_d, e_d, p_d = dm.refine_marked_dev()
            torch.cuda.synchronize(DEV)
            # through host arrays
            s_h = ctx.step(U, want=('s',))['s']
            est = ctx.estimate(s_h)
            marked_h, out_h = fep.mark_bulk(est['eta2'], 0.5, device=DEV)
            dm.mark(marked_h)
            c_h, e_h, p_h = dm.refine_marked()
        w = np.asarray(ctx.geometry()[2], dtype=float).ravel()
    same(s_d.cpu().numpy(), np.asarray(s_h))
    same(eta2_d.cpu().numpy(), est['eta2'])
    same(marked_d.cpu().numpy().view(np.bool_), marked_h)
    same(out_d.cpu().numpy(), out_h)
    assert 0 < marked_h.sum() < elem.shape[1] and info['n_child'] == e_h.shape[1] > elem.shape[1]
    same(c_d.cpu().numpy(), c_h)
    same(e_d.cpu().numpy().astype(np.int64), e_h)
    same(p_d.cpu().numpy().astype(np.int64), p_h)
    # and the twin all the way: indicator, marks, refinement
    twin = fep.estimate_np(elem, w, xc.SHEAR, xc.BULK, None, np.asarray(s_h), coord.shape[1])
    marked_t, out_t = fep.mark_bulk(twin['eta2'], 0.5)
    same(marked_h, marked_t)
    same(out_h, out_t)
    c_t, e_t, p_t = fep.refine_marked(coord, elem, marked_t, curves=curves)
    same(c_h, c_t)
    same(e_h, e_t)
    same(p_h, p_t)


# ---- the driver -------------------------------------------------------------------------------------------------------------
def test_driver_zz_gpu_against_the_host_run(fep):
    """solve_tsx_tunnel(adapt=2, mark='zz') on the GPU and under the oracle context (the NumPy twin).  The two stresses differ
    by the rounding of two solvers, so a round's marks agree except among the values within 1e-8 of its threshold; rounds
    are compared for as long as the meshes are the same."""
    import marked_cases as mc
    from oracle_context import OracleContext
    coord, elem = mc.tunnel()
    kw = dict(adapt=2, mark='zz', theta=0.5, n_load_steps=4)
    g = fep.solve_tsx_tunnel(coord, elem, 'P1', **kw)                            # host vectors, MeshContext.estimate
    h = fep.solve_tsx_tunnel(coord, elem, 'P1', context_factory=OracleContext, **kw)
    d = fep.solve_tsx_tunnel(coord, elem, 'P1', linear_solver='pcg', **kw)       # device vectors, MeshContext.estimate_dev
    assert len(g['adapt']) == len(h['adapt']) == len(d['adapt']) == 3
    # (conjugate gradients stop at a residual of 1e-11; with K's condition number of about 1e5 on this mesh: 1e-6)
    assert d['adapt'][0]['eta'] > 0 and abs(d['adapt'][0]['eta'] / g['adapt'][0]['eta'] - 1) <= 1e-6
    assert np.abs(d['adapt'][0]['eta2'] - g['adapt'][0]['eta2']).max() <= 1e-6 * g['adapt'][0]['eta2'].max()
    for a, b in zip(g['adapt'], h['adapt']):
        assert a['eta'] > 0 and b['eta'] > 0 and a['theta'] == b['theta'] == 0.5 and a['n_nonfinite'] == b['n_nonfinite'] == 0
        assert a['n_e'] == b['n_e'] and abs(a['eta'] / b['eta'] - 1) <= 1e-8
        assert np.abs(a['eta2'] - b['eta2']).max() <= 1e-8 * a['eta2'].max()
        if a['marked'] is None:
            break
        t = a['eta2'][a['marked']].min()
        ties = np.abs(a['eta2'] - t) <= 1e-8 * t
        differ = a['marked'] != b['marked']
        print('round: n_e', a['n_e'], 'marked', a['n_marked'], b['n_marked'], 'ties', int(ties.sum()), 'differ', int(differ.sum()))
        assert not (differ & ~ties).any() and abs(a['n_marked'] - b['n_marked']) <= ties.sum()
        assert 0 < a['n_marked'] < a['n_e']
        if differ.any():
            break
    print('TSX tunnel, zz, theta 0.5, GPU:', [(r['n_e'], r['n_marked'], r['eta']) for r in g['adapt']])

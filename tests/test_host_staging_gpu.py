"""
The *_host entry points at sizes where a transfer is longer than the staging ring (fem-elastoplasticity_amd/csrc/fep_staging.h:
four pinned slots of 8 MiB; sizes and inputs in tests/staging_cases.py).

What is compared with what.  The reference of a *_host call is the same operation through its *_dev entry point on torch
tensors: torch does the copies, the staging engine is not involved, and torch.cuda.synchronize() runs before the comparison.
Every comparison is np.array_equal, no tolerance: host and device forms run the same kernels, which use no floating-point
atomics and a fixed summation order (already held to bit equality at 3 200 elements by tests/test_sharding_gpu.py).
Second check, independent of the *_dev path: the large mesh-free inputs are a 1000-point base set tiled along the points, so
column k of every output must equal column k mod 1000 of the same call on the base set alone, and neither a slot (1 048 576
doubles) nor the ring (4 194 304) is a multiple of 1000.

What these tests can and cannot prove.  A race on the GPU is a matter of timing, and no test here can prove its absence: a slot
reused without waiting for its DMA may well deliver the right bytes on the day.  The deterministic proof that every reuse
waits, that every parked chunk reaches its destination and that every tail is sized right is tests/staging_san.cpp, where the
stand-in runtime defers each copy to the latest moment the API allows.  This file proves that the REAL runtime, at chunk sizes
where the DMA is still in flight when the copy threads return, delivers the same bytes as torch's copies.

The mesh host forms (fep_mesh_*_host, fep_mark_bulk_host) take the same engine with device
blocks of the call; their section is at the end, with the same reference (the *_dev form on torch tensors) and the same rule.
"""
import threading

import numpy as np
import pytest

import staging_cases as sc
from staging_cases import _lib, _p, fep

pytestmark = pytest.mark.gpu

N = sc.N_POINTS
OUT = ('s', 'ds', 'ind', 'counts', 'ep')


# ---- mesh-free return map ----------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle(model, with_field):
    """*_dev on the tiled points, accepting: computed once per (model, field), never modified."""
    key = (model, with_field)
    if key not in _ORACLE:
        r = sc.return_map_dev(model, sc.tiled(model), True, with_field)
        b = sc.base(model)
        small = _host_call(model, b, sc.N_BASE, 'pageable', True, with_field)       # one chunk per array: today's path
        for k in ('s', 'ds', 'ind', 'ep'):                                           # the tiling itself, on the oracle
            assert np.array_equal(r[k], sc.tile(small[k])), (model, k)
        _ORACLE[key] = (r, small)
    return _ORACLE[key]


def _host_call(model, d, n, kinds, accept, with_field, layout='C'):
    """One raw *_host call with every array placed by `kinds` (one kind for all, or a dict name -> kind, default pageable)."""
    kind = (lambda name: kinds) if isinstance(kinds, str) else (lambda name: kinds.get(name, 'pageable'))
    if layout == 'C':
        e, ps, cs = sc.place(kind('e'), d['E']), 1, n
    elif layout == 'F':                                                              # the driver's F-ordered array: (3, 1)
        e, ps, cs = sc.place(kind('e'), np.ascontiguousarray(d['E'].T)), 3, 1
    else:                                                                            # point stride 5: the span is 5 n - 2 doubles
        full = sc.place(kind('e'), np.full((n, 5), np.nan))
        full[:, :3] = d['E'].T
        e, ps, cs = full, 5, 1
    ep = sc.place(kind('ep'), d['ep'], canary=True)
    mats = [sc.place(kind(f'm{i}'), m) for i, m in enumerate(d['mats'])]
    fld = sc.place(kind('field'), d['field']) if with_field else None
    e0 = sc.place(kind('e0'), d['e0'])
    s = sc.place(kind('s'), np.zeros((4, n)), canary=True)
    ds = sc.place(kind('ds'), np.zeros((9, n)), canary=True)
    ind = sc.place(kind('ind'), np.full(n, 7, np.uint8), canary=True)
    counts = sc.place(kind('counts'), np.zeros(2, np.int64), canary=True)
    sc.return_map_host(model, n, e, ps, cs, e0, ep, mats, accept, s, ds, ind, counts, fld)
    r = dict(s=s, ds=ds, ind=ind, counts=counts, ep=ep)
    for k, v in r.items():
        assert sc.canary_intact(v), (model, k)
    # inputs are the caller's: not a byte changed (the strain with the NaN padding of the stride-5 layout)
    assert all(np.array_equal(a, b) for a, b in zip(mats, d['mats'])) and (fld is None or np.array_equal(fld, d['field']))
    assert np.array_equal(e0, d['e0']) and (accept or np.array_equal(ep, d['ep']))
    e_in = d['E'] if layout == 'C' else d['E'].T
    assert np.array_equal(e[:, :3] if layout == 'stride5' else e, e_in)
    assert layout != 'stride5' or np.isnan(e[:, 3:]).all()
    return r


def _same(r, ref, model, accept=True):
    for k in OUT:
        want = ref[k] if (k != 'ep' or accept) else sc.tiled(model)['ep']
        assert np.array_equal(r[k], want), (model, k, int((r[k] != want).sum()))


def _tiles(r, small, model):
    """Independent of the *_dev path: column k equals column k mod 1000 of the call on the base set."""
    for k in ('s', 'ds', 'ind', 'ep'):
        assert np.array_equal(r[k], sc.tile(small[k])), (model, k)
    q, rest = divmod(N, sc.N_BASE)
    first = _host_counts_of_first(small, rest)
    assert np.array_equal(r['counts'], q * small['counts'] + first), (model, r['counts'], small['counts'])


def _host_counts_of_first(small, m):
    """The branch counts of the first m base points, from the base call's own flags and tangents: a plastic point with an
    all-zero tangent is an apex point (Drucker-Prager, Mohr-Coulomb); von Mises counts every plastic point first."""
    plastic = small['ind'][:m] != 0
    apex = plastic & (np.abs(small['ds'][:, :m]).max(axis=0) == 0)
    return np.array([int(plastic.sum() - apex.sum()), int(apex.sum())], dtype=np.int64)


@pytest.mark.parametrize('model', sc.MODELS)
def test_return_map_pageable_arrays_longer_than_the_ring(model):
    """Raw C ABI, every array pageable and 8 bytes off its allocation, accepting: ep_prev goes down and comes back through the
    ring in place.  e is two chunks, ep_prev and s three (32-byte tail), ds five (the last 4 MiB + 72 bytes)."""
    ref, small = oracle(model, False)
    assert 0 < ref['counts'].sum() < N
    r = _host_call(model, sc.tiled(model), N, 'pageable', True, False)
    _same(r, ref, model)
    _tiles(r, small, model)


@pytest.mark.parametrize('model', sc.MODELS)
def test_return_map_field_pageable_arrays(model):
    """fep_return_map_field_host: the field is a seventh input of three chunks."""
    ref, small = oracle(model, True)
    assert 0 < ref['counts'].sum() < N
    r = _host_call(model, sc.tiled(model), N, 'pageable', True, True)
    _same(r, ref, model)
    _tiles(r, small, model)


@pytest.mark.parametrize('model', sc.MODELS)
def test_return_map_pinned_and_mixed_arrays(model):
    """Every array in a pinned block (views 8 bytes into it: the direct path both ways): not accepting, ep_prev stays as it
    was; accepting, ep_prev is DMA-ed back into the pinned view it came from; the field variant.  Then pinned and pageable
    arrays mixed so that direct copies and ring chunks alternate on the stream."""
    ref, small = oracle(model, False)
    ref_f, small_f = oracle(model, True)
    d = sc.tiled(model)
    r = _host_call(model, d, N, 'pinned', False, False)
    _same(r, ref, model, accept=False)
    r = _host_call(model, d, N, 'pinned', True, False)
    _same(r, ref, model)
    _tiles(r, small, model)
    r = _host_call(model, d, N, 'pinned', True, True)
    _same(r, ref_f, model)
    _tiles(r, small_f, model)
    mixed = {'e': 'pinned', 'm1': 'pinned', 'm2': 'pinned', 's': 'pinned', 'ind': 'pinned', 'field': 'pinned'}
    r = _host_call(model, d, N, mixed, True, False)
    _same(r, ref, model)
    _tiles(r, small, model)
    _same(_host_call(model, d, N, mixed, True, True), ref_f, model)


@pytest.mark.parametrize('model', sc.MODELS)
@pytest.mark.parametrize('layout', ['F', 'stride5'])
def test_return_map_strain_layouts(model, layout):
    """The F-ordered (3, 1) strain and a padded one (point stride 5, component stride 1: the span copied is 5 n - 2 doubles,
    three chunks) against the C-ordered (1, n) call, which the tests above hold to the oracle."""
    d = sc.tiled(model)
    c_ordered = _host_call(model, d, N, 'pageable', True, False)
    r = _host_call(model, d, N, 'pageable', True, False, layout=layout)
    _same(r, c_ordered, model)
    _same(r, oracle(model, False)[0], model)


# ---- context calls on the large mesh -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    """The context of square_mesh(724, 'P1') with its state, built once; tests set the model they need and copy what they
    change."""
    mesh = fep.square_mesh(sc.MESH_N, 'P1', 10)
    elem, coord = mesh['elements'], mesh['coordinates']
    ctx = fep.MeshContext(elem, coord)
    assert (ctx.n_n, ctx.n_e) == (525625, 1048352)
    U2 = np.ascontiguousarray(sc.displacement(coord))
    yield dict(ctx=ctx, coord=coord, elem=elem, U2=U2, U=np.ascontiguousarray(U2.reshape(-1, order='F')), dev={})
    ctx.close()


def use_model(ctx, model):
    ctx.set_model(model)
    ctx.set_materials(*sc.model_materials(model, ctx.n_int))
    if model == 'vmi':
        import vmi_cases
        ctx.set_hardening(*vmi_cases.curve(sc.VMI_CURVE))
        assert 'p1_point_vmi_kernel' in ctx.kernel_names(0)


def dev_step(big, model, want, accept=False, field=None, scale=1.0, e0=None):
    """The *_dev oracle of one step on the large context, cached per argument set."""
    key = (model, tuple(want), accept, field is not None)
    if key not in big['dev']:
        ctx = big['ctx']
        use_model(ctx, model)
        r = sc.step_dev(ctx, sc.model_scale(model) * big['U'], np.zeros((4, ctx.n_int)), accept, want, e0=e0, field=field, scale=scale)
        n0, n1 = (int(v) for v in r['counts'])
        if model in ('vm', 'vmi'):                          # {plastic points, 0}
            assert 0 < n0 < ctx.n_int and n1 == 0, ('the generator', model, n0, n1)
        else:                                               # a failure here blames the generator, not the engine
            assert n0 > 0 and n1 > 0 and n0 + n1 < ctx.n_int, ('the generator', model, n0, n1)
        big['dev'][key] = r
    return big['dev'][key]


def host_step(big, model, want, accept=False, planar=False, kind='pageable', field=None, scale=1.0, e0=None):
    ctx = big['ctx']
    use_model(ctx, model)
    u = sc.model_scale(model) * (big['U2'] if planar else big['U'])
    ep = sc.place('pageable', np.zeros((4, ctx.n_int)), canary=True)
    r = sc.step_host(ctx, sc.place('pageable', u), ep, accept, want, kind=kind, planar=planar, e0=e0,
                     field=None if field is None else sc.place('pageable', field), scale=scale)
    assert sc.canary_intact(ep)
    r['ep'] = ep
    return r


def same_step(r, ref, want):
    for k in tuple(want) + ('counts', 'ep'):
        assert np.array_equal(r[k], ref[k]), (k, int((r[k] != ref[k]).sum()))


@pytest.mark.parametrize('want,accept', [(sc.STEP_KEYS, False), (('K',), False), (('F',), False), (('ind_p',), True)],
                         ids=['full', 'K', 'F', 'ind_p-accept'])
def test_step_pageable_outputs_on_the_large_mesh(big, want, accept):
    """Drucker-Prager, node route, raw C ABI, every output pageable with a canary tail: every output (K is fifteen chunks),
    K alone and F alone (the one-kernel step), ind_p alone on an accepting call (uint8 chunks, ep_prev back in place)."""
    ref = dev_step(big, 'dp', want, accept)
    assert 'p1_node' in big['ctx'].kernel_names(0)
    same_step(host_step(big, 'dp', want, accept), ref, want)


def test_step_planar_displacement_is_the_interleaved_one(big):
    """fep_step_host_planar: the (2, n_n) array is interleaved inside the staging copy, 524 288 nodes per chunk, the second
    chunk 1 337 nodes."""
    assert big['ctx'].n_n - sc.SLOT_BYTES // 16 == 1337
    want = ('E', 's', 'F')
    ref = dev_step(big, 'dp', want)
    interleaved = host_step(big, 'dp', want)
    same_step(host_step(big, 'dp', want, planar=True), interleaved, want)
    same_step(interleaved, ref, want)
    same_step(host_step(big, 'dp', want, planar=True, kind='pinned'), ref, want)


@pytest.mark.parametrize('model', sc.STEP_MODELS)
def test_step_of_the_other_models_on_the_large_mesh(big, model):
    """set_model on the same context, every output (E comes from the model's own point kernel), accepting."""
    want = sc.STEP_KEYS
    try:
        same_step(host_step(big, model, want, accept=True), dev_step(big, model, want, accept=True), want)
    finally:
        use_model(big['ctx'], 'dp')


def test_step_with_an_initial_strain_field(big):
    """fep_step_field_host: the field is a third input of three chunks."""
    ctx = big['ctx']
    rng = np.random.default_rng(724)
    field = sc.fcases.eps_y('dp') * rng.normal(0, 0.2, size=(4, ctx.n_int))
    e0 = np.array([1e-5, -2e-5, 3e-5, 0.5e-5])
    want = ('s', 'ds', 'ind_p', 'K', 'F')
    ref = dev_step(big, 'dp', want, field=field, scale=0.37, e0=e0)
    same_step(host_step(big, 'dp', want, field=field, scale=0.37, e0=e0), ref, want)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', 0))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def test_assemble_transform_loads_and_point_coords(big):
    """fep_assemble_host on the step's own ds and s against fep_assemble_dev; fep_transform_host, fep_load_volume_host (point
    values, and the weight override) and fep_ctx_point_coords_host against their _dev forms.  Pageable arrays, canary tails."""
    import torch
    ctx, l = big['ctx'], _lib.lib()
    use_model(ctx, 'dp')
    step = dev_step(big, 'dp', sc.STEP_KEYS)
    n, f64 = ctx.n_int, dict(dtype=torch.float64, device=torch.device('cuda', 0))
    ds, s = sc.place('pageable', step['ds']), sc.place('pageable', step['s'])
    # assemble
    Kd, Fd = torch.empty(ctx.nnz, **f64), torch.empty(ctx.n_dof, **f64)
    DS, S = _t(step['ds']), _t(step['s'])
    ctx.assemble_dev(_stream(), ds=DS.data_ptr(), s=S.data_ptr(), k_data=Kd.data_ptr(), f_out=Fd.data_ptr())
    torch.cuda.synchronize()
    K, F = sc.pageable(ctx.nnz, canary=True), sc.pageable(ctx.n_dof, canary=True)
    assert l.fep_assemble_host(ctx.handle, _p(ds), _p(s), _p(K), _p(F)) == 0
    assert np.array_equal(K, Kd.cpu().numpy()) and np.array_equal(F, Fd.cpu().numpy())
    assert sc.canary_intact(K) and sc.canary_intact(F)
    del Kd, DS
    # transform
    rng = np.random.default_rng(5)
    q = rng.normal(size=n)
    Qn = torch.empty(ctx.n_n, **f64)
    Q = _t(q)
    ctx.transform_dev(_stream(), Q.data_ptr(), Qn.data_ptr())
    torch.cuda.synchronize()
    qn = sc.pageable(ctx.n_n, canary=True)
    assert l.fep_transform_host(ctx.handle, _p(sc.place('pageable', q)), _p(qn)) == 0
    assert np.array_equal(qn, Qn.cpu().numpy()) and sc.canary_intact(qn)
    # load_volume: a value per point, then a caller's weights as well
    hatp = ctx._hatp(None)
    fv, w = rng.normal(size=(2, n)), rng.uniform(0.5, 1.5, size=n)
    FV, W = _t(fv), _t(w)
    for weight_d, weight_h in ((0, None), (W.data_ptr(), sc.place('pageable', w))):
        ctx.load_volume_dev(_stream(), Fd.data_ptr(), f_v_int=FV.data_ptr(), weight=weight_d)
        torch.cuda.synchronize()
        out = sc.pageable(ctx.n_dof, canary=True)
        assert l.fep_load_volume_host(ctx.handle, _p(hatp), _p(sc.place('pageable', fv)), 0.0, 0.0, _p(weight_h), _p(out)) == 0
        assert np.array_equal(out, Fd.cpu().numpy()) and sc.canary_intact(out)
    # point_coords
    XQ = torch.empty((2, n), **f64)
    ctx.point_coords_dev(_stream(), XQ.data_ptr())
    torch.cuda.synchronize()
    xq = sc.pageable((2, n), canary=True)
    assert l.fep_ctx_point_coords_host(ctx.handle, _p(hatp), _p(xq)) == 0
    assert np.array_equal(xq, XQ.cpu().numpy()) and sc.canary_intact(xq)


@pytest.mark.parametrize('stats', [True, False], ids=['stats', 'no-stats'])
def test_recover_stress_and_estimate(big, stats):
    """fep_recover_stress_host and fep_estimate_host on the step's own s against their _dev forms, with the statistics and
    with a NULL stats_h (no statistics kernel, nothing copied back for it).  Pageable arrays, canary tails."""
    import torch
    ctx, l = big['ctx'], _lib.lib()
    use_model(ctx, 'dp')
    step = dev_step(big, 'dp', sc.STEP_KEYS)
    eta2_d, stats_d, sn_d = ctx.estimate_dev(_t(step['s']), stats=stats)
    torch.cuda.synchronize()
    s = sc.place('pageable', step['s'])
    sn = sc.pageable((4, ctx.n_n), canary=True)
    assert l.fep_recover_stress_host(ctx.handle, _p(s), _p(sn)) == 0
    assert np.array_equal(sn, sn_d.cpu().numpy()) and sc.canary_intact(sn)
    eta2 = sc.pageable(ctx.n_e, canary=True)
    st = sc.pageable(4, canary=True) if stats else None
    assert l.fep_estimate_host(ctx.handle, _p(ctx._hatp(None)), _p(s), _p(sn), _p(eta2), _p(st)) == 0
    assert np.array_equal(eta2, eta2_d.cpu().numpy()) and sc.canary_intact(eta2)
    if stats:
        assert np.array_equal(st, stats_d.cpu().numpy()) and sc.canary_intact(st)
    assert np.array_equal(s, step['s'])                                              # the input is the caller's


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def _small_case():
    mesh = fep.square_mesh(sc.SMALL_MESH_N, 'P1', 10)
    elem, coord = mesh['elements'], mesh['coordinates']
    ctx = fep.MeshContext(elem, coord)
    ctx.set_materials(*sc.model_materials('dp', ctx.n_int))
    U2 = np.ascontiguousarray(sc.displacement(coord))
    return ctx, U2, np.ascontiguousarray(U2.reshape(-1, order='F'))


def test_small_large_small_calls_on_one_device(big):
    """Growth of the engine's and the contexts' persistent buffers and different ring start positions: a small context, the
    large one, the small one again (its buffers now smaller than the engine's), mesh-free calls of 1000 and 524 289 points in
    between.  Each result equals that call's result in a fresh sequence (the oracles above; the small context's first call)."""
    small, U2, U = _small_case()
    try:
        want = ('s', 'ds', 'ind_p', 'K', 'F')
        ep0 = np.zeros((4, small.n_int))
        first = sc.step_host(small, sc.place('pageable', U), sc.place('pageable', ep0), False, want)
        ref_small = sc.step_dev(small, U, ep0, False, want)
        ref_rm, base_rm = oracle('dp', False)
        ref_big = dev_step(big, 'dp', ('K', 'F'))
        for k in want:
            assert np.array_equal(first[k], ref_small[k]), k
        for rep in range(2):
            r = _host_call('dp', sc.base('dp'), sc.N_BASE, 'pageable', True, False)
            assert all(np.array_equal(r[k], base_rm[k]) for k in OUT)
            same_step(host_step(big, 'dp', ('K', 'F')), ref_big, ('K', 'F'))
            _same(_host_call('dp', sc.tiled('dp'), N, 'pageable', True, False), ref_rm, 'dp')
            again = sc.step_host(small, sc.place('pageable', U2), sc.place('pageable', ep0), False, want, planar=True)
            for k in want + ('counts',):
                assert np.array_equal(again[k], first[k]), (rep, k)
    finally:
        small.close()


def test_two_threads_with_a_context_each():
    """Two Python threads on device 0, each with its own 40-cell context, alternating step and construct_constitutive_problem
    twenty times (ctypes releases the GIL; the engine's call lock serialises the calls, the copy pool its jobs).  Every result
    equals the serial one."""
    cases = []
    b = sc.base('dp')
    for t in range(2):
        ctx, U2, U = _small_case()
        cases.append(dict(ctx=ctx, U2=(1.0 + 0.25 * t) * U2, E=(1.0 + 0.25 * t) * b['E']))

    def one(c):
        r = c['ctx'].step(c['U2'], np.zeros((4, c['ctx'].n_int)))
        m = fep.construct_constitutive_problem(c['E'], b['ep'].copy(), *b['mats'], apply_plastic_strain=True)
        return [r['s'].copy(), r['ds'].copy(), r['ind_p'].copy(), r['K'].data.copy(), r['F'].copy(), np.array([r['n_smooth'], r['n_apex']]),
                m['s'].copy(), m['ds'].copy(), m['ind_p'].copy(), m['ep'].copy(), np.array([m['n_smooth'], m['n_apex']])]

    try:
        serial = [one(c) for c in cases]
        bad, errors = [], []

        def worker(i):
            try:
                for rep in range(20):
                    got = one(cases[i])
                    bad.extend((i, rep, j) for j, (a, b) in enumerate(zip(got, serial[i])) if not np.array_equal(a, b))
            except Exception as exc:                                               # noqa: BLE001 - reported by the main thread
                errors.append((i, repr(exc)))
        threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors and not bad, (errors, bad[:10])
    finally:
        for c in cases:
            c['ctx'].close()


def test_dev_and_host_steps_alternate_on_one_context(big):
    """The sequence include/fep.h allows, with no wait beyond the one it asks for: a *_dev step on a stream, a wait for THAT
    stream only (never the device), a *_host step; then a *_dev step straight after the *_host call has returned.  Both forms
    use the context's ds / s scratch and branch counters, the host form on the engine's own stream.  Nothing else touches the
    GPU between the legs (model and materials are set before, the host arrays are placed before).  Same bits as each alone."""
    import torch
    want = ('K', 'F')                                       # both go through the context's scratch and counters
    ref = dev_step(big, 'dp', want)
    ref_acc = dev_step(big, 'dp', want, accept=True)
    full = dev_step(big, 'dp', sc.STEP_KEYS)
    ctx = big['ctx']
    use_model(ctx, 'dp')
    ep0 = np.zeros((4, ctx.n_int))
    u_h = sc.place('pageable', big['U'])
    side = torch.cuda.Stream()
    main = torch.cuda.current_stream()
    torch.cuda.synchronize()
    for rep in range(2):
        ep_h = sc.place('pageable', ep0, canary=True)
        with torch.cuda.stream(side):                       # enqueued on `side`; the host waits for `side` and nothing else
            d = sc.step_dev(ctx, big['U'], ep0, True, want, sync=side.synchronize)
            h = sc.step_host(ctx, u_h, ep_h, False, sc.STEP_KEYS)                   # returns with its own stream synchronised
            h['ep'] = ep_h
        same_step(d, ref_acc, want)
        same_step(h, full, sc.STEP_KEYS)
        d = sc.step_dev(ctx, big['U'], ep0, False, want, sync=main.synchronize)     # no wait needed after the host call
        h = sc.step_host(ctx, u_h, ep_h, False, want)
        h['ep'] = ep_h
        same_step(d, ref, want)
        same_step(h, ref, want)
        assert sc.canary_intact(ep_h)


# ---- mesh host forms: the engine, device blocks of the call -------------------------------------------------------
FEP_TYPE = {'P2': 2, 'P4': 5}


def _out(kind, shape, dtype):
    """An output array of `kind` with a canary tail, holding neither a result nor the canary."""
    a = (sc.pageable if kind == 'pageable' else sc.pinned)(shape, dtype, canary=True)
    a.view(np.uint8).reshape(-1)[...] = 0x3C
    return a


def _bits(got, ref, what):
    """Host arrays against the tensors of the *_dev form: shape, dtype and every byte."""
    assert len(got) == len(ref), what
    for j, (a, b) in enumerate(zip(got, ref)):
        b = b.cpu().numpy() if hasattr(b, 'cpu') else b
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, j)
        assert sc.canary_intact(a), (what, j)


def _enrich_host(m, t, kind='pageable', with_ed=True):
    """Raw fep_mesh_enrich_host -> [elem_ext, coord_ext, surf[, elem_ed, edge_el]]."""
    i, p2 = m.info, t == 'P2'
    out = [_out(kind, (6 if p2 else 15, i['n_e']), np.int32), _out(kind, (2, i['n_n'] + m.new_nodes(t)), np.float64),
           _out(kind, (3 if p2 else 5, i['n_boundary_edges']), np.int32)]
    if p2 and with_ed:
        out += [_out(kind, (3, i['n_e']), np.int32), _out(kind, (2, i['n_edges']), np.int32)]
    assert _lib.lib().fep_mesh_enrich_host(m._h, FEP_TYPE[t], *([_p(a) for a in out] + [None] * (5 - len(out)))) == 0
    return out


def _refine_host(m, kind='pageable'):
    """Raw fep_mesh_refine_host -> [coord_ext, child], the order of DeviceMesh.refine_dev."""
    i = m.info
    child, coord_ext = _out(kind, (3, 4 * i['n_e']), np.int32), _out(kind, (2, i['n_n'] + i['n_edges']), np.float64)
    assert _lib.lib().fep_mesh_refine_host(m._h, _p(child), _p(coord_ext)) == 0
    return [coord_ext, child]


@pytest.fixture(scope='module')
def big_mesh(big):
    """The large mesh analysed once; 'refine': its refine_dev result as NumPy arrays, computed once, never modified."""
    import torch
    m = fep.DeviceMesh(big['coord'], big['elem'], 0)
    assert m.info['n_e'] == 1048352 and m.info['n_nonmanifold'] + m.info['n_inconsistent'] + m.info['n_degenerate'] == 0
    ref = [a.cpu().numpy() for a in m.refine_dev()]
    torch.cuda.synchronize()
    yield dict(m=m, refine=ref)
    m.close()


@pytest.fixture(scope='module')
def small_mesh():
    """The 40-cell square: (DeviceMesh, coord, elem)."""
    mesh = fep.square_mesh(sc.SMALL_MESH_N, 'P1', 10)
    m = fep.DeviceMesh(mesh['coordinates'], mesh['elements'], 0)
    yield m, mesh['coordinates'], mesh['elements']
    m.close()


def _p4_ref(big_mesh):
    """enrich_dev('P4') of the large mesh as NumPy arrays: computed once, never modified."""
    import torch
    if 'P4' not in big_mesh:
        big_mesh['P4'] = [a.cpu().numpy() for a in big_mesh['m'].enrich_dev('P4')]
        torch.cuda.synchronize()
    return big_mesh['P4']


def test_enrich_p4_on_the_large_mesh(big_mesh):
    """elem_ext is 62.9 MB, eight chunks, coord_ext 134 MB: the ring comes round inside each."""
    m = big_mesh['m']
    assert sc.chunks(15 * 4 * m.info['n_e'])[0] == 8
    _bits(_enrich_host(m, 'P4'), _p4_ref(big_mesh), 'P4')


def test_refine_on_the_large_mesh(big_mesh):
    """child is 50.3 MB, six chunks."""
    m = big_mesh['m']
    assert sc.chunks(12 * 4 * m.info['n_e'])[0] == 6
    _bits(_refine_host(m), big_mesh['refine'], 'refine')


@pytest.mark.parametrize('kind', ['pageable', 'pinned'])
@pytest.mark.parametrize('with_ed', [True, False], ids=['ed', 'no-ed'])
def test_enrich_p2_with_and_without_the_edge_tables(small_mesh, kind, with_ed):
    """P2 with and without elem_ed / edge_el (NULL: no block, no transfer), into pageable arrays 8 bytes off their allocation
    and into pinned ones: the bits of enrich_dev, the values of the NumPy create_midpoints_P2, and DeviceMesh.enrich's dict
    equal to the NumPy one key by key (shape, dtype, values), as tests/test_mesh_gpu.py compares them."""
    import torch
    m, coord, elem = small_mesh
    ref = m.enrich_dev('P2')
    torch.cuda.synchronize()
    got = _enrich_host(m, 'P2', kind, with_ed)
    _bits(got, ref[:len(got)], ('P2', kind, with_ed))
    h = fep.create_midpoints_P2(coord, elem)
    for a, k in zip(got, ('elem_ext', 'coord_ext', 'surf', 'elem_ed', 'edge_el')):
        assert a.shape == h[k].shape and np.array_equal(a, h[k]), k
    d = m.enrich('P2')
    assert sorted(d) == sorted(h)
    for k in h:
        assert d[k].shape == h[k].shape and d[k].dtype == h[k].dtype and np.array_equal(d[k], h[k]), k


def test_area_stats_with_two_chunks_each(big):
    """elem (12.6 MB) and coord (8.4 MB) are two chunks each."""
    import torch
    e32 = np.ascontiguousarray(big['elem'][0:3], dtype=np.int32)
    coord = np.ascontiguousarray(big['coord'], dtype=np.float64)
    assert sc.chunks(e32.nbytes)[0] == 2 and sc.chunks(coord.nbytes)[0] == 2
    ref = fep.area_stats_dev(_t(coord), _t(e32), 0)
    torch.cuda.synchronize()
    out = _out('pageable', (4,), np.float64)
    e_h, c_h = sc.place('pageable', e32), sc.place('pageable', coord)
    assert _lib.lib().fep_mesh_area_stats_host(0, e32.shape[1], coord.shape[1], _p(e_h), _p(c_h), _p(out)) == 0
    _bits([out], [ref], 'area_stats')
    assert out[2] == 0 and out[3] == e32.shape[1] and out[1] > 0
    assert np.array_equal(e_h, e32) and np.array_equal(c_h, coord)                  # the inputs are the caller's


def test_mark_bulk_on_five_chunks():
    """n = 4 * 2^20 + 1000 doubles: four full slots and 8000 bytes.  The values are the 1000 indicators of the marking tests
    tiled by the rule of staging_cases, so equal values share a fate and a chunk that lands a slot off shows: marked[k] must
    equal marked[k mod 1000]."""
    import torch
    import estimate_cases as ec
    n = 4 * (1 << 20) + 1000
    x = sc.tile(ec.value_set(sc.N_BASE), n)
    assert sc.chunks(x.nbytes) == (5, 8000)
    l = _lib.lib()
    X = _t(x)
    M = torch.empty(n, dtype=torch.uint8, device=X.device)
    O = torch.empty(4, dtype=torch.float64, device=X.device)
    assert l.fep_mark_bulk_dev(0, _stream(), n, X.data_ptr(), 0.5, M.data_ptr(), O.data_ptr()) == 0
    torch.cuda.synchronize()
    x_h, marked, out = sc.place('pageable', x), _out('pageable', (n,), np.uint8), _out('pageable', (4,), np.float64)
    assert l.fep_mark_bulk_host(0, n, _p(x_h), 0.5, _p(marked), _p(out)) == 0
    _bits([marked, out], [M, O], 'mark_bulk')
    assert 0 < int(marked.sum()) < n and out[2] == marked.sum()
    assert np.array_equal(marked, sc.tile(marked[:sc.N_BASE], n))
    assert np.array_equal(x_h, x)


@pytest.mark.parametrize('with_parent', [True, False], ids=['parent', 'no-parent'])
def test_refine_marked_with_and_without_parent(with_parent):
    """The 40-cell square with the marks of marked_cases' first round (the elements at node 0 and 10 % at random)."""
    import torch
    import marked_cases as mc
    mesh = fep.square_mesh(sc.SMALL_MESH_N, 'P1', 10)
    elem = mesh['elements']
    with fep.DeviceMesh(mesh['coordinates'], elem, 0) as m:
        info = m.mark(mc.round_marks(1, elem, np.random.default_rng(40)))
        assert elem.shape[1] < info['n_child'] < 4 * elem.shape[1]
        ref = m.refine_marked_dev()
        torch.cuda.synchronize()
        n_child, n_tot = info['n_child'], m.info['n_n'] + info['n_new_nodes']
        child, coord_ext = _out('pageable', (3, n_child), np.int32), _out('pageable', (2, n_tot), np.float64)
        parent = _out('pageable', (n_child,), np.int32) if with_parent else None
        assert _lib.lib().fep_mesh_refine_marked_host(m._h, _p(child), _p(coord_ext), _p(parent)) == 0
        _bits([coord_ext, child] + ([parent] if with_parent else []), ref[:2 + with_parent], 'refine_marked')


def test_mesh_host_forms_alternate_with_dev_forms_and_the_return_map(big_mesh, small_mesh):
    """What include/fep.h states for these forms.  A *_dev P4 enrich of the large mesh (197 MB written) enqueued on a side stream
    and a host P4 enrich of the same mesh with nothing between them (both only read the mesh; the host form waits for its own
    stream alone): both right.  Then, on
    the engine the mesh-free return map keeps its buffers in: a 1000-point return map, the large refine, the return map again,
    the small enrich (small -> large -> small through one ring), each equal to its result alone."""
    import torch
    m, coord, elem = small_mesh
    ref = [a.cpu().numpy() for a in m.enrich_dev('P2')]
    torch.cuda.synchronize()
    big, ref4 = big_mesh['m'], _p4_ref(big_mesh)
    side = torch.cuda.Stream()
    for rep in range(2):
        with torch.cuda.stream(side):
            d = big.enrich_dev('P4')
            got = _enrich_host(big, 'P4')
        side.synchronize()
        _bits(got, ref4, ('host beside dev', rep))
        _bits([a.cpu().numpy() for a in d], ref4, ('dev beside host', rep))
        del d, got
    base_rm = oracle('dp', False)[1]
    for rep in range(2):
        r = _host_call('dp', sc.base('dp'), sc.N_BASE, 'pageable', True, False)
        assert all(np.array_equal(r[k], base_rm[k]) for k in OUT)
        _bits(_refine_host(big_mesh['m']), big_mesh['refine'], ('refine after the return map', rep))
        _bits(_enrich_host(m, 'P2'), ref, ('small enrich after the large refine', rep))

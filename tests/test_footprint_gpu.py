"""
What every launch form WRITES: all of its outputs, nothing else, and the same bits whatever the memory held before.

The per-entry tests compare the full-output step with float64 references; every other form (the K,F-only step, on P1
p1_fused_kernel, the kernel a Newton iterate runs; the K-only and F-only steps; the accepting step; assemble(ds, s); the same
forms of the staged steps of the other models and of the field step) is pinned to that step bitwise.  This module runs the forms through step_dev /
assemble_dev on caller memory with known contents (tests/footprint.py): a fresh arena of poison per call, inputs copied in,
the call on torch's current stream, a synchronise, then
  1. every guard band (64 KiB before and after every array) is intact;
  2. every requested output is fully written, F at the nodes of no element exactly 0;
  3. every input (u, ep without accept, ds / s of assemble, the field) is unchanged;
  4. every output, and counts, equals the output of the same name of form A (the full-output step);
  5. A and B on an arena of 0xFF equal A and B on an arena of 0x00;
  6. the accepting step leaves ep's input bits where ind_p is false;
  7. the accepting step's s, K and F equal A's.
      A  e_out, s, ds, ind_p, k_data, f_out, counts       B  k_data, f_out, counts (P1 node route: the one-kernel step)
      C  k_data                                           D  f_out, with ep and with ep = NULL
      E  s, ds, ind_p, counts                             G  k_data, f_out, s (K without ds: the context's ds scratch)
      F  s, k_data, f_out, counts, accepting              H  assemble_dev on A's ds and s: K + F, K only, F only
What A is worth is tested elsewhere: this module has no reference arithmetic and no tolerance.  The cases come from the
tables of p1_node_cases.py, test_element_route_gpu.py, meshes.py, model_step_cases.py and e0_field_cases.py.
The second half runs the other entry points that write caller device memory the same way, each under its contract of
include/fep.h (an array the caller must zero is zeroed, and only its guards stay poisoned).

Out of reach of this method: the library's own tables and scratch (pt_codes, Pc, Pf, blk_counts, Kc, the ds / s scratch,
the solvers' vectors, the mesh object's lists).  A store that misses one of THOSE is seen here only if it lands in an arena
or changes an output.  A stray store farther than 64 KiB from every array of the call is not seen either.

An entry point that allocates scratch on first use is called once on plain tensors before its arena call; a failure
message says so if the library still allocated device memory during the arena call.

Do these tests bite?  Three mutants of the library, none of which can fault (each only leaves a store out), built on a
scratch copy of the tree and run on an MI355X against a selection of the bitwise pins as they were (full, then kf, k_only,
f_only, assemble on one context: P1 node-route cases of test_p1_node_route_gpu.py and test_parity_gpu.py, patch-form cases
of test_element_route_gpu.py and test_high_degree_gpu.py, model, field and non-finite steps), against the same pins with
footprint.scrub between the forms, and against this module:
  (a) fep_assemble_dev returns FEP_OK before its launches on the P1 node route
  (b) p1_fused_kernel skips the K store of the last tile
  (c) the fix-up of K's open blocks (launch_fixup) is skipped where no point output is asked for and in fep_assemble_dev
        pins as they were               pins with scrub                       this module
  (a)   2 of 27 failed (F of assemble   12 of 27 failed: every P1 node case   13 of 101 failed: form H of every P1 node case,
        after an (s, F) step, test_     of the four modules, models too       "k_data: 15600 of 15600 element(s) not written"
        parity_gpu.py); K never
  (b)   27 of 27 passed                 10 of 27 failed: every P1 node case   10 failed: form B of every P1 node case, "k_data:
                                        that runs the one-kernel step (the    12 of 15600 element(s) not written, the first at
                                        model and field steps do not)         [15588]" (rect53x10: the last tile of one node)
  (c)   27 of 27 passed                 5 of 27 failed: the patch-form cases  22 failed: forms B and H of every patch-form case,
                                        but the P1 fan of 16 elements         "k_data: 3396 of 46212 element(s) not written"
On the product library all of these pass.  An over-run is not shown by a kernel mutant but by test_footprint_host.py, where
torch writes one element before and one after a view.
"""
import zlib

import numpy as np
import pytest
import torch

import e0_field_cases
import meshes
import model_step_cases
import p1_node_cases
from footprint import Arena, fully_written, guards_intact, same_bits, unchanged, untouched
from routes import assert_route
from test_element_route_gpu import _state, _structured_cases

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F64, U8, I64, I32 = torch.float64, torch.uint8, torch.int64, torch.int32
FULL = ('e_out', 's', 'ds', 'ind_p', 'k_data', 'f_out', 'counts')
FORMS = {'B': ('k_data', 'f_out', 'counts'), 'C': ('k_data',), 'D': ('f_out',), 'E': ('s', 'ds', 'ind_p', 'counts'),
         'G': ('k_data', 'f_out', 's')}
FORM_F = ('s', 'k_data', 'f_out', 'counts')


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Plain:
    """The arena's interface on plain tensors: the warm-up call of an entry point that allocates scratch on first use."""
    fill = None

    def take(self, shape, dtype=F64, align=16, name=None):
        return torch.zeros(shape, dtype=dtype, device=DEV)

    def put(self, array, dtype=None, align=16, name=None):
        src = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.array(array, order='C'))
        v = src.to(device=DEV, dtype=dtype or src.dtype).clone()
        return v, v.clone()


def _arena(fill):
    return _Plain() if fill is None else Arena(DEV, fill=fill)


def _run(arena, call, label):
    """`call()` (it only enqueues), a synchronise, then check 1; -> a note for failure messages if the library allocated."""
    free0 = torch.cuda.mem_get_info()[0]
    call()
    torch.cuda.synchronize()
    grown = free0 - torch.cuda.mem_get_info()[0]
    note = label + (f' [the library allocated {grown} bytes of device memory during this call]' if grown else '')
    if arena.fill is not None:
        _checked(note, guards_intact, arena)
    return note


def _checked(note, check, *a, **k):
    try:
        return check(*a, **k)
    except AssertionError as e:
        raise AssertionError(f'{note}: {e}') from None


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _dev(a, dtype=None):
    """A host array as a device tensor (a copy: torch takes no read-only array)."""
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(DEV)


def _shapes(ctx):
    n = ctx.n_int
    return {'e_out': ((3, n), F64), 's': ((4, n), F64), 'ds': ((9, n), F64), 'ind_p': ((n,), U8), 'k_data': ((ctx.nnz,), F64),
            'f_out': ((ctx.n_dof,), F64), 'counts': ((2,), I64)}


def _orphan_dofs(ctx):
    used = np.zeros(ctx.n_n, dtype=bool)
    used[np.unique(ctx.elements)] = True
    return _dev(np.repeat(~used, 2))


def _step(ctx, label, U, Ep, outs, accept=False, e0=None, field=None, scale=1.0, fill=0xFF):
    """One step_dev call on a fresh arena with checks 1 to 3 -> dict of the output views, plus 'ep' and 'ep_in'."""
    a = _arena(fill)
    U = np.asarray(U, dtype=float)
    u, u_in = a.put(U.reshape(-1, order='F') if U.ndim == 2 else U, name='u')
    ep, ep_in = (None, None) if Ep is None else a.put(Ep, name='ep')
    fld, fld_in = (None, None) if field is None else a.put(field, name='e0_field')
    sh = _shapes(ctx)
    o = {k: a.take(*sh[k], name=k) for k in outs}
    note = _run(a, lambda: ctx.step_dev(_stream(), u.data_ptr(), ep=_ptr(ep), accept=accept, e0=e0,
                                        e0_field=None if fld is None else fld.data_ptr(), e0_scale=scale,
                                        **{k: v.data_ptr() for k, v in o.items()}), label)
    if fill == 0xFF:
        for k, v in o.items():
            _checked(note, fully_written, v, name=k)
    if fill is not None:
        if 'f_out' in o:
            orphan = _orphan_dofs(ctx)
            assert bool((o['f_out'][orphan] == 0).all()), f'{note}: F at a node of no element is not 0'
        _checked(note, unchanged, u, u_in, 'u')
        if ep is not None and not accept:
            _checked(note, unchanged, ep, ep_in, 'ep')
        if fld is not None:
            _checked(note, unchanged, fld, fld_in, 'e0_field')
    return dict(o, ep=ep, ep_in=ep_in, note=note)


def _same_outputs(got, want, keys=None):
    for k in keys or [k for k in got if k in FULL]:
        _checked(got['note'], same_bits, got[k], want[k], f'{k} against form A')


def _assemble(ctx, label, A, fill=0xFF):
    """Form H: assemble_dev on A's ds and s, K + F, K only, F only; checks 1 to 4."""
    sh = _shapes(ctx)
    for outs in (('k_data', 'f_out'), ('k_data',), ('f_out',)):
        a = _arena(fill)
        ds, ds_in = a.put(A['ds'], name='ds')
        s, s_in = a.put(A['s'], name='s')
        o = {k: a.take(*sh[k], name=k) for k in outs}
        note = _run(a, lambda: ctx.assemble_dev(_stream(), ds=ds.data_ptr() if 'k_data' in o else 0,
                                                s=s.data_ptr() if 'f_out' in o else 0,
                                                **{k: v.data_ptr() for k, v in o.items()}), f'{label} H {"+".join(outs)}')
        if fill is None:
            continue
        for k, v in o.items():
            _checked(note, fully_written, v, name=k)
            _checked(note, same_bits, v, A[k], f'{k} against form A')
        if 'f_out' in o:
            assert bool((o['f_out'][_orphan_dofs(ctx)] == 0).all()), f'{note}: F at a node of no element is not 0'
        _checked(note, unchanged, ds, ds_in, 'ds')
        _checked(note, unchanged, s, s_in, 's')


def _accepting(ctx, label, A, U, Ep, kw):
    """Form F with checks 6 and 7."""
    Fm = _step(ctx, f'{label} F', U, Ep, FORM_F, accept=True, **kw)
    _same_outputs(Fm, A)
    elastic = A['ind_p'] == 0
    _checked(Fm['note'], same_bits, Fm['ep'][:, elastic], Fm['ep_in'][:, elastic], 'ep where ind_p is false')
    if bool((~elastic).any()):
        assert not torch.equal(Fm['ep'], Fm['ep_in']), f'{label} F: an accepting step with plastic points left ep as it was'


def _all_forms(ctx, label, U, Ep, e0=None, forms='ABCDEGFH', field=None, scale=1.0, branches=False):
    kw = dict(e0=e0, field=field, scale=scale)
    # every form once on plain tensors: scratch that is allocated on first use exists before an arena is looked at
    _step(ctx, label, U, Ep, FULL, fill=None, **kw)
    for f in forms:
        if f in FORMS:
            _step(ctx, label, U, Ep, FORMS[f], fill=None, **kw)
    if 'F' in forms:
        _step(ctx, label, U, Ep, FORM_F, accept=True, fill=None, **kw)
    A = _step(ctx, f'{label} A', U, Ep, FULL, **kw)
    if 'H' in forms:
        _assemble(ctx, label, A, fill=None)
    n_smooth, n_apex = (int(v) for v in A['counts'].cpu())
    assert n_smooth + n_apex == int(A['ind_p'].sum()) and bool((A['ind_p'] <= 1).all())
    if branches and ctx.n_int >= 200:
        assert n_smooth > 0 and n_apex > 0 and n_smooth + n_apex < ctx.n_int, (n_smooth, n_apex)
    _same_outputs(_step(ctx, f'{label} A on 0x00', U, Ep, FULL, fill=0x00, **kw), A)
    for f in forms:
        if f in FORMS:
            _same_outputs(_step(ctx, f'{label} {f}', U, Ep, FORMS[f], **kw), A)
    if 'B' in forms:
        _same_outputs(_step(ctx, f'{label} B on 0x00', U, Ep, FORMS['B'], fill=0x00, **kw), A)
    if 'D' in forms:
        A0 = _step(ctx, f'{label} A, ep = 0', U, None, FULL, **kw)
        _same_outputs(_step(ctx, f'{label} D, ep = 0', U, None, FORMS['D'], **kw), A0)
    if 'F' in forms:
        _accepting(ctx, label, A, U, Ep, kw)
    if 'H' in forms:
        _assemble(ctx, label, A)
    return A


def _context(fep, monkeypatch, route, elem, coord):
    """route: node (P1 default), default (comes out as the patch form), patch | coo (FEP_ROUTE)."""
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    ctx = fep.MeshContext(elem, coord)
    assert_route(ctx, 'patch' if route == 'default' else route)
    return ctx


# ---- 2. the step forms --------------------------------------------------------------------------------------------------------
P1_NODE = ('rect53x10', 'rect17x12-1', 'square1', 'square7', 'tsx', 'shuffled60', 'swapped24-accept', 'orphans', 'fan15')
P1_OTHER = [('patch', 'rect53x10'), ('coo', 'rect53x10'), ('patch', 'orphans'), ('coo', 'orphans'), ('default', 'fan16')]


def _p1_case(name):
    kind = p1_node_cases.CASES[name][0]
    elem, coord, h = p1_node_cases.mesh(name)
    rng = np.random.default_rng(p1_node_cases.seed(name) + 1)
    return (elem, coord) + _state(kind, coord, h, elem.shape[1], rng)[:4]


@pytest.mark.parametrize('route,name', [('node', n) for n in P1_NODE] + P1_OTHER)
def test_p1_step_forms_write_their_outputs_and_nothing_else(fep, monkeypatch, route, name):
    elem, coord, U, Ep, mats, e0 = _p1_case(name)
    ctx = _context(fep, monkeypatch, route, elem, coord)
    try:
        ctx.set_materials(*mats)
        A = _all_forms(ctx, f'P1 {route} {name}', U, Ep, e0=e0, branches=True)
        if name == 'orphans':
            for n in p1_node_cases.ORPHANS:
                assert float(A['f_out'][2 * n]) == 0 and float(A['f_out'][2 * n + 1]) == 0
    finally:
        ctx.close()


def _element_names(t):
    st = _structured_cases(t)
    odd = st[1] if t in ('Q1', 'Q2') else st[3]
    return ['structured_{}x{}-{}'.format(*st[0]), 'structured_{}x{}-{}'.format(*odd), 'renumbered', 'curved']


def _first_structured(t):
    return _element_names(t)[0]


@pytest.mark.parametrize('t,route,name', [(t, r, n) for t in ('P2', 'Q1', 'Q2', 'P4') for r in ('default', 'coo')
                                          for n in _element_names(t)])
def test_element_route_step_forms_write_their_outputs_and_nothing_else(fep, monkeypatch, t, route, name):
    rng = np.random.default_rng(zlib.crc32(f'{t} {name}'.encode()))
    elem, coord, h, kind = meshes.named(t, name, rng)
    ctx = _context(fep, monkeypatch, route, elem, coord)
    try:
        U, Ep, mats, e0, _ = _state(kind, coord, h, ctx.n_int, rng)
        ctx.set_materials(*mats)
        _all_forms(ctx, f'{t} {route} {name}', U, Ep, e0=e0, branches=True)
    finally:
        ctx.close()


def _model_mesh(t, name):
    if t == 'P1':
        return p1_node_cases.mesh(name)[:2]
    return meshes.named(t, name, np.random.default_rng(0))[:2]


def _curve(model):
    """'vmi' runs on the eight-segment curve of its fixture (kappa of the state spread over all of it); rule 6 then covers
    row 3 of ep, kappa, like the other three: _accepting compares whole columns."""
    import vmi_cases
    return vmi_cases.curve(2) if model == 'vmi' else None


def _set_curve(ctx, model):
    if model == 'vmi':
        ctx.set_hardening(*_curve(model))
        assert 'vmi_kernel' in ctx.kernel_names(0) and len(ctx.hardening[0]) == 8


MODEL_MESHES = [('P1', 'node', 'rect53x10'), ('P1', 'node', 'tsx'), ('P2', 'default', _first_structured('P2')),
                ('P2', 'coo', _first_structured('P2')), ('Q2', 'default', _first_structured('Q2'))]


@pytest.mark.parametrize('t,route,name', MODEL_MESHES)
@pytest.mark.parametrize('model', model_step_cases.MODELS)
def test_model_step_forms_write_their_outputs_and_nothing_else(fep, monkeypatch, model, t, route, name):
    elem, coord = _model_mesh(t, name)
    rng = np.random.default_rng(zlib.crc32(f'footprint {model} {t} {name}'.encode()))
    U, Ep, mats, e0 = model_step_cases.state(model, t, elem, coord, rng, _curve(model))
    ctx = _context(fep, monkeypatch, route, elem, coord)
    try:
        ctx.set_model(model)
        ctx.set_materials(*mats)
        _set_curve(ctx, model)
        A = _all_forms(ctx, f'{model} {t} {route} {name}', U, Ep, e0=e0, forms='ABFH')
        n_plastic = int(A['ind_p'].sum())
        assert 0 < n_plastic < ctx.n_int
    finally:
        ctx.close()


@pytest.mark.parametrize('t,route,name', [MODEL_MESHES[0], MODEL_MESHES[2]])
@pytest.mark.parametrize('model', e0_field_cases.MODELS)
def test_field_step_forms_write_their_outputs_and_nothing_else(fep, monkeypatch, model, t, route, name):
    elem, coord = _model_mesh(t, name)
    rng = np.random.default_rng(zlib.crc32(f'footprint field {model} {t} {name}'.encode()))
    if model == 'dp':
        from elem_ref import ElemRef
        U, Ep, mats, e0 = e0_field_cases.dp_state(elem, coord, ElemRef(elem, coord, fep.element_tables(t)), rng)
    else:
        U, Ep, mats, e0 = model_step_cases.state(model, t, elem, coord, rng, _curve(model))
    ctx = _context(fep, monkeypatch, route, elem, coord)
    try:
        ctx.set_model(model)
        ctx.set_materials(*mats)
        _set_curve(ctx, model)
        field = e0_field_cases.eps_y(model) * rng.normal(0, 0.2, size=(4, ctx.n_int))
        A = _all_forms(ctx, f'field {model} {t} {route} {name}', U, Ep, e0=e0, forms='AB', field=field,
                       scale=e0_field_cases.SCALE)
        assert 0 < int(A['ind_p'].sum()) < ctx.n_int
    finally:
        ctx.close()


# ---- 3. the other entry points that write caller device memory ---------------------------------------------------------------
def _lib(fep):
    from importlib import import_module
    return import_module(fep.__name__ + '._lib')


def _host_ptr(fep, a):
    return _lib(fep).ptr(a)


RM_ENTRY = {'dp': 'fep_return_map_dev', 'vm': 'fep_return_map_vm_dev', 'mc': 'fep_return_map_mc_dev'}


def _mesh_free_points(model, n):
    """(E (3, n), ep (4, n), four materials, e0 (4, 1), field (4, n)): the generators of the mesh-free tests."""
    if model == 'mc':
        import mc_cases
        e, p, e0, sh, bu, sp, c = mc_cases.points(n, False, 5)
        field = e0_field_cases.mesh_free('mc', n, 5)[4]
        return e, p, (sh, bu, sp, c), e0, field
    return e0_field_cases.mesh_free(model, n, 5)


def _return_map_call(fep, label, entry, model, pts, order, accept, fill=0xFF):
    """One mesh-free call on a fresh arena, checks 1 to 3 -> the outputs."""
    E, Ep, mats, e0, field = pts
    n = E.shape[1]
    a = _arena(fill)
    if order == 'C':
        e = a.take((3, n), name='e')
        e.copy_(_dev(E))
        whole, used, pt, comp = e, e, 1, n
    elif order == 'F':
        whole = a.take((n, 3), name='e')
        whole.copy_(_dev(E.T))
        used, pt, comp = whole.t(), 3, 1
    else:                                                               # (n, 5): two columns nobody reads or writes
        whole = a.take((n, 5), name='e')
        whole[:, :3].copy_(_dev(E.T))
        used, pt, comp = whole[:, :3].t(), 5, 1
    e_in = whole.clone()
    ep, ep_in = a.put(Ep, name='ep')
    md = [a.put(m, name=f'material {i}') for i, m in enumerate(mats)]
    fld = a.put(field, name='e0_field') if entry == 'field' else None
    o = {'s': a.take((4, n), name='s'), 'ds': a.take((9, n), name='ds'), 'ind_p': a.take((n,), U8, name='ind_p'),
         'counts': a.take((2,), I64, name='counts')}
    e0v = np.ascontiguousarray(e0, dtype=np.float64).ravel()
    st = _stream()
    tail = [ep.data_ptr(), *(m.data_ptr() for m, _ in md), int(accept), o['s'].data_ptr(), o['ds'].data_ptr(),
            o['ind_p'].data_ptr(), o['counts'].data_ptr()]
    if entry == 'field':
        call = lambda: _lib(fep).check(fep.lib().fep_return_map_field_dev(                                 # noqa: E731
            fep.hotpath.MODELS[model], 0, st, n, whole.data_ptr(), pt, comp, _host_ptr(fep, e0v), fld[0].data_ptr(),
            e0_field_cases.SCALE, *tail), 'fep_return_map_field_dev')
    else:
        call = lambda: _lib(fep).check(getattr(fep.lib(), RM_ENTRY[model])(                                # noqa: E731
            0, st, n, whole.data_ptr(), pt, comp, _host_ptr(fep, e0v), *tail), RM_ENTRY[model])
    note = _run(a, call, label)
    if fill is None:
        return None
    for k, v in o.items():
        _checked(note, fully_written, v, name=k)
    _checked(note, unchanged, whole, e_in, 'strain')                    # the unused columns with it: they stay poison
    if order == 'strided':
        _checked(note, untouched, whole[:, 3:], name='unused columns of the strain view')
        assert bool((used == _dev(E)).all())
    for i, (m, m_in) in enumerate(md):
        _checked(note, unchanged, m, m_in, f'material {i}')
    if fld is not None:
        _checked(note, unchanged, *fld, 'e0_field')
    elastic = o['ind_p'] == 0
    assert bool((o['ind_p'] <= 1).all()) and int(o['counts'].sum()) == int(o['ind_p'].sum()), note
    if accept:
        _checked(note, same_bits, ep[:, elastic], ep_in[:, elastic], 'ep where ind_p is false')
    else:
        _checked(note, unchanged, ep, ep_in, 'ep')
    return dict(o, note=note)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
@pytest.mark.parametrize('entry,model', [('plain', 'dp'), ('plain', 'vm'), ('plain', 'mc'), ('field', 'dp'), ('field', 'vm'),
                                         ('field', 'mc')])
def test_mesh_free_return_maps_write_their_outputs_and_nothing_else(fep, entry, model, n):
    pts = _mesh_free_points(model, n)
    label = f'return map {entry} {model} n = {n}'
    _return_map_call(fep, label, entry, model, pts, 'C', False, fill=None)       # the counters' scratch of the stream
    first = None
    for order in ('C', 'F', 'strided'):
        for accept in (False, True):
            r = _return_map_call(fep, f'{label} {order} accept = {accept}', entry, model, pts, order, accept)
            if first is None:
                first = r
            for k in ('s', 'ds', 'ind_p', 'counts'):                    # the layout of the strain and the accept flag change no bit
                _checked(r['note'], same_bits, r[k], first[k], f'{k} against the C-order, non-accepting call')
    if n >= 255:
        assert 0 < int(first['ind_p'].sum()) < n


def _dp_context(fep, monkeypatch, t, route, elem, coord):
    from conftest import dp_materials
    ctx = _context(fep, monkeypatch, route, elem, coord)
    ctx.set_materials(*dp_materials(ctx.n_int))
    return ctx


def _caller_meshes():
    from fan_mesh import fan_mesh
    yield ('P1', 'node', 'orphans') + p1_node_cases.mesh('orphans')[:2]
    yield ('P4', 'default', 'curved') + meshes.named('P4', 'curved', np.random.default_rng(zlib.crc32(b'P4 curved')))[:2]
    yield ('P1', 'default', 'fan16') + tuple(fan_mesh(16, 'P1'))


@pytest.mark.parametrize('t,route,name,elem,coord', list(_caller_meshes()), ids=lambda v: v if isinstance(v, str) else '')
def test_transform_loads_and_point_coordinates_write_their_outputs_and_nothing_else(fep, monkeypatch, t, route, name, elem, coord):
    ctx = _dp_context(fep, monkeypatch, t, route, elem, coord)
    try:
        rng = np.random.default_rng(zlib.crc32(f'callers {t} {name}'.encode()))
        q = rng.normal(size=ctx.n_int)
        fv = rng.normal(size=(2, ctx.n_int))
        orphan_dofs = _orphan_dofs(ctx)
        orphan = orphan_dofs[::2]
        assert (name == 'orphans') == bool(orphan.any())
        for fill in (None, 0xFF):
            label = f'{t} {name}'
            # transform: a node of no element holds a COMPUTED NaN (0 / 0), not the poison
            a = _arena(fill)
            qd, q_in = a.put(q, name='q_int')
            out = a.take(ctx.n_n, name='q_node')
            note = _run(a, lambda: ctx.transform_dev(_stream(), qd.data_ptr(), out.data_ptr()), label + ' transform_dev')
            if fill is not None:
                _checked(note, fully_written, out, name='q_node')
                _checked(note, unchanged, qd, q_in, 'q_int')
                assert bool(torch.isnan(out[orphan]).all()) and bool(torch.isfinite(out[~orphan]).all()), note
                _checked(note, same_bits, out, _dev(ctx.transform(q)), 'q_node against the host form')
            # volume load: a field, then the uniform form
            for what in ('field', 'uniform'):
                a = _arena(fill)
                fd, f_in = a.put(fv, name='f_v')
                out = a.take(ctx.n_dof, name='f_out')
                kw = dict(f_v_int=fd.data_ptr()) if what == 'field' else dict(uniform=(0.37, -9.81))
                note = _run(a, lambda: ctx.load_volume_dev(_stream(), out.data_ptr(), **kw), f'{label} load_volume_dev {what}')
                if fill is not None:
                    _checked(note, fully_written, out, name='f_out')
                    _checked(note, unchanged, fd, f_in, 'f_v')
                    assert bool((out[orphan_dofs] == 0).all()) and bool(torch.isfinite(out).all()), note
            a = _arena(fill)
            xq = a.take((2, ctx.n_int), name='xq')
            note = _run(a, lambda: ctx.point_coords_dev(_stream(), xq.data_ptr()), label + ' point_coords_dev')
            if fill is not None:
                _checked(note, fully_written, xq, name='xq')
                _checked(note, same_bits, xq, _dev(ctx.point_coords()), 'xq against the host form')
    finally:
        ctx.close()


def test_traction_load_writes_its_output_and_nothing_else(fep):
    """fep_load_traction_dev: f_out zeroed by the caller (include/fep.h: zero off the loaded edges), the guards poisoned."""
    import load_cases as lc
    case = lc.traction_case(fep, 'tunnel wall level 0 P2, 2-point, random, shuffled')
    ed = np.ascontiguousarray(case.edges, dtype=np.int32)
    host = fep.load_traction(*case.args())
    for fill in (None, 0xFF):
        a = _arena(fill)
        xy, xy_in = a.put(case.coord, name='xy')
        t, t_in = a.put(case.t_int, name='t_int')
        out = a.take(2 * case.n_n, name='f_out')
        out.zero_()
        def call():
            rc = _lib(fep).lib().fep_load_traction_dev(0, _stream(), case.n_n, case.n_e_s, case.n_p_s, case.n_q_s, _host_ptr(fep, ed),
                                                       xy.data_ptr(), _host_ptr(fep, case.h), _host_ptr(fep, case.dh),
                                                       _host_ptr(fep, case.wf), t.data_ptr(), out.data_ptr())
            assert rc == 0
        note = _run(a, call, 'fep_load_traction_dev')
        if fill is not None:
            _checked(note, unchanged, xy, xy_in, 'xy')
            _checked(note, unchanged, t, t_in, 't_int')
            want = _dev(np.ascontiguousarray(host.T).ravel())
            _checked(note, same_bits, out, want, 'f_out against the host form')


def test_solver_entry_points_write_their_outputs_and_nothing_else(fep, monkeypatch):
    """fep_solver_spmv_dev (y), fep_solver_pcg_dev and fep_solver_amg_pcg_dev (x) on one small case of solver_cases."""
    import solver_cases as sc
    name = 'orphans-P1'
    elem, coord, t = sc.mesh(name)
    ctx = _dp_context(fep, monkeypatch, t, 'node', elem, coord)
    sol = None
    try:
        r = ctx.step(sc.displacement(name), np.zeros((4, ctx.n_int)), want=('K', 'F'))
        K, b = r['K'].data, np.random.default_rng(3).normal(size=ctx.n_dof)
        sol = fep.KrylovSolver(ctx, sc.free_dofs(name))
        x0 = b * sol.free_dof
        results = {}
        for what in ('spmv', 'spmv masked', 'jacobi', 'amg'):
            if what == 'amg':
                sol.setup_amg(K, coord, coarse_nodes=sc.ALL[name]['coarse_nodes'])
            for fill in (None, 0xFF, 0x00):
                a = _arena(fill)
                kd, k_in = a.put(K, name='k_data')
                vd, v_in = a.put(x0 if what.startswith('spmv') else b, name='x' if what.startswith('spmv') else 'b')
                out = a.take(ctx.n_dof, name='y' if what.startswith('spmv') else 'x')
                if what.startswith('spmv'):
                    call = lambda: sol.spmv(kd, vd, out=out, masked=what.endswith('masked'))       # noqa: E731
                else:
                    call = lambda: sol.pcg(kd, vd, out=out, rtol=1e-10, max_iter=2000, precond=what)   # noqa: E731
                note = _run(a, call, f'solver {what} on {name}')
                if fill is None:
                    continue
                if fill == 0xFF:
                    _checked(note, fully_written, out, name='output')
                    results[what] = out.clone()
                else:
                    _checked(note, same_bits, out, results[what], 'output on 0x00 against the one on 0xFF')
                _checked(note, unchanged, kd, k_in, 'k_data')
                _checked(note, unchanged, vd, v_in, 'input vector')
                assert bool(torch.isfinite(out).all()), note
                if not what.startswith('spmv'):
                    assert sol.last['state'] == 1, (note, sol.last)
                    assert bool((out[_dev(~sol.free_dof)] == 0).all()), note
    finally:
        if sol is not None:
            sol.close()
        ctx.close()


def test_interface_exchange_kernels_write_their_outputs_and_nothing_else(fep):
    """fep_gather_f64, fep_scatter_f64, fep_iface_sum_f64 on the tables of test_iface_sum_kernel_is_the_host_rank_order_sum's
    partition: entries off the index list stay as they were."""
    mesh = fep.rect_mesh(9, 7, 'P1', 10, 10)
    rng = np.random.default_rng(11)
    elem = mesh['elements'][:, rng.permutation(mesh['elements'].shape[1])]
    part = fep.Partition(elem, mesh['coordinates'].shape[1], 1, 3, exchange='p2p')
    assert (part.mult == 3).any() and (part.mult == 2).any()
    lib, check = fep.lib(), _lib(fep).check
    n_loc = 2 * part.nodes.size
    F = rng.normal(size=n_loc)
    loc_h, slot_h = part.iface_local_dofs.astype(np.int32), part.iface_slot_dofs.astype(np.int32)
    pack_h = np.full(2 * part.n_iface, -1, dtype=np.int32)
    pack_h[slot_h] = loc_h
    assert 0 < loc_h.size < n_loc and (pack_h < 0).any()
    # gather: every entry of dst written, 0 where the index is negative
    a = _arena(0xFF)
    src, src_in = a.put(F, name='src')
    idx, idx_in = a.put(pack_h, name='idx')
    dst = a.take(pack_h.size, name='dst')
    note = _run(a, lambda: check(lib.fep_gather_f64(0, _stream(), pack_h.size, src.data_ptr(), idx.data_ptr(), dst.data_ptr()),
                                 'fep_gather_f64'), 'fep_gather_f64')
    _checked(note, fully_written, dst, name='dst')
    _checked(note, unchanged, src, src_in, 'src')
    _checked(note, unchanged, idx, idx_in, 'idx')
    _checked(note, same_bits, dst, _dev(np.where(pack_h >= 0, F[np.maximum(pack_h, 0)], 0.0)), 'dst')
    # scatter: dst[loc] = buf[slot], the rest of dst as it was
    buf_h = rng.normal(size=pack_h.size)
    a = _arena(0xFF)
    buf, buf_in = a.put(buf_h, name='src')
    slot, slot_in = a.put(slot_h, name='src_idx')
    loc, loc_in = a.put(loc_h, name='dst_idx')
    dst, dst_in = a.put(F, name='dst')
    note = _run(a, lambda: check(lib.fep_scatter_f64(0, _stream(), slot_h.size, buf.data_ptr(), slot.data_ptr(), loc.data_ptr(),
                                                     dst.data_ptr()), 'fep_scatter_f64'), 'fep_scatter_f64')
    off = np.ones(n_loc, dtype=bool)
    off[loc_h] = False
    off_d = _dev(off)
    _checked(note, same_bits, dst[off_d], dst_in[off_d], 'dst off the index list')
    _checked(note, same_bits, dst, _dev(_scattered(F, buf_h, slot_h, loc_h)), 'dst against the host statement')
    for v, v_in, nm in ((buf, buf_in, 'src'), (slot, slot_in, 'src_idx'), (loc, loc_in, 'dst_idx')):
        _checked(note, unchanged, v, v_in, nm)
    # interface sum: f on the interface DOFs, the rest of f as it was
    recv_h = rng.normal(size=part.p2p_send_dofs.size)
    want = F.copy()
    part._iface_sum_host(want, recv_h)
    a = _arena(0xFF)
    f, f_in = a.put(F, name='f')
    recv, recv_in = a.put(recv_h, name='recv')
    loc, loc_in = a.put(loc_h, name='loc')
    ptr, ptr_in = a.put(part.p2p_ptr, name='ptr')
    srx, srx_in = a.put(part.p2p_src, name='src')
    assert ptr.dtype == I32 and srx.dtype == I32
    note = _run(a, lambda: check(lib.fep_iface_sum_f64(0, _stream(), loc_h.size, loc.data_ptr(), ptr.data_ptr(), srx.data_ptr(),
                                                       recv.data_ptr(), f.data_ptr()), 'fep_iface_sum_f64'), 'fep_iface_sum_f64')
    _checked(note, same_bits, f[off_d], f_in[off_d], 'f off the interface')
    _checked(note, same_bits, f, _dev(want), 'f against the host statement')
    for v, v_in, nm in ((recv, recv_in, 'recv'), (loc, loc_in, 'loc'), (ptr, ptr_in, 'ptr'), (srx, srx_in, 'src')):
        _checked(note, unchanged, v, v_in, nm)


def _scattered(F, buf, slot, loc):
    out = F.copy()
    out[loc] = buf[slot]
    return out


def test_csr_merge_writes_all_of_its_output_and_nothing_else(fep):
    """fep_csr_merge_f64 on one plan of test_gathered_solve_gpu.py (pairs of one, two and three contributions)."""
    from test_gathered_solve_gpu import _plans
    m = fep.square_mesh(5, 'P2', 10)
    elem, n_n = m['elements'], m['coordinates'].shape[1]
    p0 = _plans(fep, elem, n_n, 7)[0]
    cnt = np.diff(p0.multi_ptr)
    assert (p0.first >= 0).any() and (cnt == 2).any() and cnt.max() == 3
    rng = np.random.default_rng(7)
    recv_h = rng.normal(size=p0.n_recv) * 10.0 ** rng.integers(-8, 8, size=p0.n_recv)
    k_h, _ = p0.merge_host(recv_h)
    outs = []
    for fill in (0xFF, 0x00):
        a = _arena(fill)
        tabs = [a.put(np.ascontiguousarray(t, dtype=np.int32), name=nm)
                for t, nm in ((p0.first, 'first'), (p0.multi_ptr, 'multi_ptr'), (p0.multi_src, 'multi_src'))]
        recv, recv_in = a.put(recv_h, name='recv')
        k = a.take(p0.nnz, name='k_global')
        assert p0.nnz == 4 * p0.n_blocks
        note = _run(a, lambda: _lib(fep).check(fep.lib().fep_csr_merge_f64(0, _stream(), p0.n_blocks, *(t.data_ptr() for t, _ in tabs),
                                                                           recv.data_ptr(), k.data_ptr()), 'fep_csr_merge_f64'),
                    f'fep_csr_merge_f64 on {fill:#04x}')
        if fill == 0xFF:
            _checked(note, fully_written, k, name='k_global')
        _checked(note, same_bits, k, _dev(k_h), 'k_global against the host statement')
        _checked(note, unchanged, recv, recv_in, 'recv')
        for (t, t_in), nm in zip(tabs, ('first', 'multi_ptr', 'multi_src')):
            _checked(note, unchanged, t, t_in, nm)


TAIL = 7                                                                # elements past what fep_mesh_info sizes: must stay poison


def _mesh_cases():
    from conftest import load_golden
    from test_mesh_gpu import _orient
    g = load_golden('tsx')
    yield 'tunnel', g['coord'], g['elem']
    el, co = meshes.delaunay('P1', 40, np.random.default_rng(3))
    yield 'delaunay 40, last 40 dropped', co, meshes.drop_last(_orient(el, co), 40)


def _with_tail(a, shape, dtype, name):
    """A view of `shape` whose allocation is TAIL elements longer: -> (view, tail)."""
    n = int(np.prod(shape))
    flat = a.take(n + TAIL, dtype, name=name)
    return flat[:n].view(shape), flat[n:]


@pytest.mark.parametrize('name,coord,elem', list(_mesh_cases()), ids=lambda v: v if isinstance(v, str) else '')
def test_mesh_entry_points_write_their_outputs_and_nothing_else(fep, name, coord, elem):
    """fep_mesh_enrich_dev (P2, P4), fep_mesh_refine_dev and fep_mesh_area_stats_dev: the int32 tables and coord_ext fully
    written at the sizes fep_mesh_info gives, and not an element past them."""
    import ctypes as C
    lib, check = fep.lib(), _lib(fep).check
    p = lambda t: C.c_void_p(t.data_ptr())                              # noqa: E731
    with fep.DeviceMesh(coord, elem, 0) as dm:
        i = dm.info
        host = {'P2': dm.enrich('P2'), 'P4': dm.enrich('P4')}
        for fill in (None, 0xFF):
            for t, rows_e, rows_s in (('P2', 6, 3), ('P4', 15, 5)):
                a = _arena(fill)
                n_tot = i['n_n'] + dm.new_nodes(t)
                arrays = [_with_tail(a, (rows_e, i['n_e']), I32, 'elem_ext'), _with_tail(a, (2, n_tot), F64, 'coord_ext'),
                          _with_tail(a, (rows_s, i['n_boundary_edges']), I32, 'surf')]
                if t == 'P2':
                    arrays += [_with_tail(a, (3, i['n_e']), I32, 'elem_ed'), _with_tail(a, (2, i['n_edges']), I32, 'edge_el')]
                ptrs = [p(v) for v, _ in arrays] + [None] * (5 - len(arrays))
                note = _run(a, lambda: check(lib.fep_mesh_enrich_dev(dm._h, dm._stream(), 2 if t == 'P2' else 5, *ptrs),
                                             'fep_mesh_enrich_dev'), f'fep_mesh_enrich_dev {t} on {name}')
                if fill is None:
                    continue
                for (v, tail), nm in zip(arrays, ('elem_ext', 'coord_ext', 'surf', 'elem_ed', 'edge_el')):
                    _checked(note, fully_written, v, name=nm)
                    _checked(note, untouched, tail, name=f'the {TAIL} elements past {nm}')
                h = host[t]
                _checked(note, same_bits, arrays[0][0], _dev(h['elem_ext'].astype(np.int32)), 'elem_ext')
                _checked(note, same_bits, arrays[1][0], _dev(h['coord_ext']), 'coord_ext')
            a = _arena(fill)
            child, coord_ext = _with_tail(a, (3, 4 * i['n_e']), I32, 'elem_child'), _with_tail(a, (2, i['n_n'] + i['n_edges']), F64, 'coord_ext')
            note = _run(a, lambda: check(lib.fep_mesh_refine_dev(dm._h, dm._stream(), p(child[0]), p(coord_ext[0])),
                                         'fep_mesh_refine_dev'), f'fep_mesh_refine_dev on {name}')
            if fill is not None:
                for (v, tail), nm in ((child, 'elem_child'), (coord_ext, 'coord_ext')):
                    _checked(note, fully_written, v, name=nm)
                    _checked(note, untouched, tail, name=f'the {TAIL} elements past {nm}')
                co_h, el_h = dm.refine()
                _checked(note, same_bits, child[0], _dev(el_h.astype(np.int32)), 'elem_child')
                _checked(note, same_bits, coord_ext[0], _dev(co_h), 'coord_ext')
    for fill in (None, 0xFF):
        a = _arena(fill)
        el, el_in = a.put(np.ascontiguousarray(elem, dtype=np.int32), name='elem')
        co, co_in = a.put(coord, name='coord')
        out, tail = _with_tail(a, (4,), F64, 'out')
        note = _run(a, lambda: fep.area_stats_dev(co, el, 0, out=out), f'fep_mesh_area_stats_dev on {name}')
        if fill is not None:
            _checked(note, fully_written, out, name='out')
            _checked(note, untouched, tail, name='the elements past out')
            _checked(note, unchanged, el, el_in, 'elem')
            _checked(note, unchanged, co, co_in, 'coord')
            assert float(out[3]) == elem.shape[1] and bool(torch.isfinite(out).all()), (note, out.tolist())

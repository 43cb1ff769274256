"""
A context's results depend on its current configuration and on the arguments of the current call, and on nothing that was
called before: long, mixed sequences of every call a MeshContext has, on one context, each call compared bit for bit with the
same call on a fresh context that was configured directly (tests/sequence_cases.py; the generator, the coverage conditions
and the harness itself are checked on the CPU by test_sequence_cases_host.py).

What the sequences walk (struct fep_ctx, fep_api.hip): the model, the homogeneous-material fast path decided inside
fep_ctx_set_materials_host, the four material arrays that every model reads its own way, the hardening curve that outlives a
change of its model and back, the lazily allocated ds / s scratch and branch counters shared by the Drucker-Prager and the
model steps, by the P1 one-kernel and two-kernel steps and by the *_host and *_dev forms, the persistent device blocks of the
host forms that alias by design (step, assemble, transform, load_volume, point_coords, recover_stress and estimate write
into each other's blocks), and the profiling events.

Per (element type, route) eight sequences of about forty call ops: together they hold every ordered pair of the twelve call
classes, once across configuration ops and once with nothing between the two calls, every ordered pair of models, uniform
<-> per-point materials under three models or more, curves replaced by shorter and by longer ones, model changes that leave
the material arrays to be read anew, host / dev / graph-replay forms in every order, refused calls (fep_ctx_set_model(h, 7), set_hardening on another model, a curve that does not increase, a NULL
U, a misaligned F) and poisoned ones (a NaN at one node of U, one NaN in the per-point materials) in between.

Precondition, asserted first for every context: two fresh contexts give identical bytes for a representative op of every call
class in every form, on a Drucker-Prager context with uniform materials and on a 'vmi' context with per-point materials and
the eight-segment curve.  No class or form is excepted.

Two directed sequences, written out by hand: the aliased host blocks in every order on a 'dp' and on a 'vmi' context, and one
P1 node context taken through all five models twice with, at each stop, a K,F-only *_dev step replayed from a graph captured
at that stop, an accepting K-only step and a points-only step (the one-kernel and the two-kernel step sharing the counters
and the ds / s scratch across every model).
"""
import numpy as np
import pytest

import sequence_cases as sq
from routes import assert_route
from sequence_cases import EVERY, Config, op

pytestmark = pytest.mark.gpu

GRID = [(t, r) for t in sq.TYPES for r in sq.ROUTES[t]]
_MEMO = {}                                                              # (t, route) -> results of fresh contexts, shared by its tests
_PRECONDITION = {}


def _maker(fep, monkeypatch, t, route):
    """make_context of (t, route): route selection and its assertion as test_model_step_routes_gpu.py has them."""
    if route in ('default', 'node'):
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    elem, coord = sq.mesh(t)

    def make():
        ctx = fep.MeshContext(np.array(elem), np.array(coord))
        assert_route(ctx, 'patch' if route == 'default' else route)
        return ctx
    return make


def _step(state, want=EVERY, form='host', **kw):
    d = dict(state=state, form=form, want=want, accept=False, ep='state', e0=True, field=False, poison=None, profile=False)
    d.update(kw)
    return op('step', **d)


def representative_ops(model):
    """One op per call class and form (the refusals return nothing)."""
    ops = []
    for form in sq.FORMS:
        ops += [_step('A', form=form), _step('A', ('K', 'F'), form), _step('A', ('s', 'ds', 'ind_p'), form),
                _step('A', ('K',), form, accept=True), _step('A', form=form, field=True), _step('A', form=form, poison='U')]
        if model != 'vmi':
            ops.append(_step('A', ('K', 'F'), form, poison='mats'))
    for form in ('host', 'dev'):
        ops += [op('assemble', state='A', form=form, which='KF', profile=False), op('transform', state='A', form=form),
                op('load_volume', state='A', form=form, mode='weight'), op('point_coords', state='A', form=form),
                op('recover', state='A', form=form), op('estimate', state='A', form=form)]
    ops.append(_step('A', ('K', 'F'), 'dev', profile=True))
    return ops


def _precondition(make, t, route):
    """Fresh against fresh, once per context -> the (model, class, form) that are NOT bit-reproducible (none is expected)."""
    if (t, route) not in _PRECONDITION:
        bad = []
        for cfg in (Config('dp', 'uniform', 'dp', None, False), Config('vmi', 'per_point', 'vmi', 2, False)):
            first, second = {}, {}
            for o in representative_ops(cfg.model):
                a, b = sq.fresh(make, t, cfg, o, first), sq.fresh(make, t, cfg, o, second)
                assert a is not b
                d = sq.first_difference(a, b)
                if d is not None:
                    bad.append((cfg.model, sq.call_class(o), o.get('form'), d))
        print(f'[precondition] {t} {route}: fresh against fresh differs in {len(bad)} of the representative ops {bad}')
        _PRECONDITION[t, route] = bad
    return _PRECONDITION[t, route]


@pytest.mark.parametrize('t,route', GRID)
def test_two_fresh_contexts_give_identical_bytes(fep, monkeypatch, t, route):
    assert _precondition(_maker(fep, monkeypatch, t, route), t, route) == []


@pytest.mark.parametrize('t,route,seed', [(t, r, s) for t, r in GRID for s in range(sq.N_SEEDS)])
def test_results_do_not_depend_on_the_calls_before(fep, monkeypatch, t, route, seed):
    make = _maker(fep, monkeypatch, t, route)
    assert _precondition(make, t, route) == []
    seq = sq.sequence(t, route, seed)
    outs = sq.check(make, t, seq, _MEMO.setdefault((t, route), {}))
    calls = [r for r in outs if r]
    assert len(calls) >= 30 and all(isinstance(v, np.ndarray) for r in calls for v in r.values())


def test_the_comparison_sees_another_configuration(fep, monkeypatch):
    """The harness on the GPU's own data: against the fresh results of the OTHER materials, or of the other state, the first
    call op is named; against its own it passes."""
    make = _maker(fep, monkeypatch, 'P2', 'default')
    seq = _config_ops('vm', 'per_point') + [_step('A', ('F',), 'dev'), _step('B', ('ind_p',), 'host')]
    outs = sq.run(make, 'P2', seq)
    memo = {}
    sq.compare(seq, outs, lambda cfg, o: sq.fresh(make, 'P2', cfg, o, memo))
    for wrong in (lambda cfg, o: (cfg._replace(mats_kind='uniform'), o),
                  lambda cfg, o: (cfg, sq.Op(o.kind, tuple((k, 'AB'[v == 'A'] if k == 'state' else v) for k, v in o.args)))):
        with pytest.raises(sq.SequenceMismatch) as e:
            sq.compare(seq, outs, lambda cfg, o: sq.fresh(make, 'P2', *wrong(cfg, o), memo))
        assert e.value.index == 2, str(e.value)


def _config_ops(model, mats, curve=None):
    ops = [op('set_model', model=model), op('set_materials', mats=mats)]
    return ops + ([op('set_hardening', curve=curve)] if curve is not None else [])


@pytest.mark.parametrize('model', ['dp', 'vmi'])
@pytest.mark.parametrize('t,route', [('P1', 'node'), ('P2', 'default')])
def test_aliased_host_blocks_in_every_order(fep, monkeypatch, t, route, model):
    """fep_ctx::hbuf: kBufFv = kBufXq = kBufS, kBufLoad = kBufF, kBufWeight = kBufQ.  The host calls that write into each
    other's blocks, forwards, then backwards."""
    make = _maker(fep, monkeypatch, t, route)
    host = dict(form='host')
    calls = [op('load_volume', state='A', mode='points', **host), _step('B', ('F',)), op('transform', state='A', **host),
             op('load_volume', state='B', mode='weight', **host), _step('A', ('K', 'F')), op('point_coords', state='B', **host),
             op('recover', state='A', **host), _step('B'), op('estimate', state='A', **host)]
    seq = _config_ops(model, 'per_point', 3 if model == 'vmi' else None) + calls + calls[::-1]
    sq.check(make, t, seq, _MEMO.setdefault((t, route), {}))


def test_p1_node_context_through_all_models_twice(fep, monkeypatch):
    """The one-kernel step (K,F-only, here replayed from a graph captured at the stop) and the two-kernel steps (accepting
    K-only through the ds / s scratch, points-only) share slot_counts, the branch counters and the scratch across every model;
    the second visit of 'vmi' runs on the curve of the first."""
    make = _maker(fep, monkeypatch, 'P1', 'node')
    seq, n = [], 0
    for lap in range(2):
        for model in sq.MODELS:
            seq += _config_ops(model, ('uniform', 'per_point')[(lap + sq.MODELS.index(model)) % 2],
                               2 if (model, lap) == ('vmi', 0) else None)
            seq += [_step('AB'[n % 2], ('K', 'F'), 'graph'), _step('AB'[(n + 1) % 2], ('K',), 'host', accept=True),
                    _step('AB'[n % 2], ('s', 'ds', 'ind_p'), 'dev')]
            n += 1
    assert sq.illegal('P1', seq) is None
    sq.check(make, 'P1', seq, _MEMO.setdefault(('P1', 'node'), {}))

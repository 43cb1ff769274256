"""The generator and the harness of tests/sequence_cases.py, on the CPU.

1. The generator is deterministic, every sequence is legal, and the sequences that test_call_sequences_gpu.py runs for a
   (type, route) meet the coverage conditions below.  They are conditions on the generator: where one fails, the generator is
   tuned, never the condition.
2. The harness passes on a correct implementation: SwitchContext, a context look-alike that switches between the per-model
   CPU contexts of plastic_exact_cases.lookalike (assemble from oracle.fep_oracle's tangent and internal_force, transform
   from newton.transform, load_volume from tests/loads_ref.py, recover / estimate from the NumPy twins of estimate.py; its
   *_dev and graph forms are the host form), run through every sequence against its own fresh copies.
3. The harness has teeth: nine subclasses of the look-alike with ONE planted history fault each, modelled on state that fep_ctx
   really keeps between calls (fep_api.hip, struct fep_ctx).  Each must fail a short sequence at the first call op at which
   the fault is observable, and that index is asserted; the random P1 sequences must catch each of them as well.
"""
import numpy as np
import pytest

import e0_field_ref as fref
import loads_ref
import plastic_exact_cases as pec
import sequence_cases as sq
from sequence_cases import EVERY, op

fep = sq.fep


# ---------------------------------------------------------------------------------------
# the look-alike
# ---------------------------------------------------------------------------------------
class StateError(RuntimeError):
    code = sq.FEP_ESTATE


class SwitchContext:
    """A MeshContext look-alike for all five models: the per-model CPU contexts behind one configuration."""
    is_lookalike = True

    def __init__(self, t):
        self.t = t
        self.elem, self.coord = (np.array(v) for v in sq.mesh(t))
        self.tab = fep.element_tables(t)
        self.n_e, self.n_n = self.elem.shape[1], self.coord.shape[1]
        self.n_int, self.n_dof = self.n_e * sq.msc.NQ[t], 2 * self.n_n
        tt = fep.LagrangeElementType[t]
        self.hatp = np.asarray(fep.get_local_basis_volume(tt, fep.get_quadrature_volume(tt)[0])[0], dtype=float)
        self.model, self._mats, self._hardening = 'dp', None, (np.zeros(1), np.zeros(1))
        self._subs, self._set_on, self._version = {}, {}, 0

    def close(self):
        pass

    # -- configuration
    def set_model(self, model):
        if model not in sq.MODELS:
            raise ValueError(model)
        self.model = model

    def refused(self, what):
        """The refusals of sequence_cases.REFUSALS as this look-alike meets them."""
        if what == 'model7':
            with pytest.raises(ValueError):
                self.set_model(7)
        elif what == 'hardening_state':
            with pytest.raises(StateError):
                self.set_hardening(*sq.curve_arrays(1))
        elif what == 'bad_curve':
            with pytest.raises((ValueError, StateError)):
                self.set_hardening(*sq.BAD_CURVE)
        elif what == 'null_U':
            with pytest.raises(ValueError):
                self.step(None)
        else:
            assert what == 'misaligned_F'                                   # host arrays have no such refusal

    def set_materials(self, *mats):
        a = tuple(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=float).ravel(), (self.n_int,))) for v in mats)
        if self.model == 'vmi':
            fep.hardening.check_curve(*self._hardening, shear=a[0], a=a[2], Y=a[3])
        self._mats = a
        self._version += 1

    def set_hardening(self, kappa, slope):
        if self.model != 'vmi':
            raise StateError('set_hardening on a context of another model')
        if self._mats is not None:
            curve = fep.hardening.check_curve(kappa, slope, shear=self._mats[0], a=self._mats[2], Y=self._mats[3])
        else:
            curve = fep.hardening.check_curve(kappa, slope)
        self._hardening = self._store_curve(curve)

    def _store_curve(self, curve):
        return curve

    def _materials(self):
        return self._mats

    def _sub(self):
        """The current model's CPU context on the current materials (and curve)."""
        m = self.model
        if m not in self._subs:
            self._subs[m] = (fref.FieldContext if m == 'dp' else pec.lookalike(m))(self.elem, self.coord, *self.tab)
        sub = self._subs[m]
        if self._set_on.get(m) != self._version:
            sub.set_materials(*self._materials())
            self._set_on[m] = self._version
        if m == 'vmi':
            sub.hardening = self._hardening
        return sub

    # -- calls
    def step(self, U, ep_prev=None, e0=None, apply_plastic_strain=False, want=(), e0_field=None, e0_scale=1.0):
        if U is None:
            raise ValueError('U')
        sub = self._sub()
        accept = bool(apply_plastic_strain) and ep_prev is not None
        if e0_field is None:
            r = sub.step(U, ep_prev, e0=e0, apply_plastic_strain=accept)
        else:
            z = fref.z_of(e0, e0_field, e0_scale)
            if self.model in ('dp', 'vmi'):                                 # these restatements take an initial strain per point
                r = sub.step(U, ep_prev, e0=z, apply_plastic_strain=accept)
            else:
                r = self._field_step(sub, U, ep_prev, z, accept)
        if 'E' not in r:
            r = dict(r, E=np.asarray(sub.orc.strain(sub.c['B'], np.asarray(U, dtype=float))))
        r = self._after_step(dict(r), want)
        out = {k: r[k] for k in want}
        out['n_smooth'], out['n_apex'] = int(r['n_smooth']), int(r['n_apex'])
        return out

    def _field_step(self, sub, U, ep_prev, z, accept):
        """RefContext.step with the initial strain z[:, k] at point k: the model's restatement takes one (4, 1) initial
        strain, so it is applied point by point."""
        c, n = sub.c, self.n_int
        E = np.asarray(sub.orc.strain(c['B'], np.asarray(U, dtype=float)))
        s, ds, ind, ep = np.empty((4, n)), np.empty((9, n)), np.zeros(n, dtype=bool), np.zeros((4, n))
        counts = [0, 0]
        for k in range(n):
            r = sub.return_map(E[:, k:k + 1], None if ep_prev is None else ep_prev[:, k:k + 1], *(m[k:k + 1] for m in sub.m),
                               apply_plastic_strain=accept, e0=z[:, k].reshape(4, 1))
            s[:, k], ds[:, k], ind[k], ep[:, k] = r['s'][:, 0], r['ds'][:, 0], r['ind_p'][0], r['ep'][:, 0]
            counts[0] += int(r['n_smooth'])
            counts[1] += int(r['n_apex'])
        if accept:
            ep_prev[...] = ep
        K = sub.orc.tangent(c['K_elast'], c['B'], c['D_elast'], c['weight'], ds, c['iD'], c['jD'])
        return {'E': E, 'K': K.tocsr(), 'F': sub.orc.internal_force(c['B'], c['weight'], s), 's': s, 'ds': ds, 'ind_p': ind,
                'n_smooth': counts[0], 'n_apex': counts[1]}

    def _after_step(self, r, want):
        return r

    def _weight(self):
        return np.asarray(self._sub().c['weight'], dtype=float).ravel()

    def assemble(self, ds=None, s=None):
        sub = self._sub()
        c = sub.c
        K = None if ds is None else sub.orc.tangent(c['K_elast'], c['B'], c['D_elast'], c['weight'], np.asarray(ds, dtype=float),
                                                    c['iD'], c['jD']).tocsr()
        F = None if s is None else sub.orc.internal_force(c['B'], c['weight'], np.asarray(s, dtype=float))
        return K, F

    def transform(self, q_int):
        with np.errstate(invalid='ignore'):                                 # a node whose weights sum to zero: 0 / 0, as the kernel's
            return fep.transform(q_int, self.elem, self._weight())

    def load_volume(self, f_v_int=None, uniform=None, hatp=None, weight=None):
        f = np.asarray(f_v_int, dtype=float) if uniform is None else np.array(uniform, dtype=float).reshape(2, 1) * np.ones((1, self.n_int))
        return loads_ref.volume(self.elem, self.n_n, f, self.hatp, self._weight() if weight is None else weight)[0]

    def point_coords(self):
        return fref.point_coords(fep, self.t, self.elem, self.coord)[0]

    def recover_stress(self, s):
        return fep.recover_stress_np(self.elem, self._weight(), s, self.n_n)

    def estimate(self, s):
        return fep.estimate_np(self.elem, self._weight(), self._mats[0], self._mats[1], self.hatp, s, self.n_n)


# ---------------------------------------------------------------------------------------
# the planted faults
# ---------------------------------------------------------------------------------------
class StaleUniformFlag(SwitchContext):
    """a. fep_ctx::matu: the uniform flag is kept from an earlier set_materials, so per-point arrays set after uniform ones
    are read at their first value everywhere."""
    def set_materials(self, *mats):
        super().set_materials(*mats)
        uniform = all(np.all(v == v[0]) for v in self._mats)
        self._matu = getattr(self, '_matu', False) or uniform

    def _materials(self):
        return tuple(np.full_like(v, v[0]) for v in self._mats) if self._matu else self._mats


class CountersNotReset(SwitchContext):
    """b. blk_counts / slot_counts: the branch counters are not zeroed between steps, n_smooth accumulates."""
    def _after_step(self, r, want):
        self._acc = getattr(self, '_acc', 0) + int(r['n_smooth'])
        r['n_smooth'] = self._acc
        return r


class StaleTangentScratch(SwitchContext):
    """c. ds_int / s_int: a K-only or K,F-only step assembles the ds and s of the previous call."""
    def _after_step(self, r, want):
        last = getattr(self, '_last', None)
        self._last = (r['ds'], r['s'])
        if last is not None and set(want) <= {'K', 'F'}:
            r['K'], r['F'] = self.assemble(*last)
        return r


class ModelChangeResetsCurve(SwitchContext):
    """d. fep_ctx::hard: set_model resets the curve to the flat one."""
    def set_model(self, model):
        super().set_model(model)
        self._hardening = (np.zeros(1), np.zeros(1))


class ShorterCurveKeepsTail(SwitchContext):
    """e. fep_ctx::hard: a curve with fewer segments leaves the old tail segments in place."""
    def _store_curve(self, curve):
        old = self._hardening
        if old[0].size > curve[0].size:
            return (np.concatenate([curve[0], old[0][curve[0].size:]]), np.concatenate([curve[1], old[1][curve[1].size:]]))
        return curve


class LoadLeftInF(SwitchContext):
    """f. kBufLoad = kBufF: load_volume's result is still in F when the next F-only step returns."""
    def load_volume(self, *a, **k):
        out = super().load_volume(*a, **k)
        self._load = out.reshape(-1, order='F')
        return out

    def _after_step(self, r, want):
        if tuple(want) == ('F',) and getattr(self, '_load', None) is not None:
            r['F'] = np.asarray(r['F']).ravel() + self._load
        self._load = None
        return r


class TransformReadsLoadWeights(SwitchContext):
    """g. kBufWeight = kBufQ: transform's weights are those of the previous load_volume(weight=)."""
    def load_volume(self, f_v_int=None, uniform=None, hatp=None, weight=None):
        if weight is not None:
            self._w = np.array(weight)
        return super().load_volume(f_v_int, uniform, hatp, weight)

    def transform(self, q_int):
        w = getattr(self, '_w', None)
        with np.errstate(invalid='ignore'):
            return fep.transform(q_int, self.elem, self._weight() if w is None else w)


class RefusedModelSticks(SwitchContext):
    """h. fep_ctx::model: a refused set_model changes the model all the same (to the first one)."""
    def refused(self, what):
        super().refused(what)
        if what == 'model7':
            self.model = 'dp'


class PoisonSurvives(SwitchContext):
    """i. the persistent blocks: the NaN of a poisoned call survives in the next call's F."""
    def _after_step(self, r, want):
        F = np.array(r['F'], dtype=float).ravel()
        stale = getattr(self, '_nan', None)
        self._nan = np.isnan(F)
        if stale is not None and stale.any():
            F[stale] = np.nan
            r['F'] = F
        return r


def _step(state, want=EVERY, **kw):
    d = dict(state=state, form='host', want=want, accept=False, ep='state', e0=False, field=False, poison=None, profile=False)
    d.update(kw)
    return op('step', **d)


def _setup(model, kind='uniform'):
    return [op('set_model', model=model), op('set_materials', mats=kind)]


# fault -> (class, the short sequence, the index of the first call op at which the fault is observable)
FAULTS = {
    'a': (StaleUniformFlag, _setup('vm') + [_step('A'), op('set_materials', mats='per_point'), _step('B'), _step('A')], 4),
    'b': (CountersNotReset, _setup('mc') + [_step('A'), _step('B', want=('ind_p',)), _step('A')], 3),
    'c': (StaleTangentScratch, _setup('dp') + [_step('A'), _step('B', want=('K', 'F')), _step('A')], 3),
    'd': (ModelChangeResetsCurve, _setup('vmi') + [op('set_hardening', curve=2), _step('A'), op('set_model', model='vm'), _step('B'),
                                                   op('set_model', model='vmi'), _step('A'), _step('B')], 7),
    'e': (ShorterCurveKeepsTail, _setup('vmi') + [op('set_hardening', curve=2), _step('A'), op('set_hardening', curve=1), _step('B'),
                                                  _step('A')], 5),
    'f': (LoadLeftInF, _setup('vmps') + [op('load_volume', state='A', form='host', mode='points'), _step('B', want=('F',)), _step('A')], 3),
    'g': (TransformReadsLoadWeights, _setup('dp') + [op('load_volume', state='A', form='host', mode='weight'),
                                                     op('transform', state='B', form='host'), _step('A')], 3),
    'h': (RefusedModelSticks, _setup('vm') + [op('refuse', what='model7'), _step('A'), _step('B')], 2),  # the driver reads ctx.model
    'i': (PoisonSurvives, _setup('mc') + [_step('A', poison='U'), _step('B', want=('F',)), _step('A')], 3),
}


# ---------------------------------------------------------------------------------------
# 1. the generator
# ---------------------------------------------------------------------------------------
GRID = [(t, r) for t in sq.TYPES for r in sq.ROUTES[t]]


def _sequences(t, route):
    return [sq.sequence(t, route, seed) for seed in range(sq.N_SEEDS)]


@pytest.mark.parametrize('t,route', GRID)
def test_generator_is_deterministic_and_legal(t, route):
    for seed in range(sq.N_SEEDS):
        seq = sq.sequence(t, route, seed)
        assert seq == sq.sequence(t, route, seed)
        assert sq.illegal(t, seq) is None, (seed, sq.illegal(t, seq))
        calls = [o for o in seq if sq.is_call(o) and o.kind != 'refuse']
        assert [o.get('state') for o in calls] == ['AB'[k % 2] for k in range(len(calls))]      # A and B alternate
    assert _sequences(t, route) != _sequences(*GRID[(GRID.index((t, route)) + 1) % len(GRID)])


def test_illegal_draws_are_recognised():
    bad = [[_step('A')],
           _setup('vm') + [op('set_model', model='mc'), _step('A')],
           _setup('vm') + [op('set_hardening', curve=1)],
           _setup('vmi') + [_step('A', poison='mats')],
           _setup('vmi') + [op('refuse', what='hardening_state')],
           _setup('vm') + [_step('A', accept=True, ep='zeros')],
           _setup('vm') + [op('transform', state='A', form='graph')]]
    for seq in bad:
        assert sq.illegal('P1', seq) is not None, seq


@pytest.mark.parametrize('t,route', GRID)
def test_coverage_conditions(t, route):
    cov = sq.coverage(_sequences(t, route))
    # every ordered pair of the twelve call classes
    missing = {(a, b) for a in sq.CLASSES for b in sq.CLASSES} - cov['class_pairs']
    assert not missing, sorted(missing)
    missing = {(a, b) for a in sq.CLASSES for b in sq.CLASSES} - cov['direct_class_pairs']      # and with nothing between the two
    assert not missing, sorted(missing)
    mixed = sq.coverage(_sequences(t, route)[:sq.N_PARTS])['class_pairs']                       # and across configuration ops
    assert len(mixed) == len(sq.CLASSES) ** 2
    assert cov['refusals'] == set(sq.REFUSALS)
    # every ordered pair of distinct models
    assert cov['model_pairs'] == {(a, b) for a in sq.MODELS for b in sq.MODELS if a != b}
    # uniform -> per point and back, each under three models or more
    for a, b in (('uniform', 'per_point'), ('per_point', 'uniform')):
        assert len({m for x, y, m in cov['kind_changes'] if (x, y) == (a, b)}) >= 3, (a, b, cov['kind_changes'])
    # a curve replaced by one with fewer segments and by one with more
    assert cov['curves'] == {'fewer', 'more'}
    # a model change followed by a call with no set_materials between
    assert cov['reinterpreted']
    assert all(sq.FAMILY[a] == sq.FAMILY[b] for a, b in cov['reinterpreted'])
    # a return to 'vmi' steps on the curve of the earlier stay
    assert cov['curve_kept']
    # forms
    assert {('host', 'dev'), ('dev', 'host'), ('graph', 'host'), ('host', 'graph')} <= cov['form_pairs']
    # P1 node: the one-kernel K,F-only step directly beside the full-output step and beside an accepting K-only step
    if (t, route) == ('P1', 'node'):
        kf, full, k_acc = ('step-KF', ('K', 'F'), False), ('step-every', EVERY, False), ('step-accepting', ('K',), True)
        assert {(kf, full), (full, kf), (kf, k_acc), (k_acc, kf)} <= cov['direct_pairs']


@pytest.mark.parametrize('t', sq.TYPES)
def test_states_reach_both_branches_on_the_shared_mesh(t):
    """Every state, with the uniform and the per-point materials of its model, has plastic and elastic points on the one mesh
    all models share (the generators drew it for their own jitter of the same rectangle): a twentieth of the points or more on
    either side, which is 12 points of the smallest mesh.  ('vmi' puts the median point at 1.5 yield radii, and state B is 1.7
    times state A, so its plastic share is the largest.)"""
    ctx = SwitchContext(t)
    S = sq.states(t)
    assert S['n_int'] > 256 and S['n_int'] % 256 != 0
    for m in sq.MODELS:
        ctx.set_model(m)
        for kind in ('uniform', 'per_point'):
            ctx.set_materials(*S['mats'][m, kind])
            for label in 'AB':
                st = S['state'][m][label]
                r = ctx.step(np.array(st['U']), np.array(st['ep']), want=('ind_p',))
                share = r['ind_p'].mean()
                assert 0.05 <= share <= 0.95, (m, kind, label, share)
        if m == 'mc':
            assert r['n_apex'] > 0 or t != 'P4'


# ---------------------------------------------------------------------------------------
# 2. the harness passes on a correct implementation
# ---------------------------------------------------------------------------------------
_MEMO = {}


def _memo(cls, t):
    return _MEMO.setdefault((cls, t), {})


@pytest.mark.parametrize('t,route,seed', [(t, r, s) for t, r in GRID for s in range(sq.N_SEEDS)])
def test_lookalike_passes_every_sequence(t, route, seed):
    outs = sq.check(lambda: SwitchContext(t), t, sq.sequence(t, route, seed), _memo(SwitchContext, t))
    assert sum(r is not None for r in outs) >= 30


# ---------------------------------------------------------------------------------------
# 3. the harness has teeth
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_planted_fault_is_caught_at_the_first_observable_op(fault):
    cls, seq, index = FAULTS[fault]
    assert sq.illegal('P1', seq) is None
    sq.check(lambda: SwitchContext('P1'), 'P1', seq, _memo(SwitchContext, 'P1'))       # the sequence itself is sound
    with pytest.raises(sq.SequenceMismatch) as e:
        sq.check(lambda: cls('P1'), 'P1', seq, _memo(SwitchContext, 'P1'))             # the oracle is the CORRECT fresh context
    assert e.value.index == index, (fault, e.value.index, str(e.value))
    with pytest.raises(sq.SequenceMismatch) as e:
        sq.check(lambda: cls('P1'), 'P1', seq, _memo(cls, 'P1'))                       # and the faulty one's own fresh copies
    assert e.value.index == index, (fault, e.value.index, str(e.value))


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_random_sequences_catch_every_planted_fault(fault):
    cls = FAULTS[fault][0]
    for route, seed in [(r, s) for r in sq.ROUTES['P1'] for s in range(sq.N_SEEDS)]:
        try:
            sq.check(lambda: cls('P1'), 'P1', sq.sequence('P1', route, seed), _memo(cls, 'P1'))
        except sq.SequenceMismatch:
            return
    raise AssertionError(f'no P1 sequence catches fault {fault}')

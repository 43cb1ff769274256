"""Shared by test_sequence_cases_host.py and test_call_sequences_gpu.py: long, mixed sequences of calls on ONE context, and the
check that every result depends only on the context's current configuration and on the arguments of the current call.

The oracle of a call is the same call on a fresh context that was configured directly (`fresh`): set_model, set_materials,
set_hardening once each, the one call, close.  The library promises reproducible bytes, so the comparison is bit for bit (the
sign bit of a NaN excepted, as transfer_cases.same_but_nan_sign has it).  What a fresh context computes is what the per-entry
suites hold to the float64 restatements: the states are those of their generators.

Configuration (`Config`): the model, the materials (uniform or per point, and the model whose generator drew them: a model
change without set_materials reinterprets the arrays set last, which set_model's docstring allows), the hardening curve as last
set (an id of model_step_cases.CURVES or None: never set; it outlives a change of the model and back) and whether the call is
bracketed by profile_begin / profile_end.

States (`states`): per model two states A and B of displacement, previous plastic strain, (4, 1) initial strain and field with
its scale.  A is the first accepted draw of the model's own generator for the mesh block257 (model_step_cases.build,
vmps_cases.build, e0_field_cases.build for 'dp'), drawn again here because those return the materials and the initial strain by
the case's flags only; the draws are asserted equal to the generators'.  B is footprint.scrub's second state: -1.7 U, half the
plastic strain with its points reversed.  Successive call ops alternate A and B, so that an output left over from the call
before differs from the expected one.  ONE mesh per element type carries all five models (a context has one mesh): the
block257 mesh of the 'vm' case; the generators jitter the same rectangle by another seed per model, so a state keeps its
sizes and, to the jitter, its strains (test_sequence_cases_host.py asserts that every state has plastic and elastic points
under its model on this mesh).  Point kernels run two or more workgroups with a partial last one on it.

Ops (`op`): configuration ops set_model, set_materials, set_hardening; call ops step (want, accept, ep in {None, zeros, the
state's}, e0, field, poison in {None, 'U', 'mats'}, profile), assemble (K and F, K, F), transform, load_volume (point values,
uniform=, weight=), point_coords, recover, estimate; and refusals (`refuse`), which must leave the configuration and every
later result alone.  A call op has a form: 'host' (MeshContext's methods), 'dev' (the *_dev entry point on torch tensors on a
side stream) or 'graph' (a step only: one replay of a graph captured from the *_dev call after one eager warm call of the
same form).  The stream contract of include/fep.h is followed to the letter: before a host call (a configuration call is
one) the stream of the pending *_dev calls is synchronised, and the harness waits for nothing else; the results of *_dev calls
are read back only then.  (One wait is not the harness's: torch.cuda.graph synchronises the device before it captures.)

Two model families share the meaning of the four material arrays: (shear, bulk, a, Y) for 'vm', 'vmps', 'vmi' and (shear, bulk,
friction, cohesion) for 'dp', 'mc'.  A model change inside a family may leave the arrays in place; one across families is
followed by set_materials before the next call (a hardening modulus read as a friction coefficient makes every result NaN,
and a comparison of NaNs sees nothing)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import e0_field_cases as fc
import model_step_cases as msc
import vmps_cases
from conftest import dp_materials
from elem_ref import ElemRef

fep = msc.fep
MODELS = ('dp', 'vm', 'mc', 'vmps', 'vmi')
FAMILY = {'dp': 'cone', 'mc': 'cone', 'vm': 'mises', 'vmps': 'mises', 'vmi': 'mises'}
MESH = 'block257'
TYPES = msc.TYPES
ROUTES = {'P1': ('node', 'patch', 'coo'), 'P2': ('default', 'coo'), 'Q1': ('default',), 'Q2': ('default',), 'P4': ('default',)}
EVERY = ('E', 's', 'ds', 'ind_p', 'K', 'F')
WANTS = (EVERY, ('K', 'F'), ('K',), ('F',), ('s', 'ds', 'ind_p'), ('ind_p',))
CLASSES = ('step-every', 'step-KF', 'step-points', 'step-accepting', 'step-field', 'assemble', 'transform', 'load_volume',
           'point_coords', 'recover/estimate', 'refused', 'poisoned')
REFUSALS = ('model7', 'hardening_state', 'bad_curve', 'null_U', 'misaligned_F')
FORMS = ('host', 'dev', 'graph')
N_PARTS = 4                                                             # a circuit of the call classes is walked in four parts
N_SEEDS = 2 * N_PARTS                                                   # sequences per (type, route): two circuits
FEP_EINVAL, FEP_ESTATE = -1, -6

Config = namedtuple('Config', 'model mats_kind mats_from curve profiling')
START = Config('dp', None, None, None, False)                          # a context as fep_ctx_create leaves it


class Op(namedtuple('Op', 'kind args')):
    __slots__ = ()

    def get(self, key, default=None):
        return dict(self.args).get(key, default)

    def __repr__(self):
        return f'{self.kind}(' + ', '.join(f'{k}={v!r}' for k, v in self.args) + ')'


def op(kind, **kw):
    return Op(kind, tuple(sorted(kw.items())))


CONFIG_OPS = ('set_model', 'set_materials', 'set_hardening')


def is_call(o):
    return o.kind not in CONFIG_OPS


def call_class(o):
    if o.kind == 'refuse':
        return 'refused'
    if o.kind in ('recover', 'estimate'):
        return 'recover/estimate'
    if o.kind != 'step':
        return o.kind
    if o.get('poison'):
        return 'poisoned'
    if o.get('field'):
        return 'step-field'
    if o.get('accept'):
        return 'step-accepting'
    want = tuple(o.get('want'))
    if want == EVERY:
        return 'step-every'
    return 'step-KF' if set(want) <= {'K', 'F'} else 'step-points'


def next_config(cfg, o):
    """The configuration after `o` (a refusal and a call change nothing; a poisoned call restores the materials itself)."""
    if o.kind == 'set_model':
        return cfg._replace(model=o.get('model'))
    if o.kind == 'set_materials':
        return cfg._replace(mats_kind=o.get('mats'), mats_from=cfg.model)
    if o.kind == 'set_hardening':
        return cfg._replace(curve=o.get('curve'))
    return cfg


def configs(seq):
    """The configuration each op of `seq` meets."""
    out, cfg = [], START
    for o in seq:
        out.append(cfg)
        cfg = next_config(cfg, o)
    return out


def curve_arrays(c):
    return msc.vmi_cases.curve(c)


def curve_is_legal(t, cfg):
    """set_hardening / set_materials of a 'vmi' context check the law's preconditions on the host (hardening.check_curve)."""
    if cfg.model != 'vmi' or cfg.mats_kind is None:
        return True
    m = materials(t, cfg)
    kap, slo = (np.zeros(1), np.zeros(1)) if cfg.curve is None else curve_arrays(cfg.curve)
    try:
        fep.hardening.check_curve(kap, slo, shear=m[0], a=m[2], Y=m[3])
        return True
    except ValueError:
        return False


def illegal(t, seq):
    """None, or (index, why) of the first op a correct context would not take as the sequence means it."""
    cfg = START
    for i, o in enumerate(seq):
        if o.kind == 'set_model' and o.get('model') not in MODELS:
            return i, 'unknown model'
        if o.kind == 'set_hardening' and cfg.model != 'vmi':
            return i, 'set_hardening on another model is a refusal, not a configuration op'
        if is_call(o) and o.kind != 'refuse':
            if cfg.mats_kind is None:
                return i, 'a call before set_materials'
            if FAMILY[cfg.mats_from] != FAMILY[cfg.model]:
                return i, 'materials of the other family'
            if o.get('form') == 'graph' and o.kind != 'step':
                return i, 'graph form of another call than a step'
            if o.get('poison') == 'mats' and cfg.model == 'vmi':
                return i, "set_materials of a 'vmi' context refuses a NaN (check_curve)"
            if o.get('accept') and o.get('ep') != 'state':
                return i, 'an accepting call needs the plastic strain'
            if o.get('profile') and o.get('form') != 'dev':
                return i, 'profiling brackets *_dev calls'
        if o.kind == 'refuse' and o.get('what') == 'hardening_state' and cfg.model == 'vmi':
            return i, "set_hardening is legal on 'vmi'"
        cfg = next_config(cfg, o)
        if o.kind in CONFIG_OPS and not curve_is_legal(t, cfg):
            return i, 'the curve breaks the preconditions on these materials'
    return None


# ---------------------------------------------------------------------------------------
# meshes, states, materials
# ---------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mesh(t):
    """(elem, coord): the block257 mesh of the 'vm' case of model_step_cases."""
    elem, coord = msc.mesh(t, MESH, np.random.default_rng(msc.seed('vm', t, MESH)))
    elem, coord = np.ascontiguousarray(elem), np.ascontiguousarray(coord)
    elem.setflags(write=False)
    coord.setflags(write=False)
    return elem, coord


def _draw_a(model, t):
    """State A and the per-point materials of `model`: the generator's own accepted draw, made again with every array kept."""
    if model == 'vmps':
        c = vmps_cases.build(t, MESH)
        rng = np.random.default_rng(msc.seed('vmps', t, MESH))
        elem, coord = msc.mesh(t, MESH, rng)
        U, ep, per_point, e0 = vmps_cases.state(t, elem, coord, rng)
        field = None
    elif model == 'dp':
        c = fc.build('dp', t, MESH)
        rng = np.random.default_rng(fc.seed('dp', t, MESH))
        elem, coord = msc.mesh(t, MESH, rng)
        ref = ElemRef(elem, coord, fep.element_tables(t))
        for _ in range(c['draw'] + 1):
            U, ep, per_point, e0 = fc.dp_state(elem, coord, ref, rng)
            field = fc.eps_y('dp') * rng.normal(0, 0.2, size=(4, ref.n_int))
        assert np.array_equal(field, c['field'])
    else:
        c = msc.build(model, t, MESH)
        rng = np.random.default_rng(msc.seed(model, t, MESH))
        elem, coord = msc.mesh(t, MESH, rng)
        for _ in range(c['draw'] + 1):
            U, ep, per_point, e0 = msc.state(model, t, elem, coord, rng, c['curve'])
        field = None
    assert np.array_equal(U, c['U']) and np.array_equal(ep, c['ep']), (model, t, 'not the draw of the generator')
    if field is None:
        rng = np.random.default_rng(zlib.crc32(f'sequence field {model} {t}'.encode()))
        field = fc.eps_y('vm' if model == 'vmps' else model) * rng.normal(0, 0.2, size=ep.shape)
    return dict(U=U, ep=ep, e0=e0, field=field), per_point


def _second(a):
    """State B of state A: footprint.scrub's."""
    return dict(U=-1.7 * a['U'], ep=np.ascontiguousarray(0.5 * a['ep'][:, ::-1]), e0=-0.6 * a['e0'],
                field=np.ascontiguousarray(0.8 * a['field'][:, ::-1]))


@functools.lru_cache(maxsize=None)
def states(t):
    """-> dict: 'state'[model][A | B] = dict U, ep, e0, field; 'mats'[model, uniform | per_point] = four (n_int,) arrays;
    'aux'[A | B] = dict ds, s, q, f, w (the inputs of assemble, recover / estimate, transform and load_volume: symmetric
    tangents and stresses that no context computed); sizes.  Computed once per session, read-only."""
    elem, coord = mesh(t)
    n_int, n_n = elem.shape[1] * msc.NQ[t], coord.shape[1]
    one = np.ones(n_int)
    st, mats = {}, {}
    for m in MODELS:
        a, per_point = _draw_a(m, t)
        assert a['U'].shape == (2, n_n) and a['ep'].shape == (4, n_int)
        st[m] = {'A': _frozen(a), 'B': _frozen(_second(a))}
        uni = dp_materials(n_int) if m == 'dp' else tuple(v * one for v in (vmps_cases.UNIFORM if m == 'vmps' else msc.UNIFORM[m]))
        mats[m, 'uniform'] = tuple(np.ascontiguousarray(v, dtype=float) for v in uni)
        mats[m, 'per_point'] = tuple(np.ascontiguousarray(v, dtype=float) for v in per_point)
        for v in mats[m, 'uniform'] + mats[m, 'per_point']:
            v.setflags(write=False)
    aux = {}
    for label in 'AB':
        rng = np.random.default_rng(zlib.crc32(f'sequence aux {t} {label}'.encode()))
        ds = np.zeros((9, n_int))
        for (i, j), v in zip(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), (3e5, 3e5, 1e5, 1e5, 0.0, 0.0)):
            ds[3 * i + j] = ds[3 * j + i] = v * rng.uniform(0.6, 1.4, n_int) + 2e4 * rng.normal(size=n_int)
        aux[label] = _frozen(dict(ds=ds, s=300.0 * rng.normal(size=(4, n_int)), q=rng.normal(size=n_int),
                                  f=rng.normal(size=(2, n_int)), w=rng.uniform(0.5, 1.5, n_int)))
    return dict(state=st, mats=mats, aux=aux, n_int=n_int, n_n=n_n)


def materials(t, cfg):
    return states(t)['mats'][cfg.mats_from, cfg.mats_kind]


def poisoned_materials(t, cfg):
    """The configuration's materials per point with one NaN (the shear modulus of the middle point)."""
    m = [np.array(v) for v in materials(t, cfg)]
    m[0][m[0].size // 2] = np.nan
    return tuple(m)


BAD_CURVE = (np.array([0.0, 1e-3, 1e-3]), np.array([1e4, 1e4, 1e4]))    # not strictly increasing: check_curve rejects it


# ---------------------------------------------------------------------------------------
# the seeded generator
# ---------------------------------------------------------------------------------------
def _circuit(n, loops, rng):
    """A random Eulerian circuit of the complete digraph on n vertices (with loops: n * n edges) -> the vertices visited,
    first = last (Hierholzer)."""
    out = {v: [w for w in rng.permutation(n).tolist() if loops or w != v] for v in range(n)}
    stack, walk = [int(rng.integers(n))], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(' '.join(str(k) for k in key).encode()))


def _pick(rng, seq, p=None):
    return seq[int(rng.choice(len(seq), p=p))]


def _draw_call(rng, cls, cfg, state, n_refused=0):
    """One call op of class `cls` on configuration `cfg`; draws a correct context would not take are replaced.  Refusals
    come in rotation (`n_refused`: how many the circuit has had)."""
    form = _pick(rng, FORMS, p=(0.5, 0.3, 0.2))
    plain = 'dev' if form == 'graph' else form
    if cls.startswith('step') or cls == 'poisoned':
        kw = dict(state=state, form=form, want=EVERY, accept=False, ep=_pick(rng, (None, 'zeros', 'state')), e0=bool(rng.integers(2)),
                  field=False, poison=None, profile=False)
        if cls == 'step-KF':
            kw['want'] = _pick(rng, (('K', 'F'), ('K',), ('F',)))
        elif cls == 'step-points':
            kw['want'] = _pick(rng, (('s', 'ds', 'ind_p'), ('ind_p',)))
        elif cls == 'step-accepting':
            kw.update(want=_pick(rng, WANTS), accept=True, ep='state')
        elif cls == 'step-field':
            kw.update(want=_pick(rng, WANTS), field=True)
            if rng.integers(2):
                kw.update(accept=True, ep='state')
        elif cls == 'poisoned':
            kw.update(want=_pick(rng, (EVERY, ('K', 'F'), ('F',))), poison='U' if cfg.model == 'vmi' else _pick(rng, ('U', 'mats')))
        if kw['form'] == 'dev' and rng.random() < 0.3:
            kw['profile'] = True
        return op('step', **kw)
    if cls == 'assemble':
        return op('assemble', state=state, form=plain, which=_pick(rng, ('KF', 'K', 'F')),
                  profile=plain == 'dev' and rng.random() < 0.3)
    if cls == 'load_volume':
        return op('load_volume', state=state, form=plain, mode=_pick(rng, ('points', 'uniform', 'weight')))
    if cls == 'recover/estimate':
        return op(_pick(rng, ('recover', 'estimate')), state=state, form=plain)
    if cls == 'refused':
        what = REFUSALS[n_refused % len(REFUSALS)]
        if what == 'hardening_state' and cfg.model == 'vmi':
            what = 'bad_curve'
        elif what == 'bad_curve' and cfg.model != 'vmi' and n_refused >= len(REFUSALS):
            what = 'hardening_state'                                        # the turn it lost on a 'vmi' context
        return op('refuse', what=what)
    return op(cls, state=state, form=plain)                                # transform, point_coords


def _other_curve(rng, current):
    """A curve with another number of segments than the one in place (ids 0 and 1 have one segment, 2 eight, 3 four)."""
    size = None if current is None else curve_arrays(current)[0].size
    return _pick(rng, [c for c in range(4) if curve_arrays(c)[0].size != size])


def _model_change(rng, t, cfg, model, out):
    """set_model(model) and, across families always, inside one half of the time, set_materials; on 'vmi' often a curve."""
    def push(o):
        nxt = next_config(cfg_now[0], o)
        if o.kind in CONFIG_OPS and not curve_is_legal(t, nxt):
            return
        out.append(o)
        cfg_now[0] = nxt
    cfg_now = [cfg]
    push(op('set_model', model=model))
    c = cfg_now[0]
    if c.mats_kind is None or FAMILY[c.mats_from] != FAMILY[model] or rng.random() < 0.5:
        push(op('set_materials', mats=_pick(rng, ('uniform', 'per_point'))))
    if model == 'vmi':
        push(op('set_hardening', curve=_other_curve(rng, cfg_now[0].curve)))
    return cfg_now[0]


def sequence(t, route, seed):
    """The ops of sequence `seed` (0 .. N_SEEDS - 1) of (t, route): deterministic.  The call classes of sequences 0 .. 3
    together walk one Eulerian circuit of all 144 ordered class pairs, each sequence a quarter of it, and their model changes
    one of the 20 ordered pairs of models; what else happens between the calls is drawn.  Sequences 4 .. 7 walk a second pair
    of circuits with nothing between two calls but the model changes, after each of which the class before it is called
    again, so that every class pair also occurs with nothing at all between the two calls."""
    assert 0 <= seed < N_SEEDS and route in ROUTES[t]
    part, direct = seed % N_PARTS, seed >= N_PARTS
    shared = _rng('sequence', t, route, 'direct' if direct else 'mixed')
    classes = _circuit(len(CLASSES), True, shared)
    models = _circuit(len(MODELS), False, shared)
    per = (len(classes) - 1) // N_PARTS
    cls = [CLASSES[k] for k in classes[part * per:(part + 1) * per + 1]]
    mdl = [MODELS[k] for k in models[part * 5:(part + 1) * 5 + 1]]
    rng = _rng('sequence', t, route, seed)
    out = []
    cfg = _model_change(rng, t, START, mdl[0], out)
    if cfg.mats_kind is None:
        out.append(op('set_materials', mats='uniform'))
        cfg = next_config(cfg, out[-1])
    n_calls = 0
    n_refused = sum(CLASSES[k] == 'refused' for k in classes[:part * per])

    def call(c):
        nonlocal n_calls
        nonlocal n_refused
        out.append(_draw_call(rng, c, cfg, 'AB'[n_calls % 2], n_refused))
        n_calls += out[-1].kind != 'refuse'                                 # a refusal takes no state
        n_refused += out[-1].kind == 'refuse'
    if t == 'P1' and route == 'node' and seed == 0:
        # the one-kernel and the two-kernel step and the lazily allocated ds / s scratch, directly adjacent
        for want, accept in ((EVERY, False), (('K', 'F'), False), (EVERY, False), (('K',), True), (('K', 'F'), False), (('K',), True)):
            out.append(op('step', state='AB'[n_calls % 2], form='host', want=want, accept=accept, ep='state' if accept else 'zeros',
                          e0=False, field=False, poison=None, profile=False))
            n_calls += 1
    change_at = set((1 + np.sort(rng.choice(len(cls) - 1, size=len(mdl) - 1, replace=False))).tolist())
    k = 1
    for i, c in enumerate(cls):
        if i in change_at:
            cfg = _model_change(rng, t, cfg, mdl[k], out)
            k += 1
            if direct:
                call(cls[i - 1])
        elif i and not direct and rng.random() < (0.7 if cfg.model == 'vmi' else 0.4):
            if cfg.model == 'vmi' and rng.random() < 0.6:
                o = op('set_hardening', curve=_other_curve(rng, cfg.curve))
            else:
                o = op('set_materials', mats='per_point' if cfg.mats_kind == 'uniform' or rng.random() < 0.2 else 'uniform')
            if curve_is_legal(t, next_config(cfg, o)):
                out.append(o)
                cfg = next_config(cfg, o)
        call(c)
    # the curve outlives a change of the model and back: a stay on 'vmi' with a curve, another model of the family, 'vmi' again
    if cfg.model != 'vmi' or cfg.curve is None:
        cfg = _model_change(rng, t, cfg, 'vmi', out)
    call('step-KF')
    out.append(op('set_model', model=_pick(rng, ('vm', 'vmps'))))
    cfg = next_config(cfg, out[-1])
    call('step-every')
    out.append(op('set_model', model='vmi'))
    cfg = next_config(cfg, out[-1])
    call(_pick(rng, ('step-every', 'step-accepting', 'step-field')))
    return out


def coverage(seqs):
    """The sets the coverage conditions of test_sequence_cases_host.py are stated on, over the sequences `seqs`.
    class_pairs: classes of two call ops with nothing but configuration ops between them; direct_class_pairs: with nothing
    between them; direct_pairs: (class, want, accept) of two ops with nothing between them; model_pairs: (from, to) of
    set_model; kind_changes: (from, to, model) of a set_materials that changes uniform <-> per point; curves: 'fewer' /
    'more' segments than the curve replaced;
    reinterpreted: (from, to) of a model change with no set_materials before the next call; curve_kept: (model left, curve)
    of a return to 'vmi' that steps on the curve of an earlier stay, with no set_hardening since; form_pairs."""
    cov = dict(class_pairs=set(), direct_pairs=set(), model_pairs=set(), kind_changes=set(), curves=set(), reinterpreted=set(),
               form_pairs=set(), classes=set(), refusals=set(), curve_kept=set(), direct_class_pairs=set())
    for seq in seqs:
        cfgs = configs(seq)
        last = prev = pending = back = None
        for cfg, o in zip(cfgs, seq):
            if is_call(o):
                c = call_class(o)
                cov['classes'].add(c)
                if o.kind == 'refuse':
                    cov['refusals'].add(o.get('what'))
                if last is not None:
                    cov['class_pairs'].add((call_class(last), c))
                    if last.get('form') and o.get('form'):
                        cov['form_pairs'].add((last.get('form'), o.get('form')))
                if prev is not None and is_call(prev):
                    cov['direct_class_pairs'].add((call_class(prev), c))
                    cov['direct_pairs'].add(((call_class(prev), prev.get('want'), prev.get('accept')),
                                             (c, o.get('want'), o.get('accept'))))
                if pending is not None and o.kind != 'refuse':
                    cov['reinterpreted'].add(pending)
                    pending = None
                if back is not None and o.kind == 'step':
                    cov['curve_kept'].add(back)
                    back = None
                last = o
            elif o.kind == 'set_model':
                if o.get('model') != cfg.model:
                    cov['model_pairs'].add((cfg.model, o.get('model')))
                    pending = (cfg.model, o.get('model')) if cfg.mats_kind is not None else None
                    back = (cfg.model, cfg.curve) if o.get('model') == 'vmi' and cfg.curve is not None else None
            elif o.kind == 'set_materials':
                pending = None
                if cfg.mats_kind is not None and cfg.mats_kind != o.get('mats'):
                    cov['kind_changes'].add((cfg.mats_kind, o.get('mats'), cfg.model))
            elif o.kind == 'set_hardening':
                back = None
                a, b = (None if c is None else curve_arrays(c)[0].size for c in (cfg.curve, o.get('curve')))
                if a is not None and a != b:
                    cov['curves'].add('fewer' if b < a else 'more')
            prev = o
    return cov


# ---------------------------------------------------------------------------------------
# running ops on a context
# ---------------------------------------------------------------------------------------
class Driver:
    """Applies ops to one context (a MeshContext, or a CPU look-alike with `is_lookalike`, on which every form is the host
    form).  Results of *_dev calls stay on the device until `sync`, which waits for the side stream alone."""

    def __init__(self, ctx, t):
        self.ctx, self.t, self.S = ctx, t, states(t)
        self.gpu = not getattr(ctx, 'is_lookalike', False)
        self.pending = []                                                   # result dicts that still hold tensors
        self.side = None

    # -- the stream contract
    def sync(self):
        if self.pending:
            self.side.synchronize()
            for r in self.pending:
                for k, v in list(r.items()):
                    if not isinstance(v, np.ndarray):                       # (a poisoned call has read its results back already)
                        r[k] = v.cpu().numpy()
            self.pending = []

    def _stream(self):
        import torch
        if self.side is None:
            self.side = _side_stream()
        return torch.cuda.stream(self.side)

    def _up(self, a):
        import torch
        return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(torch.device('cuda', 0))

    def _empty(self, shape, dtype=None):
        import torch
        return torch.empty(shape, dtype=dtype or torch.float64, device=torch.device('cuda', 0))

    # -- configuration
    def configure(self, cfg):
        """A fresh context straight to `cfg`: one call each."""
        self.ctx.set_model(cfg.model)
        self.ctx.set_materials(*materials(self.t, cfg))
        if cfg.model == 'vmi' and cfg.curve is not None:
            self.ctx.set_hardening(*curve_arrays(cfg.curve))

    def apply(self, cfg, o):
        """`o` on the context, which is configured as `cfg` -> None (a configuration op) or the dict of the call's outputs
        (a refusal: empty)."""
        ctx = self.ctx
        if o.kind in CONFIG_OPS:
            self.sync()
            if o.kind == 'set_model':
                ctx.set_model(o.get('model'))
            elif o.kind == 'set_materials':
                ctx.set_materials(*materials(self.t, next_config(cfg, o)))
            else:
                ctx.set_hardening(*curve_arrays(o.get('curve')))
            return None
        if o.kind == 'refuse':
            self.sync()
            self._refuse(cfg, o.get('what'))
            assert ctx.model == cfg.model, ('a refused call changed the model', o)
            return {}
        host = not self.gpu or o.get('form') == 'host'
        if host:
            self.sync()
        r = getattr(self, '_' + o.kind)(cfg, o, host)
        if not host:
            self.pending.append(r)
        return r

    def _refuse(self, cfg, what):
        ctx = self.ctx
        if not self.gpu:
            return ctx.refused(what)
        import ctypes
        l = fep.lib()
        if what == 'model7':
            assert l.fep_ctx_set_model(ctx.handle, 7) == FEP_EINVAL
            code = ctypes.c_int(-1)
            assert l.fep_ctx_model(ctx.handle, ctypes.byref(code)) == 0 and code.value == fep.hotpath.MODELS[cfg.model]
        elif what == 'hardening_state':
            try:
                ctx.set_hardening(*curve_arrays(1))
            except fep.FepError as e:
                assert e.code == FEP_ESTATE
            else:
                raise AssertionError('set_hardening on a context of another model was not refused')
        elif what == 'bad_curve':
            try:
                ctx.set_hardening(*BAD_CURVE)
            except ValueError:
                pass
            else:
                raise AssertionError('check_curve took a curve that does not increase')
            rc = l.fep_ctx_set_hardening(ctx.handle, 3, BAD_CURVE[0].ctypes.data_as(ctypes.c_void_p),
                                         BAD_CURVE[1].ctypes.data_as(ctypes.c_void_p))
            assert rc == (FEP_EINVAL if cfg.model == 'vmi' else rc) and rc in (FEP_EINVAL, FEP_ESTATE)
        elif what == 'null_U':
            F = np.zeros(ctx.n_dof)
            cnt = np.zeros(2, dtype=np.int64)
            rc = l.fep_step_host(ctx.handle, None, None, None, 0, None, None, None, None, None, F.ctypes.data_as(ctypes.c_void_p),
                                 cnt.ctypes.data_as(ctypes.c_void_p))
            assert rc == FEP_EINVAL and not F.any() and not cnt.any()
        elif what == 'misaligned_F':
            with self._stream():
                U = self._up(np.zeros(ctx.n_dof))
                F = self._empty(ctx.n_dof + 1)
                try:
                    ctx.step_dev(self.side.cuda_stream, U.data_ptr(), f_out=F.data_ptr() + 8)
                except fep.FepError as e:
                    assert e.code == FEP_EINVAL
                else:
                    raise AssertionError('a misaligned F was not refused')
        else:
            raise ValueError(what)

    # -- call ops
    def _step_inputs(self, cfg, o):
        st = self.S['state'][cfg.model][o.get('state')]
        U = np.array(st['U'])
        if o.get('poison') == 'U':
            U[:, U.shape[1] // 2] = np.nan
        ep = {None: None, 'zeros': np.zeros_like(st['ep']), 'state': np.array(st['ep'])}[o.get('ep')]
        kw = {'e0': np.array(st['e0'])} if o.get('e0') else {}
        if o.get('field'):
            kw.update(e0_field=np.array(st['field']), e0_scale=fc.SCALE if o.get('e0') else 1.0)
        return U, ep, kw

    def _step(self, cfg, o, host):
        ctx = self.ctx
        U, ep, kw = self._step_inputs(cfg, o)
        want, accept = tuple(o.get('want')), bool(o.get('accept'))
        if o.get('poison') == 'mats':
            self.sync()
            ctx.set_materials(*poisoned_materials(self.t, cfg))
        if host:
            with np.errstate(all='ignore'):
                r = ctx.step(U, ep, apply_plastic_strain=accept, want=want, **kw)
            out = {k: np.array(r[k].data if k == 'K' else r[k]) for k in want}
            out['counts'] = np.array([r['n_smooth'], r['n_apex']], dtype=np.int64)
            if ep is not None:
                out['ep'] = ep
        else:
            out = self._step_dev(o, U, ep, kw, want, accept)
        if o.get('poison') == 'mats':
            if not host:                                                    # the step is only enqueued: it reads the arrays
                self.pending.append(out)                                    # that set_materials is about to overwrite
            self.sync()                                                     # the next set_materials is clean
            ctx.set_materials(*materials(self.t, cfg))
        return out

    def _step_dev(self, o, U, ep, kw, want, accept):
        import torch
        ctx, n = self.ctx, self.ctx.n_int
        names = {'E': ('e_out', (3, n)), 's': ('s', (4, n)), 'ds': ('ds', (9, n)), 'K': ('k_data', (ctx.nnz,)),
                 'F': ('f_out', (ctx.n_dof,))}
        with self._stream():
            stream = self.side.cuda_stream
            Ud = self._up(U.reshape(-1, order='F'))
            Epd = None if ep is None else self._up(ep)
            fd = self._up(kw['e0_field']) if 'e0_field' in kw else None
            outs = {k: self._empty(names[k][1]) for k in want if k != 'ind_p'}
            if 'ind_p' in want:
                outs['ind_p'] = self._empty(n, torch.uint8)
            outs['counts'] = self._empty(2, torch.int64)

            def call():
                args = {names[k][0] if k in names else k: v.data_ptr() for k, v in outs.items()}
                ctx.step_dev(stream, Ud.data_ptr(), ep=0 if Epd is None else Epd.data_ptr(), accept=accept, e0=kw.get('e0'),
                             e0_field=None if fd is None else fd.data_ptr(), e0_scale=kw.get('e0_scale', 1.0), **args)
            if o.get('form') == 'graph':
                call()                                                      # the eager warm call: whatever allocates does so now
                self.side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    args = {names[k][0] if k in names else k: v.data_ptr() for k, v in outs.items()}
                    ctx.step_dev(torch.cuda.current_stream().cuda_stream, Ud.data_ptr(), ep=0 if Epd is None else Epd.data_ptr(),
                                 accept=accept, e0=kw.get('e0'), e0_field=None if fd is None else fd.data_ptr(),
                                 e0_scale=kw.get('e0_scale', 1.0), **args)
                for v in outs.values():
                    v.zero_()
                if Epd is not None:
                    Epd.copy_(self._up(ep))                                 # the warm call may have accepted: the replay is the run
                g.replay()
                self.graphs = getattr(self, 'graphs', []) + [g]             # alive until the results are read
            else:
                if o.get('profile'):
                    ctx.profile_begin()
                call()
                if o.get('profile'):
                    ms, n_steps = ctx.profile_end(stream)
                    assert n_steps == 1, n_steps
            out = dict(outs)
            if Epd is not None:
                out['ep'] = Epd
            self.keep = (Ud, fd)
        return out

    def _assemble(self, cfg, o, host):
        ctx, a = self.ctx, self.S['aux'][o.get('state')]
        ds = a['ds'] if 'K' in o.get('which') else None
        s = a['s'] if 'F' in o.get('which') else None
        if host:
            K, F = ctx.assemble(ds, s)
            return {k: np.array(v) for k, v in (('K', None if K is None else K.data), ('F', F)) if v is not None}
        with self._stream():
            out = {}
            if ds is not None:
                out['K'] = self._empty(ctx.nnz)
            if s is not None:
                out['F'] = self._empty(ctx.n_dof)
            dsd, sd = (None if v is None else self._up(v) for v in (ds, s))
            if o.get('profile'):
                ctx.profile_begin()
            ctx.assemble_dev(self.side.cuda_stream, ds=0 if dsd is None else dsd.data_ptr(), s=0 if sd is None else sd.data_ptr(),
                             k_data=out['K'].data_ptr() if 'K' in out else 0, f_out=out['F'].data_ptr() if 'F' in out else 0)
            if o.get('profile'):
                ctx.profile_end(self.side.cuda_stream)
            self.keep = (dsd, sd)
        return out

    def _transform(self, cfg, o, host):
        ctx, q = self.ctx, self.S['aux'][o.get('state')]['q']
        if host:
            return {'q_node': np.array(ctx.transform(q))}
        with self._stream():
            qd, out = self._up(q), self._empty(ctx.n_n)
            ctx.transform_dev(self.side.cuda_stream, qd.data_ptr(), out.data_ptr())
            self.keep = qd
        return {'q_node': out}

    def _load_volume(self, cfg, o, host):
        ctx, a, mode = self.ctx, self.S['aux'][o.get('state')], o.get('mode')
        uniform = (0.3, -2.0) if o.get('state') == 'A' else (-1.1, 0.7)
        if host:
            if mode == 'uniform':
                return {'f': np.array(ctx.load_volume(uniform=uniform))}
            return {'f': np.array(ctx.load_volume(a['f'], weight=a['w'] if mode == 'weight' else None))}
        with self._stream():
            out = self._empty(ctx.n_dof)
            fd = None if mode == 'uniform' else self._up(a['f'])
            wd = self._up(a['w']) if mode == 'weight' else None
            ctx.load_volume_dev(self.side.cuda_stream, out.data_ptr(), f_v_int=0 if fd is None else fd.data_ptr(),
                                uniform=uniform if mode == 'uniform' else None, weight=0 if wd is None else wd.data_ptr())
            self.keep = (fd, wd)
        return {'f': out}

    def _point_coords(self, cfg, o, host):
        ctx = self.ctx
        if host:
            return {'xq': np.array(ctx.point_coords())}
        with self._stream():
            out = self._empty((2, ctx.n_int))
            ctx.point_coords_dev(self.side.cuda_stream, out.data_ptr())
        return {'xq': out}

    def _recover(self, cfg, o, host):
        ctx, s = self.ctx, self.S['aux'][o.get('state')]['s']
        if host:
            return {'s_node': np.array(ctx.recover_stress(s))}
        with self._stream():
            sd = self._up(s)
            out = ctx.recover_stress_dev(sd)
            self.keep = sd
        return {'s_node': out}

    def _estimate(self, cfg, o, host):
        ctx, s = self.ctx, self.S['aux'][o.get('state')]['s']
        if host:
            r = ctx.estimate(s)
            return {'eta2': np.array(r['eta2']), 's_node': np.array(r['s_node']),
                    'stats': np.array([r['total'], r['max'], float(r['n_nonfinite'])])}
        with self._stream():
            sd = self._up(s)
            eta2, st, sn = ctx.estimate_dev(sd)
            self.keep = sd
        return {'eta2': eta2, 's_node': sn, 'stats': st}


_SIDE = []


def _side_stream():
    import torch
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def run(make_context, t, seq):
    """`seq` on one context of `make_context()` -> per op None (a configuration op) or the dict of the call's outputs."""
    ctx = make_context()
    try:
        drv = Driver(ctx, t)
        outs = []
        for i, (cfg, o) in enumerate(zip(configs(seq), seq)):
            try:
                outs.append(drv.apply(cfg, o))
            except AssertionError as e:                                     # a refusal that was not one, or that changed the model
                raise SequenceMismatch(i, f'op {i} {o} on {cfg}: {e}') from e
        drv.sync()
        return outs
    finally:
        ctx.close()


def fresh_key(cfg, o):
    """What the result of a call may depend on: the configuration a fresh context is set to, and the op with the graph form
    read as the eager *_dev call."""
    if o.get('form') == 'graph':
        o = Op(o.kind, tuple((k, 'dev' if k == 'form' else v) for k, v in o.args))
    return cfg._replace(curve=cfg.curve if cfg.model == 'vmi' else None, profiling=bool(o.get('profile'))), o


def fresh(make_context, t, cfg, o, memo):
    """The oracle: `o` on a new context configured directly to `cfg`; memoised in `memo` on (config, op)."""
    key = fresh_key(cfg, o)
    if key not in memo:
        if o.kind == 'refuse':
            memo[key] = {}
        else:
            ctx = make_context()
            try:
                drv = Driver(ctx, t)
                drv.configure(key[0])
                r = drv.apply(key[0], key[1])
                drv.sync()
                memo[key] = r
            finally:
                ctx.close()
    return memo[key]


# ---------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------
class SequenceMismatch(AssertionError):
    def __init__(self, index, message):
        super().__init__(message)
        self.index = index


def _bits(a):
    """The integer view of an array's data, the sign bit of every NaN cleared."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a.view(np.uint8) if a.dtype == np.bool_ else a
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] &= ~(np.uint64(1) << np.uint64(63))
    return b


def first_difference(got, want):
    """None, or (output, entry, got, expected) of the first output (by name) and entry that differ bitwise."""
    for k in sorted(want):
        if k not in got:
            return k, None, 'missing', None
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            return k, None, (a.shape, a.dtype), (b.shape, b.dtype)
        d = _bits(a) != _bits(b)
        if d.any():
            idx = tuple(int(v) for v in np.argwhere(d)[0])
            return k, idx, a[idx], b[idx]
    extra = sorted(set(got) - set(want))
    return (extra[0], None, 'not an output of the fresh call', None) if extra else None


def compare(seq, outs, oracle):
    """Every call op's outputs against `oracle(cfg, op)`; SequenceMismatch at the first op that differs, with the op's index,
    the configuration, the last three ops and the first differing output and entry."""
    for i, (cfg, o) in enumerate(zip(configs(seq), seq)):
        if outs[i] is None:
            continue
        d = first_difference(outs[i], oracle(cfg, o))
        if d is not None:
            raise SequenceMismatch(i, f'op {i} {o} on {cfg}\n  after ' + ' ; '.join(repr(p) for p in seq[max(0, i - 3):i])
                                   + f'\n  output {d[0]!r} entry {d[1]}: {d[2]!r}, the fresh context gives {d[3]!r}')


def check(make_context, t, seq, memo):
    """run + compare against fresh contexts of the same `make_context`."""
    bad = illegal(t, seq)
    assert bad is None, bad
    outs = run(make_context, t, seq)
    compare(seq, outs, lambda cfg, o: fresh(make_context, t, cfg, o, memo))
    return outs

"""Closed-form load cycles through newton._load_history_loop on the CPU look-alikes (tests/plastic_exact_cases.py): the closed
forms against the many-digit return maps, the conditions on the histories, every look-alike against its closed form with the
recorded error re-measured, and the unloading steps that only converge at the loop's second attempt.  No GPU."""
import functools
from importlib import import_module

import numpy as np
import pytest

import plastic_exact_cases as pc

newton = import_module(pc.fep.__name__ + '.newton')
HISTORIES = [(case, model, name) for (case, model), names in pc.HISTORIES.items() for name in names]


@pytest.mark.parametrize('case,model,name', HISTORIES)
def test_histories_meet_their_conditions(case, model, name):
    rows = pc.check_history(case, model, name)
    assert len(rows) == len(pc.loads(case, model, name))
    if name == 'stall':                                                    # the step that stalled is the one the module names
        k = pc.STALL_STEP
        assert rows[k - 1]['plastic'] and rows[k - 1]['load'] < 0 and not rows[k]['plastic'] and rows[k]['load'] > rows[k - 1]['load']
        assert len(rows) == 21 and rows[-1]['ep'][3] == pytest.approx(0.0257756436972190, rel=1e-13)


def test_confined_compression_needs_a_material_that_yields():
    """The reference's Poisson's ratio never reaches the Mohr-Coulomb surface in confined compression; the case's own does, for
    both models."""
    s = pc.C_MATERIALS['mc'][2]
    assert 0.48 / (1 - 0.48) > (1 - s) / (1 + s) > pc.C_POISSON / (1 - pc.C_POISSON)
    assert all(pc.first_yield_pressure(m) > 0 for m in pc.MODELS['C'])


@pytest.mark.parametrize('case,model,name', HISTORIES)
def test_closed_form_is_the_many_digit_return_map(case, model, name):
    """One point of the model's 80-digit return map, driven with the closed form's strains and accepting every step: the
    stress and the state it carries are the closed form's to the bounds of the many-digit modules, and so are the branches."""
    e_s, e_p, labels, rows = pc.cross_check(case, model, name)
    b_s, b_p = pc.cross_check_bound(model, 's'), pc.cross_check_bound(model, 'ep')
    print(f'{case} {model} {name}: s {e_s:.2e} (<= {b_s:.2e})  state {e_p:.2e} (<= {b_p:.2e})')
    assert e_s <= b_s and e_p <= b_p
    plastic = {'vmi': lambda r: 1 + r['seg'], 'mc': lambda r: 2}.get(model, lambda r: 1)     # 'mc': the left edge
    assert labels == [plastic(r) if r['plastic'] else 0 for r in rows]


@functools.lru_cache(maxsize=None)
def _cpu_runs(case, model, t):
    """Every history and mesh size of the combination on the look-alike -> list of (name, size, problem, context, hist, rows)."""
    out = []
    for name in pc.HISTORIES[case, model]:
        rows = pc.exact(case, model, name)
        for size in pc.sizes(t):
            prob = pc.problem(case, t, size)
            ctx = pc.make_context(pc.lookalike(model), case, model, name, prob['elem'], prob['coord'], t)
            out.append((name, size, prob, ctx, pc.run(newton, ctx, prob, pc.loads(case, model, name)), rows))
    return out


@pytest.mark.parametrize('case,model,t', pc.CASES)
def test_lookalike_follows_the_closed_form(case, model, t):
    """Every history runs to its end; per step all points are plastic or none, as the closed form says; U and the plastic state
    of every step are the closed form's, and their largest error is the recorded figure."""
    e_u = e_p = 0.0
    for name, size, prob, ctx, hist, rows in _cpu_runs(case, model, t):
        assert hist['failed_at'] is None and len(hist['U']) == len(rows), (name, size, hist['failed_at'])
        n = prob['n_int']
        assert [a + b for a, b in hist['counts']] == [n * r['plastic'] for r in rows], (name, size)
        assert all(f.all() == f.any() == r['plastic'] for f, r in zip(hist['ind_p'], rows))
        assert all(b == 0 for _, b in hist['counts'])
        if model == 'mc':                                                  # every plastic point on the left edge (branch 2)
            assert [int(b[2]) for b in ctx.branches] == [n * r['plastic'] for r in rows]
            assert all(int(b[1]) + int(b[3]) + int(b[4]) == 0 for b in ctx.branches)
        u, p = pc.errors(case, hist, rows, prob['coord'])
        print(f'{case} {model} {t} {name} {size}: U {u:.2e}  state {p:.2e}  retries {hist["retries"]}')
        e_u, e_p = max(e_u, u), max(e_p, p)
    rec_u, rec_p = pc.PLASTIC_EXACT_CPU[case, model, t]
    assert e_u <= rec_u <= 2 * e_u + 1e-17, (e_u, rec_u)
    assert e_p <= rec_p <= 2 * e_p + 1e-17, (e_p, rec_p)


@pytest.mark.parametrize('case,model,t', pc.CASES)
def test_retries_only_where_an_elastic_step_follows_a_plastic_one(case, model, t):
    """The second attempt of a step (newton._load_history_loop) is reached only after the first has failed: a history without
    retries has made exactly the calls of its iterates and accepting calls, a retried step 25 + 1 + its second attempt's, and
    a retry happens only at an elastic step directly after a plastic one.  The 'stall' history is retried at step 13 on the
    meshes on which it used to end there, and nowhere else."""
    for name, size, prob, ctx, hist, rows in _cpu_runs(case, model, t):
        assert hist['n_calls'] == sum(hist['newton_its']) + len(rows)
        assert all(k > 0 and rows[k - 1]['plastic'] and not rows[k]['plastic'] for k in hist['retries']), hist['retries']
        assert all((hist['newton_its'][k] > 26) == (k in hist['retries']) for k in range(len(rows)))
        if name == 'stall':
            assert hist['retries'] == pc.RETRIES[t], (t, size, hist['retries'])
        if case == 'C':
            assert hist['retries'] == []


@pytest.mark.parametrize('model,t', pc.REFINED)
def test_refined_history_stays_on_the_closed_form(model, t):
    """The NumPy refinement and transfer in the middle of the history, on the look-alike: the transferred U is the step's
    linear field on the children (the parent's own error plus the per-entry bound of the transfer), every child point has a
    parent point's state bit for bit, the remaining steps run to the end on the closed form, and the error over both parts is
    the recorded figure."""
    r = pc.refined_cpu(newton, model, t)
    k = pc.REFINE_AFTER
    assert r['first']['failed_at'] is None and r['rest']['failed_at'] is None and r['rows'][k]['plastic']
    assert r['child']['elem'].shape[1] > r['prob']['elem'].shape[1] and (np.bincount(r['parent']) == 1).any()
    pc.check_child_state(t, r['parent'], r['first']['Ep'][-1], r['Ep_c'])
    Ux = pc.displacement('S', r['rows'][k], r['child']['coord'])
    parent_err = pc.errors('S', r['first'], r['rows'][:k + 1], r['prob']['coord'])[0]
    assert np.abs(r['U_c'] - Ux).max() <= (parent_err + pc.transfer_scale(t)) * np.abs(Ux).max()
    n = r['child']['n_int']
    assert [a + b for a, b in r['rest']['counts']] == [n * row['plastic'] for row in r['rows'][k + 1:]]
    e_u, e_p = pc.refined_errors(r)
    rec_u, rec_p = pc.PLASTIC_EXACT_REFINED_CPU[model, t]
    print(f'{model} {t}: U {e_u:.2e}  state {e_p:.2e}')
    assert e_u <= rec_u <= 2 * e_u + 1e-17 and e_p <= rec_p <= 2 * e_p + 1e-17


def test_a_failed_retry_ends_the_history(monkeypatch):
    """The loop's bookkeeping when the second attempt fails too: with an iteration that reports a stalled stopping quantity for
    the second load factor whatever it starts from, that step is attempted twice — the second time from the last accepted U
    plus the K_elast correction for the step's load — then named in both lists, and nothing after it runs."""
    prob = pc.problem('S', 'P1')
    ctx = pc.make_context(pc.lookalike('vm'), 'S', 'vm', 'cycle', prob['elem'], prob['coord'], 'P1')
    zetas = (0.5 * pc.PEAK, 0.7 * pc.PEAK, 0.2 * pc.PEAK)
    real, starts = newton._newton_iteration, []

    def stalls_at_the_second_factor(ops, K_elast, U_it, Ep, e0, rhs_of, hist, criterion, **kw):
        if np.abs(rhs_of(0 * U_it)).max() == pytest.approx(zetas[1] * np.abs(prob['f_ext']).max()):
            starts.append(np.array(U_it))
            return U_it, 25, 0.5
        return real(ops, K_elast, U_it, Ep, e0, rhs_of, hist, criterion, **kw)
    monkeypatch.setattr(newton, '_newton_iteration', stalls_at_the_second_factor)
    hist = pc.run(newton, ctx, prob, zetas)
    assert hist['failed_at'] == 1 and hist['retries'] == [1] and len(hist['U']) == 1 and len(starts) == 2
    U0 = hist['U'][0].flatten(order='F')
    assert np.array_equal(starts[0], U0)
    # both factors are elastic, so the elastic correction from the first factor's state is the second factor's solution
    # (to the standing 1e-13 of the array maximum)
    assert np.abs(starts[1] - U0 * (zetas[1] / zetas[0])).max() <= 1e-13 * np.abs(U0).max()


def test_a_nan_load_factor_fails_after_its_retry():
    """A NaN stopping quantity is a step that did not converge, like any other (on the GPU it is what a Krylov solve that broke
    down leaves): one iterate, the retry's step and its one iterate, then the history ends there."""
    prob = pc.problem('S', 'P1')
    ctx = pc.make_context(pc.lookalike('vm'), 'S', 'vm', 'cycle', prob['elem'], prob['coord'], 'P1')
    hist = pc.run(newton, ctx, prob, (0.5 * pc.PEAK, float('nan'), 0.2 * pc.PEAK))
    assert hist['failed_at'] == 1 and hist['retries'] == [1] and len(hist['U']) == 1
    assert hist['n_calls'] == hist['newton_its'][0] + 1 + 3

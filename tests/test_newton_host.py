"""
The load-step / Newton drivers without a GPU: `linear_solver='direct'` on the CPU oracle as hot path
(oracle_context.OracleContext through `context_factory`), against the traces recorded from the reference drivers.
What is pure host logic in newton.py — step control, stopping norms, extrapolation, what each flavour records — is
checked here; assertions and tolerances are those of tests/test_newton_gpu.py for the same traces.
"""
import numpy as np
import pytest

from conftest import load_golden, relerr
from oracle_context import OracleContext
from test_newton_gpu import _accepted


@pytest.mark.parametrize('t,n_steps,n_acc,n_calls,last_counts', [
    ('P1', 16, 16, 125, (599, 171)), ('Q1', 25, 24, 199, (700, 607)), ('Q2', 17, 16, 186, (986, 319)),
    ('P2', 13, 13, 130, (1718, 725))])
def test_dp_driver_on_oracle_vs_reference_trace(fep, t, n_steps, n_acc, n_calls, last_counts):
    g = load_golden(f'dp_{t.lower()}_level1_trace')
    assert len(g['zeta']) == n_steps and g['U_accepted'].shape[0] == n_acc and int(g['n_calls']) == n_calls
    acc = _accepted(g)
    h = fep.solve_strip_footing(t, level=1, linear_solver='direct', context_factory=OracleContext)
    assert len(h['zeta']) == n_acc == len(h['newton_its'])
    assert np.allclose(h['zeta'], g['zeta'][acc], rtol=0, atol=1e-15)           # same accepted load factors
    assert abs(h['n_calls'] - n_calls) <= (0 if t == 'P1' else 2), h['n_calls']  # (test_newton_gpu.py on the 2)
    if n_steps == n_acc:                                                        # no rejected attempt: every call is logged
        assert h['n_calls'] == sum(h['newton_its']) + n_acc
    for k in range(n_acc):
        assert relerr(h['U'][k], g['U_accepted'][k]) <= 1e-10, k
    assert np.array_equal(h['U_last'], h['U'][-1])
    pmax = np.abs(g['pressure']).max()
    for k, i in enumerate(acc):                                                 # pressure of step k is logged with k+1
        if i + 1 < len(g['pressure']):
            assert abs(h['pressure'][k] - g['pressure'][i + 1]) <= 1e-9 * pmax, k
    if t == 'P1':
        assert relerr(h['pressure'][14], 16.83867398886026) <= 1e-9             # SURVEY 8c pin (zeta = 0.52)
    assert h['counts'][-1] == tuple(g['counts'][-1]) == last_counts
    assert relerr(h['Ep'], g['Ep_final']) <= 1e-9
    assert h['pcg_iters'] is None


def test_tsx_p1_driver_on_oracle_vs_reference_replay(fep):
    g = load_golden('tsx')
    h = fep.solve_tsx_tunnel(g['coord'], g['elem'], 'P1', linear_solver='direct', context_factory=OracleContext)
    assert len(h['zeta']) == 17 and np.allclose(h['zeta'], g['p1_zeta'], rtol=0, atol=1e-15)
    assert h['n_plast'] == g['p1_nplast'].tolist() == [0] * 13 + [1, 1, 2, 3]
    assert relerr(h['F0'], g['p1_F0']) <= 1e-12
    assert relerr(h['U'][12], g['p1_U_step13']) <= 1e-10
    assert relerr(h['U'][-1], g['p1_U_final']) <= 1e-10
    assert abs(h['displ'][-1] - (-0.0019794496707526746)) <= 1e-10 * 0.0019794496707526746     # SURVEY 8c pin


def test_tsx_p2_driver_on_oracle_vs_reference_replay(fep):
    g = load_golden('tsx')
    tr = load_golden('tsx_p2_trace')
    h = fep.solve_tsx_tunnel(g['p2_coord'], g['p2_elem'], 'P2', linear_solver='direct', context_factory=OracleContext)
    assert len(h['zeta']) == 17 == len(tr['zeta']) and np.allclose(h['zeta'], tr['zeta'], rtol=0, atol=1e-15)
    assert h['n_plast'] == tr['nplast'].tolist() and h['n_plast'][-1] > 0
    assert h['n_calls'] == int(tr['n_calls'])
    assert relerr(h['F0'], tr['F0']) <= 1e-12
    for k, step in enumerate(tr['steps']):
        assert relerr(h['U'][int(step)], tr['U_steps'][k]) <= 1e-10, step
    assert np.abs(np.array(h['displ']) - tr['U_mon']).max() <= 1e-10 * np.abs(tr['U_mon']).max()


def test_driver_closes_ops_and_context_when_a_step_raises(fep):
    """An exception inside the loop must not leave the context (on the device: its buffers and the solver handle) open."""
    closed = []

    class Failing(OracleContext):
        calls = 0

        def step(self, *a, **k):
            Failing.calls += 1
            if Failing.calls == 3:                                              # K_elast, first iterate, then this one
                raise RuntimeError('step failed')
            return super().step(*a, **k)

        def close(self):
            closed.append(self)

    with pytest.raises(RuntimeError, match='step failed'):
        fep.solve_strip_footing('P1', n_cells=4, context_factory=Failing)
    assert len(closed) == 1

"""The cases of test_nonfinite_gpu.py (tests/nonfinite_cases.py) on the CPU restatements alone: each case has to reach what it
exists for, and the restatements themselves have to follow the rule the kernels are held to (a
non-finite value is never hidden, is contained, is reported promptly and leaves no trace).  A failure here blames the
generator or a restatement, before a GPU run meets the case.

Rule 1 on the restatements.  Von Mises and Mohr-Coulomb: a point whose trial strain has a NaN component is elastic, has the
elastic tangent and a NaN in its stress, and is counted nowhere (Mohr-Coulomb: only since the branch is chosen by !(f > 0);
with f <= 0 such a point fell through every comparison to the apex and came back with the finite stress c cos(phi) / sin(phi)).
Drucker-Prager keeps what the reference does, recorded here from the oracle: a NaN in a strain component gives an elastic
point with a NaN stress (a NaN in the shear strain alone is lost to the branch decision in the clamp of the squared norm,
DP:676, and such a point is judged by its volume change; point 0 is elastic by it), a +Inf in e[0] the apex with the finite
stress c / eta.  'vmi' (von Mises with isotropic hardening): the von Mises rule, with kappa as a fifth component of the trial
state; a NaN or an infinite kappa makes the point elastic with a NaN stress.  Its restatement's finiteness masks, settled here:
it is NaN in s[2] and in the shear entries of the tangent where only a normal strain, kappa or a material is poisoned (it
multiplies the zeros of (1, 1, 0, 1) and of 2 Dev G + Vol K by the poison), where the kernel's formulas s2 = 2G dv2, d02 = d12 =
0 are finite: it needs the structural-zero allowance of nonfinite_cases.masks_agree, as von Mises does and Mohr-Coulomb does not."""
import numpy as np
import pytest
import scipy.sparse as ssp
import scipy.sparse.linalg as sspl

import amg_ref
import nonfinite_cases as nf
import solver_cases as sc
from conftest import relerr_points
from oracle_context import OracleContext
from test_vcycle_gpu import _rhs


def _rule_1(model, r, bad, mats):
    assert not r['ind_p'][bad].any()
    assert np.isnan(r['s'][:, bad]).any(axis=0).all()
    # (within the per-point bound of DESIGN.md section 7, not bit for bit: Mohr-Coulomb's theta is 2G (r / r) where the in-plane
    # strains are finite, and (lam + 2G) - lam where they are not)
    assert relerr_points(r['ds'][:, bad], nf.elastic_tangent(model, [np.asarray(m)[bad] for m in mats])) <= nf.TOL_PT
    assert r['n_smooth'] + r['n_apex'] == int(r['ind_p'].sum()) == int(r['ind_p'][~bad].sum())    # counted nowhere


@pytest.mark.parametrize('model,k', nf.launch_ids())
def test_point_launches_reach_what_they_exist_for(model, k):
    c = nf.point_launch(model, k)
    n = nf.N_POINTS
    n_poisons = 2 if (model, k) == ('vmi', 2) else 6
    assert n == 3 * 256 + 1 and set(c['lanes']) == ({0, 63, 64, 255, 256, n - 1} if n_poisons == 6 else {255, 256})
    assert len(set(c['poisons'])) == len(c['lanes']) == n_poisons and set(sum(nf.LAUNCHES, ())) == set(nf.POISONS)
    assert nf.launches(model)[:2] == nf.LAUNCHES and len(nf.launches(model)) == (3 if model == 'vmi' else 2)
    assert len(c['lanes']) <= nf.MAX_POISONED_POINTS * n
    clean = np.ones(n, dtype=bool)
    clean[c['lanes']] = False
    assert (np.bincount(c['cls'][clean], minlength=3)[:2 if model in ('vm', 'vmi') else 3] > 0).all()
    if model == 'mc':
        from mc_ref import mc_return_map
        assert (np.bincount(mc_return_map(*c['clean'][:2], *c['clean'][2])['branch'][clean], minlength=5) > 0).all()
    (e, p, mats), (pe, pp, pm) = c['clean'], c['poisoned']
    for a, b in zip([e, p] + mats, [pe, pp] + pm):                           # the poison and nothing else
        assert np.array_equal(a[..., clean], b[..., clean])
    assert sum(int((~np.isfinite(a)).sum()) for a in [pe, pp] + pm) == n_poisons
    for accept in (False, True):
        good, bad = nf.restate(model, e, p, mats, None, accept), nf.restate(model, pe, pp, pm, None, accept)
        for key in ('s', 'ds', 'ind_p', 'ep'):                              # the restatement contains the poison (rule 2)
            if model == 'dp' and key != 'ind_p':
                # the oracle works on the compressed arrays of its smooth points, and their last bits move with the set
                assert relerr_points(bad[key][..., clean], good[key][..., clean]) <= 1e-14, key
            else:
                assert np.array_equal(good[key][..., clean], bad[key][..., clean]), key
        assert np.isfinite(good['s']).all() and np.isfinite(good['ds']).all()
        if model != 'dp':
            nan = nf.trial_strain_nan(pe, pp, model=model)
            assert not nan[clean].any() and nan.sum() == sum((arr in 'ep' and v != v) or (model == 'vmi' and (arr, row) == ('p', 3))
                                                             for arr, row, v in c['poisons'])
            _rule_1(model, bad, nan, pm)
            if model == 'vmi':                                              # a non-finite kappa leaves the column of ep as it went in
                assert np.array_equal(bad['ep'][:, nan], pp[:, nan], equal_nan=True)
    if model == 'vmi':                                                      # the restatement's finiteness masks (module docstring)
        bad = nf.restate(model, pe, pp, pm)
        for lane, (arr, row, val) in zip(c['lanes'], c['poisons']):
            if (arr, row) in (('e', 0), ('e', 1), ('p', 0), ('p', 3)):      # the shear strain itself is finite
                kernel_s2 = 2 * pm[0][lane] * ((pe[2, lane] - pp[2, lane]) / 2)
                assert np.isnan(bad['s'][2, lane]) and np.isfinite(kernel_s2)
                assert not nf.masks_agree('mc', {'s': np.where(np.arange(4) == 2, kernel_s2, bad['s'][:, lane]).reshape(4, 1)},
                                          {'s': bad['s'][:, [lane]]}, 's')[0]
                assert nf.masks_agree(model, {'s': np.where(np.arange(4) == 2, kernel_s2, bad['s'][:, lane]).reshape(4, 1)},
                                      {'s': bad['s'][:, [lane]]}, 's')[0]
            if arr == 'm' and row in (0, 1):                                # 2 Dev G + Vol K: the zeros of Dev and Vol times NaN
                assert np.isnan(bad['ds'][[2, 5, 6, 7], lane]).all()
    if model in ('vm', 'vmi'):                                              # nonfinite_cases.vm_infinite: the restatement's side
        odd, bad = nf.vm_infinite(model, pe, pp), nf.restate(model, pe, pp, pm)
        assert odd.sum() == sum(arr == 'e' and abs(v) == nf.INF for arr, _, v in c['poisons']) and not odd[clean].any()
        assert not bad['ind_p'][odd].any() and np.isnan(bad['s'][:, odd]).all() and np.isfinite(bad['ds'][:, odd]).all()
    if model == 'dp':                                                       # the reference's behaviour, as the oracle pins it
        bad = nf.restate(model, pe, pp, pm)
        for lane, (arr, row, val) in zip(c['lanes'], c['poisons']):
            s = bad['s'][:, lane]
            if arr == 'e' and val != val:
                assert not bad['ind_p'][lane] and np.isnan(s).any()
            elif arr == 'e' and val == nf.INF:
                assert bad['ind_p'][lane] and np.array_equal(s, np.array([1, 1, 0, 1]) * (pm[3][lane] / pm[2][lane]))
                assert not bad['ds'][:, lane].any()


@pytest.mark.parametrize('model', nf.MODELS)
def test_a_nan_initial_strain_poisons_every_point(model):
    e, p, mats = nf.point_launch(model, 0)['clean']
    for row in range(4):
        e0 = np.array([1e-5, -2e-5, 3e-5, 1e-5])
        e0[row] = nf.NAN
        assert nf.trial_strain_nan(e, p, e0, model=model).all()
        for accept in (False, True):
            r = nf.restate(model, e, p, mats, e0, accept)
            if model != 'dp':
                _rule_1(model, r, np.ones(nf.N_POINTS, dtype=bool), mats)
                assert np.array_equal(r['ep'], p)


def test_the_structural_zeros_are_the_only_disagreement_allowed():
    """masks_agree: equal finiteness passes for every model; a kernel that is finite where the restatement is not passes in the
    shear entries of Drucker-Prager and von Mises alone; a kernel that is non-finite where the restatement is finite never."""
    ref = {'s': np.ones((4, 3)), 'ds': np.ones((9, 3))}
    ref['s'][:, 1] = ref['ds'][:, 1] = nf.NAN
    for model in nf.MODELS:
        for key, shear in (('s', nf.SHEAR_S), ('ds', nf.SHEAR_DS)):
            assert nf.masks_agree(model, ref, ref, key)[0]
            for row in range(ref[key].shape[0]):
                got = {key: ref[key].copy()}
                got[key][row, 1] = 1.0
                assert nf.masks_agree(model, got, ref, key)[0] == (model != 'mc' and row in shear), (model, key, row)
                got = {key: ref[key].copy()}
                got[key][row, 0] = nf.INF
                assert not nf.masks_agree(model, got, ref, key)[0]


@pytest.mark.parametrize('t', nf.msc.TYPES)
def test_a_nan_kappa_in_a_mesh_step_reaches_what_it_exists_for(t):
    """The 'kappa' kind of 'vmi': one point of one interior element, a clean strain everywhere; on the restatement the point is
    elastic with the elastic tangent and a NaN stress, F is NaN at the DOFs of that element alone and K finite, changed at most
    in that element's blocks."""
    c = nf.mesh_case('vmi', t, 'kappa')
    k, nq = c['k'], nf.msc.NQ[t]
    assert c['points'].sum() == 1 and c['points'][k] and c['elements'].sum() == 1 and c['elements'][k // nq]
    assert np.array_equal(c['U_bad'], c['U']) and np.isnan(c['ep_bad'][3, k]) and np.isnan(c['ep_bad']).sum() == 1
    assert np.array_equal(np.delete(c['ep_bad'], k, axis=1), np.delete(c['ep'], k, axis=1))
    lo, hi = c['coord'].min(axis=1, keepdims=True), c['coord'].max(axis=1, keepdims=True)
    xy = c['coord'][:, c['elem'][:, k // nq]]
    assert ((xy > lo) & (xy < hi)).all()                                    # an interior element
    ref = nf.elem_ref(c, t)
    E, _ = ref.strain(c['U'])
    assert nf.trial_strain_nan(E, c['ep_bad'], c['e0'], model='vmi').sum() == 1
    good = nf.restate('vmi', E, c['ep'], c['mats'], c['e0'], curve=c['curve'])
    for accept in (False, True):
        r = nf.restate('vmi', E, c['ep_bad'], c['mats'], c['e0'], accept, curve=c['curve'])
        _rule_1('vmi', r, c['points'], c['mats'])
        assert np.array_equal(r['ind_p'][~c['points']], good['ind_p'][~c['points']])
        assert np.isnan(r['s'][[0, 1, 3], k]).all() and np.array_equal(r['ep'][:, k], c['ep_bad'][:, k], equal_nan=True)
        for key in ('s', 'ds'):
            assert np.array_equal(r[key][:, ~c['points']], good[key][:, ~c['points']])
    with np.errstate(invalid='ignore'):
        K, _, F, _ = ref.assemble(r['ds'], r['s'])
    assert np.array_equal(np.isnan(F), c['dofs']) and np.isfinite(K).all()
    dirty = nf.dirty_entries(c, ref.pattern())
    Kc, _, _, _ = ref.assemble(good['ds'], None)
    assert np.array_equal(K[~dirty], Kc[~dirty])


@pytest.mark.parametrize('model,t,kind', [c for c in nf.model_mesh_cases() if c[2] != 'kappa'])
def test_mesh_cases_reach_what_they_exist_for(model, t, kind):
    c = nf.mesh_case(model, t, kind)
    assert c['ep_bad'] is c['ep']
    elem, n_e = c['elem'], c['elem'].shape[1]
    assert n_e == 257 and (n_e * nf.msc.NQ[t]) % 256 == nf.msc.NQ[t]
    n_dirty = int(c['elements'].sum())
    assert 1 <= n_dirty <= nf.MAX_DIRTY_ELEMENTS * n_e
    assert (n_dirty >= 3) if kind == 'vertex' else n_dirty == {'midside': 2, 'interior': 1}[kind]
    assert np.array_equal(c['elements'], (elem == c['k']).any(axis=0)) and np.isnan(c['U_bad'][:, c['k']]).all()
    assert np.array_equal(np.isnan(c['U_bad']), np.isnan(c['U_bad']) & (np.arange(c['coord'].shape[1]) == c['k']))
    ref = nf.elem_ref(c, t)
    E, _ = ref.strain(c['U_bad'])
    assert np.array_equal(np.isnan(E), np.broadcast_to(c['points'], E.shape)) and np.isfinite(E[:, ~c['points']]).all()
    E_clean, _ = ref.strain(c['U'])
    assert np.array_equal(E[:, ~c['points']], E_clean[:, ~c['points']])
    good = nf.restate(model, E_clean, c['ep'], c['mats'], c['e0'], curve=c['curve'])
    r = nf.restate(model, E, c['ep'], c['mats'], c['e0'], curve=c['curve'])
    _rule_1(model, r, c['points'], c['mats'])
    assert np.array_equal(r['ind_p'][~c['points']], good['ind_p'][~c['points']])
    assert np.isnan(r['s'][:, c['points']]).all()
    with np.errstate(invalid='ignore'):
        K, _, F, _ = ref.assemble(r['ds'], r['s'])
    assert np.array_equal(np.isnan(F), c['dofs']) and np.isfinite(F[~c['dofs']]).all() and np.isfinite(K).all()
    # the dirty blocks are those of the dirty elements' node pairs, the dirty entries their 2 x 2 CSR entries
    dirty = nf.dirty_entries(c, ref.pattern())
    assert dirty.sum() == 4 * c['blocks'].size and 0 < dirty.mean() < 0.2
    Kc, _, _, _ = ref.assemble(good['ds'], None)
    assert np.array_equal(K[~dirty], Kc[~dirty])                            # K changes where a dirty point's tangent went in
    assert not np.array_equal(K[dirty], Kc[dirty]) or not good['ind_p'][c['points']].any()


@pytest.mark.parametrize('name', nf.solver_names())
def test_solver_poisons_break_down_or_are_never_read(name):
    assert nf.solver_names() == ('orphans-P1', 'tsx-P1') and len(sc.CASES[name]['nodes']) >= 2
    Ks, (n_s, n_a, n_int) = sc.oracle_matrices(name)
    assert 0 < n_s + n_a < n_int
    K, qf = Ks['plastic'], sc.free_dofs(name)
    b = _rhs(qf)['random']
    levels = sc.hierarchy(name, Ks['elastic'])
    refresh = sc.CASES[name]['refresh']
    direct = sspl.spsolve(K[qf][:, qf].tocsc(), b[qf])
    for which in nf.SOLVER_POISONS:
        data, rhs = nf.solver_poison(K, b, qf, which)
        Kb = ssp.csr_matrix((data, K.indices, K.indptr), shape=K.shape)
        assert int(np.isnan(data).sum()) + int(np.isnan(rhs).sum()) >= 1
        if which in 'ab':
            with np.errstate(all='ignore'):
                for M, cg in ((amg_ref.block_jacobi(Kb, qf), amg_ref.pcg_single_reduction),
                              (amg_ref.VCycle(Kb, qf, levels, refresh=refresh), amg_ref.pcg),
                              (amg_ref.VCycle(Kb, qf, levels, refresh=False), amg_ref.pcg)):
                    r = cg(Kb, qf, rhs, M, max_iter=nf.MAX_ITER, rtol=1e-10)
                    assert r['state'] == 2 and r['iters'] == 0 and not r['x'].any(), (which, r['state'], r['iters'])
        else:                                                               # the host path never reads those entries
            assert np.array_equal(Kb[qf][:, qf].toarray(), K[qf][:, qf].toarray()) and np.array_equal(rhs[qf], b[qf])
            assert np.array_equal(sspl.spsolve(Kb[qf][:, qf].tocsc(), rhs[qf]), direct)


def test_the_load_step_loop_recovers_from_a_failed_solve_on_the_oracle(fep, monkeypatch):
    """linear_solver='direct' on the CPU oracle: the first solve of the second load step returns NaN, the step is halved
    (DP:1076, DP:1117) and the run goes on to zeta_max with the sequence the GPU variants are held to."""
    kw = dict(nf.FOOTING, linear_solver='direct', context_factory=OracleContext)
    clean = fep.solve_strip_footing(**kw)
    k = 1 + clean['newton_its'][0] + 1
    calls = nf.failing_solve(monkeypatch, k)
    bad = fep.solve_strip_footing(**kw)
    assert calls[0] > k
    nf.check_recovery(clean, bad, nf.FOOTING['zeta_max'])
    assert bad['counts'][-1][0] + bad['counts'][-1][1] > 0                   # the run ends in the plastic regime
    assert bad['n_calls'] > clean['n_calls'] - 25

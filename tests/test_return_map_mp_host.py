"""The fixtures of the high-precision reference (tests/return_map_mp.py, tests/golden/make_golden_return_map_mp.py) and the
float64 restatements against them, on the CPU: the generator reproduces the committed files bit for bit on a sample of every
family, the restatements' errors are the table of DESIGN.md section 7 (return_map_mp_cases.MEASURED), from which the bounds
of the GPU tests derive, and labels and counters agree outside family E."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT  # noqa: F401
from mc_ref import mc_return_map
from return_map_mp_cases import FAMILIES, MEASURED, check, check_flags, errors, fixture, groups, merge
from vm_ref import vm_return_map

sys.path.insert(0, GOLDEN)
MODELS = ('mc', 'vm', 'dp')


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def restatement(model, fix, idx, e0):
    """The float64 restatement of the model on the points idx, accepting -> dict s, ds, ep, ind_p, n_smooth, n_apex."""
    e, p = fix['e'][:, idx], fix['p'][:, idx].copy()
    mats = [fix[k][idx] for k in ('G', 'K', 'm3', 'm4')]
    with np.errstate(all='ignore'):
        if model == 'mc':
            return mc_return_map(e, p, *mats, apply_plastic_strain=True, e0=e0)
        if model == 'vm':
            r = vm_return_map(e, p, *mats, apply_plastic_strain=True, e0=e0)
            return dict(r, n_smooth=r['n_plast'], n_apex=0)
        from oracle import fep_oracle as orc
        z = np.zeros((4, 1)) if e0 is None else e0
        r = orc.return_map(e.copy(), p, *mats, True, e0=z, tsx=True)
        return dict(r, ep=p)


def measure(model):
    fix = fixture(model)
    errs = {}
    for idx, e0 in groups(fix):
        errs = merge(errs, errors(model, fix, restatement(model, fix, idx, e0), idx))
    return errs


@pytest.mark.parametrize('model', MODELS)
def test_restatement_errors_are_the_recorded_table(model):
    """Every figure of the table is reproduced (within its rounding up to two digits), and eight times each of them, capped by
    the standing bounds, holds for the restatement itself."""
    errs = measure(model)
    for k, (wide, pt) in sorted(errs.items()):
        print(model, *k, f'{wide:.2e} {pt:.2e}', MEASURED[model][k])
        assert wide <= MEASURED[model][k][0] <= 2 * wide + 1e-17 and pt <= MEASURED[model][k][1] <= 2 * pt + 1e-17, k
    assert set(errs) == set(MEASURED[model])
    check(model, errs)


@pytest.mark.parametrize('model', MODELS)
def test_restatement_labels_and_counters(model):
    fix = fixture(model)
    for idx, e0 in groups(fix):
        r = restatement(model, fix, idx, e0)
        check_flags(model, fix, idx, r)
        if model == 'mc':
            keep = fix['family'][idx] != FAMILIES.index('E')
            assert np.array_equal(r['branch'][keep], fix['label'][idx][keep])


@pytest.mark.parametrize('model', MODELS)
def test_generator_reproduces_the_fixtures(model):
    """The inputs of every family but E entirely and two pairs per boundary of E (the bisection runs on the reference), and
    the reference itself at 64 points spread over all families: bit for bit."""
    import make_golden_return_map_mp as gen
    fix = fixture(model)
    inp = gen.INPUTS[model](n_pairs=2)
    fam_new, fam_old = inp['family'], fix['family']
    for f in range(len(FAMILIES)):
        new, old = np.flatnonzero(fam_new == f), np.flatnonzero(fam_old == f)
        if FAMILIES[f] == 'E':
            n_bound = old.size // (2 * gen.N_PAIRS)
            old = old.reshape(n_bound, -1)[:, :4].ravel()
        assert new.size == old.size
        for k in ('e', 'p', 'with_e0', 'G', 'K', 'm3', 'm4'):
            assert _bits(inp[k][..., new]) == _bits(fix[k][..., old]), (FAMILIES[f], k)
    assert np.array_equal(inp['e0'], fix['e0']) and list(inp['names_C']) == list(fix['names_C'])
    idx = np.unique(np.concatenate([np.flatnonzero(fam_old == f)[np.linspace(0, (fam_old == f).sum() - 1, 16).astype(int)]
                                    for f in np.unique(fam_old)]))[:64]
    out = gen.outputs(model, fix, idx)
    for k in gen.OUTPUT_KEYS:
        assert _bits(out[k]) == _bits(fix[k][..., idx]), k
    gen.check_conditions(model, fix)

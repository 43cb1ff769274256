"""Shared by test_return_map_mp_host.py and test_return_map_mp_gpu.py: the fixtures of tests/golden/make_golden_return_map_mp.py
(read only; this module does not import the high-precision reference), the error measures per family and output, and the
bounds of DESIGN.md section 7.

A bound is eight times the error of the float64 restatement of the law (tests/mc_ref.py, tests/vm_ref.py, the pinned
Drucker-Prager oracle) against the fixtures, MEASURED below as test_return_map_mp_host.py reproduces it, and never more than
the project's standing bounds: 1e-13 of the array maximum and 1e-12 per point in the families A, B, C, 5e-12 per point in D
(whose arrays span seventeen decades: no array-wide bound).  The fixtures are themselves rounded to float64, so no error is
resolved below the unit roundoff 2^-53: a measured figure counts as at least that.  `ds` of a Mohr-Coulomb face point is
a quotient by r: its per-point error is divided by max(1, R_FLOOR / r_rel) before it is compared.  Family E (pairs one ulp
apart across a branch boundary) compares the stress alone, and its flags not at all."""
import functools

import numpy as np

from conftest import load_golden

FAMILIES = 'ABCDE'
R_FLOOR = 1e-2                                                          # tests/mc_cases.py
MARGIN = 8.0
UNIT = 2.0 ** -53
STANDING = {'A': (1e-13, 1e-12), 'B': (1e-13, 1e-12), 'C': (1e-13, 1e-12), 'D': (None, 5e-12), 'E': (1e-13, 1e-12)}
KEYS = ('s', 'ds', 'ep')
APEX = {'mc': 4, 'vm': -1, 'dp': 2}                                     # the label that counts[1] counts

# (array-wide, per point) errors of the restatements, rounded up to two digits: the table of DESIGN.md section 7
MEASURED = {
    'mc': {
        ('A', 'ds'): (3.4e-16, 1.1e-15),
        ('A', 'ep'): (6.6e-16, 5.4e-14),
        ('A', 's'): (3.9e-16, 2.1e-15),
        ('B', 'ds'): (3.4e-16, 8.9e-16),
        ('B', 'ep'): (1.8e-16, 1.2e-14),
        ('B', 's'): (1.3e-16, 1.5e-15),
        ('C', 'ds'): (1.7e-16, 6.2e-16),
        ('C', 'ep'): (2.7e-16, 7.5e-15),
        ('C', 's'): (1.5e-16, 3.9e-15),
        ('D', 'ds'): (1.2e-16, 6.4e-13),
        ('D', 'ep'): (1.5e-16, 2.6e-15),
        ('D', 's'): (2.0e-16, 3.2e-15),
        ('E', 's'): (1.6e-16, 1.7e-15),
    },
    'vm': {
        ('A', 'ds'): (2.2e-16, 3.4e-16),
        ('A', 'ep'): (7.2e-16, 6.8e-15),
        ('A', 's'): (1.6e-16, 6.1e-16),
        ('C', 'ds'): (1.1e-16, 1.8e-16),
        ('C', 'ep'): (1.3e-16, 3.7e-16),
        ('C', 's'): (7.2e-17, 3.9e-15),
        ('D', 'ds'): (2.1e-16, 6.1e-16),
        ('D', 'ep'): (1.5e-16, 7.7e-16),
        ('D', 's'): (1.5e-16, 2.1e-15),
        ('E', 's'): (1.3e-16, 2.2e-16),
    },
    'dp': {
        ('A', 'ds'): (2.6e-16, 7.0e-16),
        ('A', 'ep'): (1.8e-16, 2.5e-15),
        ('A', 's'): (2.4e-16, 7.0e-15),
        ('C', 'ds'): (1.7e-16, 4.4e-16),
        ('C', 'ep'): (4.4e-23, 3.6e-16),
        ('C', 's'): (1.3e-17, 3.1e-16),
        ('D', 'ds'): (2.0e-16, 2.4e-15),
        ('D', 'ep'): (1.4e-16, 1.4e-15),
        ('D', 's'): (1.1e-16, 5.8e-15),
        ('E', 's'): (4.5e-16, 5.4e-15),
    },
}


@functools.lru_cache(maxsize=None)
def fixture(model):
    g = load_golden(f'return_map_mp_{model}')
    fix = {k: g[k] for k in g.files}
    for v in fix.values():
        v.setflags(write=False)
    return fix


def groups(fix):
    """The two launches: (indices, e0 or None) of the points without and with the initial strain."""
    w = fix['with_e0']
    return (np.flatnonzero(~w), None), (np.flatnonzero(w), fix['e0'].reshape(4, 1))


def errors(model, fix, got, idx):
    """got: dict s, ds, ep of the points idx -> {(family, key): (array-wide, per point)} of those points; ds without the
    `no_tangent` points, a Mohr-Coulomb face's per-point error of ds over its amplification; family E: s alone."""
    out = {}
    fam = fix['family'][idx]
    for f in np.unique(fam):
        name = FAMILIES[f]
        for key in (('s',) if name == 'E' else [k for k in KEYS if k in got]):
            sel = fam == f
            if key == 'ds':
                sel = sel & ~fix['no_tangent'][idx]
            if not sel.any():
                continue
            a, b = np.asarray(got[key])[:, sel], fix[key][:, idx[sel]]
            d, s = np.abs(a - b).max(axis=0), np.abs(b).max(axis=0)
            pt = np.where(s > 0, d / np.where(s > 0, s, 1.0), d)
            if key == 'ds' and model == 'mc':
                r_rel = np.maximum(fix['r_rel'][idx[sel]], 1e-300)
                pt = pt / np.where(fix['label'][idx[sel]] == 1, np.maximum(1.0, R_FLOOR / r_rel), 1.0)
            out[name, key] = (float(d.max() / max(s.max(), 1e-300)), float(pt.max()))
    return out


def merge(a, b):
    return {k: tuple(max(x, y) for x, y in zip(a.get(k, (0.0, 0.0)), b.get(k, (0.0, 0.0)))) for k in set(a) | set(b)}


def bound(model, family, key):
    """(array-wide or None, per point)"""
    wide, pt = (max(v, UNIT) for v in MEASURED[model][family, key])
    s_wide, s_pt = STANDING[family]
    return (None if s_wide is None else min(MARGIN * wide, s_wide)), min(MARGIN * pt, s_pt)


def check(model, errs):
    """Prints every figure, then asserts all of them."""
    bad = []
    for (family, key), (wide, pt) in sorted(errs.items()):
        b_wide, b_pt = bound(model, family, key)
        print(f'{model} {family} {key:2s} array-wide {wide:.2e} (<= {b_wide})  per point {pt:.2e} (<= {b_pt:.2e})')
        if (b_wide is not None and not wide <= b_wide) or not pt <= b_pt:
            bad.append((family, key, wide, pt))
    assert not bad, bad


def check_flags(model, fix, idx, got):
    """ind_p of every point outside family E, and both counters: equal to the labels' where the launch has no point of
    family E; otherwise a point of E may sit on either side, so the counters add up to the call's own ind_p and the apex counter
    exceeds the other families' by at most the points of E that have the apex on one side."""
    lab = fix['label'][idx]
    keep = fix['family'][idx] != FAMILIES.index('E')
    apex = APEX[model]
    assert np.array_equal(np.asarray(got['ind_p'])[keep], (lab != 0)[keep])
    n_smooth, n_apex = int(((lab != 0) & (lab != apex) & keep).sum()), int(((lab == apex) & keep).sum())
    if keep.all():
        assert (got['n_smooth'], got['n_apex']) == (n_smooth, n_apex)
    else:
        pairs = lab[~keep].reshape(-1, 2)
        assert got['n_smooth'] + got['n_apex'] == int(np.asarray(got['ind_p']).sum())
        assert 0 <= got['n_apex'] - n_apex <= 2 * int((pairs == apex).any(axis=1).sum())

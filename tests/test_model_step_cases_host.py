"""The cases of test_model_step_routes_gpu.py (tests/model_step_cases.py) on the CPU restatements alone: every case is
built, stepped on VMRefContext / MCRefContext / VMIRefContext, and has to meet the conditions the GPU module relies on — few
points near a branch boundary, a von Mises plastic share between 0.2 and 0.8, every Mohr-Coulomb branch populated, on the
multi-segment curves of 'vmi' every segment accepted, a breakpoint crossed and the softening segment reached, reversed
elements where the mesh exists for them, and the block-edge meshes at their residues.  A failure here blames the generator.
Adding a model leaves the cases of the others as they were: OLD_CASES holds digests of one case per model and type."""
import hashlib

import numpy as np
import pytest

import model_step_cases as cases
from elem_ref import ElemRef
from mc_ref import MCRefContext
from vm_ref import VMRefContext
from vmi_ref import VMIRefContext

GRID = [(m, t, n) for m in cases.MODELS for t in cases.TYPES for n in cases.names(t)]
# The cases whose first state misses a condition, and the draw they take instead (model_step_cases.build).  Mohr-Coulomb P1
# `renumbered`: uniform materials and a compressive initial strain leave one of its 1152 points at the apex, three are asked.
# 'vmi' Q1 `strip1`: at 1.5 yield radii the step from kappa = 0 has a plastic share of 0.8016, 0.8 is the most allowed.
# Every other case takes its first draw: a drift of the generator shows here and is not absorbed by a redraw.
LATER_DRAW = {('mc', 'P1', 'renumbered'): 1, ('vmi', 'Q1', 'strip1'): 1}
# sha256 (first 16 hex digits) of elem, coord, U, ep, e0, the four materials, accept and draw of one case per model and type,
# recorded on the commit before 'vmi' joined MODELS
OLD_CASES = {('vm', 'P1', 'strip2'): 'a75bc4c6bead33d2', ('vm', 'P2', 'curved'): '6f219ef97cb9ecc5',
             ('vm', 'Q1', 'block257'): '2e92d97a56994d34', ('vm', 'Q2', 'strip2'): 'b362c240b87cd174',
             ('vm', 'P4', 'mixed'): 'b0e075c160434daa', ('mc', 'P1', 'strip2'): '78593111562a71f7',
             ('mc', 'P2', 'curved'): 'bf0fdec3ebfcaedf', ('mc', 'Q1', 'block257'): 'caea1b14c626bbd2',
             ('mc', 'Q2', 'strip2'): '78759221be35e8e1', ('mc', 'P4', 'mixed'): 'b2028c79ff2f0b7f'}


def test_the_grid_covers_every_combination_of_the_state():
    for m in cases.MODELS:
        assert {cases.flags(t, n) for mm, t, n in GRID if mm == m} == {(a, b, c) for a in (False, True) for b in (False, True)
                                                                      for c in (False, True)}
    assert cases.MODELS == ('vm', 'mc', 'vmi') and len(cases.cases()) == 3 * (3 * 10 + 2 * 10 + 2 * 9 + 2 * 9 + 2 * 10)
    assert len({cases.seed(*c) for c in GRID}) == len(GRID)


def test_every_type_meets_all_five_curves():
    for t in cases.TYPES:
        ids = [cases.curve_id('vmi', t, n) for n in cases.names(t)]
        assert set(ids) == {0, 1, 2, 3, None}, (t, ids)
        for n in cases.names(t):
            crv = cases.build('vmi', t, n)['curve'] if n == 'block257' else cases.curve_of('vmi', t, n)
            c = cases.curve_id('vmi', t, n)
            assert (crv is None) == (c is None)
            if crv is not None:
                assert len(crv[0]) == {0: 1, 1: 1, 2: 8, 3: 4}[c] and (crv[1] < 0).any() == (c == 3) and (crv[1] != 0).any() == (c != 0)
    assert all(cases.curve_id(m, t, n) is None and cases.curve_of(m, t, n) is None for m, t, n in GRID if m != 'vmi')
    # the block-edge meshes (a partial last workgroup) run on a multi-segment curve for at least one type each
    for n in ('block256', 'block257', 'block255'):
        assert {cases.curve_id('vmi', t, n) for t in cases.TYPES} & {2, 3}, n


def _digest(c):
    h = hashlib.sha256()
    for k in ('elem', 'coord', 'U', 'ep', 'e0'):
        h.update(b'none' if c[k] is None else np.ascontiguousarray(c[k]).tobytes())
    for m in c['mats']:
        h.update(np.ascontiguousarray(m, dtype=np.float64).tobytes())
    h.update(bytes([c['accept'], c['draw']]))
    return h.hexdigest()[:16]


@pytest.mark.parametrize('model,t,name', sorted(OLD_CASES))
def test_cases_of_the_other_models_are_what_they_were(model, t, name):
    assert {(m, tt) for m, tt, _ in OLD_CASES} == {(m, tt) for m in ('vm', 'mc') for tt in cases.TYPES}
    c = cases.build(model, t, name)
    assert c['curve'] is None and _digest(c) == OLD_CASES[model, t, name]


@pytest.mark.parametrize('model,t,name', GRID)
def test_case_meets_its_conditions_on_the_restatement(model, t, name):
    c = cases.build(model, t, name)
    again = cases.build(model, t, name)                                     # the same case for every route
    assert all(np.array_equal(c[k], again[k]) for k in ('elem', 'coord', 'U', 'ep')) and c['accept'] == again['accept']
    assert c['draw'] == LATER_DRAW.get((model, t, name), 0)
    elem, coord = c['elem'], c['coord']
    ctx = {'vm': VMRefContext, 'mc': MCRefContext, 'vmi': VMIRefContext}[model](elem, coord, *cases.fep.element_tables(t))
    crv = c['curve']
    assert (crv is None) == (cases.curve_id(model, t, name) is None)
    if crv is not None:
        ctx.set_hardening(*crv)
    n = ctx.n_int
    assert n <= 5000 and c['ep'].shape == (4, n)
    ctx.set_materials(*c['mats'])
    ep = c['ep'].copy()
    ref = ctx.step(c['U'], ep, e0=c['e0'], apply_plastic_strain=c['accept'])
    assert np.array_equal(ep, c['ep']) == (not c['accept'])
    # the context's flags are the restatement's on the context's strain
    r = cases.return_map(model, ref['E'], c['ep'], c['mats'], c['e0'], False, crv)
    assert np.array_equal(r['ind_p'], ref['ind_p']) and (r['n_smooth'], r['n_apex']) == (ref['n_smooth'], ref['n_apex'])
    excl = cases.excluded(model, r, c['mats'], crv)
    print(model, t, name, 'n_int', n, 'excluded', int(excl.sum()), 'plastic share', round(float(r['ind_p'].mean()), 3),
          'per branch', np.bincount(r['branch'], minlength=5))
    if model == 'vmi':
        p = r['ind_p']
        print('curve', cases.curve_id(model, t, name), 'per segment', np.bincount(r['seg'][p], minlength=1),
              'crossed', int((r['seg'][p] > r['seg0'][p]).sum()))
        if c['accept']:                                                     # kappa_new is the kappa the accepting step leaves
            assert np.array_equal(ep[3], np.where(p, r['kappa_new'], c['ep'][3]))
    cases.check_conditions(model, r, excl, crv)
    # without a previous plastic strain (the ep = None step of the GPU module) the case keeps its conditions as well
    r0 = cases.return_map(model, ref['E'], None, c['mats'], c['e0'], False, crv)
    cases.check_conditions(model, r0, cases.excluded(model, r0, c['mats'], crv), crv)
    if name == 'mixed':
        assert (ElemRef(elem, coord, cases.fep.element_tables(t)).det() < 0).mean() > 0.3
    if name.startswith('block'):
        n_e = int(name[5:])
        assert elem.shape[1] == n_e
        assert n % cases.BLOCK == {256: 0, 257: cases.NQ[t], 255: cases.BLOCK - cases.NQ[t]}[n_e]

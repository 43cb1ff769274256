"""The three return-map kernels against the fixtures of the high-precision reference (tests/golden/return_map_mp_*.npz, read
through return_map_mp_cases.py; the reference itself is not imported here), per point, and the step of a Mohr-Coulomb context
in a nearly hydrostatic state against the elastic stiffness.  Bounds: DESIGN.md section 7 (return_map_mp_cases.bound).

The sum of the per-workgroup branch counters (counts_reduce_kernel, sum_block_counts) at its loop edges: the three device
entry points at 1024 * 256 + 1 and 8192 * 256 + 1 points, tiled from 1000.

The initial strain is one vector per call, so a fixture is two launches: its points without e0 (families A to E, several
256-thread workgroups and a partial last one) and those with it."""
import ctypes

import numpy as np
import pytest

from conftest import relerr, relerr_points, relerr_rows
from mc_cases import COHESION, SIN_PHI, YOUNG
from mc_ref import MCRefContext
from meshes import jitter, rect
from model_ref import DEV_ENTRY, dev_return_map
from nonfinite_cases import thousand as _thousand
from return_map_mp_cases import check, check_flags, errors, fixture, groups, merge
from test_mc_gpu import MESHES, TOL_K, TOL_K_ROW

pytestmark = pytest.mark.gpu

def _host(fep, model, e, p, e0, mats, accept):
    if model == 'dp':
        r = (fep.construct_constitutive_problem(e, p, *mats, apply_plastic_strain=accept) if e0 is None else
             fep.construct_constitutive_problem_tsx(e, e0, p, *mats, apply_plastic_strain=accept))
        return r
    if model == 'vm':
        r = fep.construct_constitutive_problem_vm(e, p, *mats, apply_plastic_strain=accept, e0=e0)
        return dict(r, n_smooth=r['n_plast'], n_apex=0)
    return fep.construct_constitutive_problem_mc(e, p, *mats, apply_plastic_strain=accept, e0=e0)


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('model', ['dp', 'vm', 'mc'])
def test_kernels_against_the_high_precision_fixtures(fep, model, order):
    fix = fixture(model)
    errs = {}
    for idx, e0 in groups(fix):
        n = idx.size
        assert n > 256 and n % 256 != 0
        e, p = fix['e'][:, idx], fix['p'][:, idx]
        ev = np.asfortranarray(e) if order == 'F' else np.ascontiguousarray(e)
        mats = [np.ascontiguousarray(fix[k][idx]) for k in ('G', 'K', 'm3', 'm4')]
        for accept in (False, True):
            ph = p.copy()
            host = _host(fep, model, ev, ph, e0, mats, accept)
            dev = dev_return_map(fep, model, e, order, p, e0, mats, accept)
            for got, ep in ((host, ph), (dev, dev['ep'])):
                check_flags(model, fix, idx, got)
                if accept:
                    errs = merge(errs, errors(model, fix, dict(s=got['s'], ds=got['ds'], ep=ep), idx))
                else:                                                   # a non-accepting call leaves ep alone
                    errs = merge(errs, errors(model, fix, dict(s=got['s'], ds=got['ds']), idx))
                    assert np.array_equal(ep, p)
    check(model, errs)


@pytest.mark.parametrize('t', ['P1', 'Q2'])
def test_nearly_hydrostatic_step_gives_the_elastic_stiffness(fep, t):
    """The footing's material (nu = 0.48) under a hydrostatic compressive initial strain and a displacement whose strains are
    1e-6 of it: every point is elastic with r / max|Et| below 1e-6, so K is the context's elastic stiffness and F the force of
    the elastic stress, at the bounds of K and F, per row as well.

    The stress of the initial strain is uniform, so its force vanishes at every interior node: what is left there is 1e-6 of
    the element contributions, and two float64 sums of them in different orders differ by 1e-16 of the contributions, 1e-10 and
    more of the node's force (the CPU restatement against the same elastic force: 1.1e-8 on the P1 mesh).  A node's error is
    therefore measured against the node's gross force, the sum of the absolute contributions, which is what its rounding
    scales with; the nodes whose force is no cancellation (a tenth of the gross force and more: the boundary) also keep the
    per-row bound against their own force."""
    rng = np.random.default_rng(48)
    elem, coord = rect(t, *MESHES[t])
    coord = jitter(elem, coord, 0.15, rng)
    shear, bulk = YOUNG / (2 * 1.48), YOUNG / (3 * 0.04)
    ref = MCRefContext(elem, coord, *fep.element_tables(fep.LagrangeElementType[t]))
    ref.set_materials(shear, bulk, SIN_PHI, COHESION)
    n = ref.n_int
    assert n > 256 and n % 256 != 0
    size = 2 * COHESION / (2 * shear)
    e0 = -size * np.array([1.0, 1.0, 0.0, 1.0]).reshape(4, 1)
    U = rng.normal(0, 1.0, size=(2, coord.shape[1]))
    U *= 1e-6 * size / np.abs(ref.orc.strain(ref.c['B'], U)).max()
    want = ref.step(U, None, e0=e0)
    print('r_rel', want['r_rel'].min(), want['r_rel'].max())
    assert not want['ind_p'].any() and want['r_rel'].max() <= 1e-6
    # the elastic answer, without the law: s = lam tr + 2G eps, K = K_elast
    E4 = np.concatenate([want['E'], np.zeros((1, n))]) + e0
    lam = bulk - 2 * shear / 3
    s_el = 2 * shear * E4 * np.array([1, 1, 0.5, 1]).reshape(4, 1) + lam * (E4[0] + E4[1] + E4[3]) * np.array([1, 1, 0, 1]).reshape(4, 1)
    K_el, F_el = ref.c['K_elast'].tocsr(), ref.orc.internal_force(ref.c['B'], ref.c['weight'], s_el)
    ctx = fep.MeshContext(elem, coord)
    ctx.set_model('mc')
    ctx.set_materials(shear, bulk, SIN_PHI, COHESION)
    try:
        got = ctx.step(U, None, e0=e0, want=('ds', 'ind_p', 'K', 'F'))
    finally:
        ctx.close()
    assert not got['ind_p'].any() and (got['n_smooth'], got['n_apex']) == (0, 0)
    K, F = got['K'], np.asarray(got['F']).reshape(-1, 2)
    F_el = F_el.reshape(-1, 2)
    gross = ref.orc.internal_force(abs(ref.c['B']), ref.c['weight'], np.abs(s_el)).reshape(-1, 2).max(axis=1)
    own = np.abs(F_el).max(axis=1)
    err = np.abs(F - F_el).max(axis=1)
    firm = own >= 0.1 * gross
    ek = abs(K - K_el).max() / abs(K_el).max()
    print('K', ek, relerr_rows(K, K_el), 'F', relerr(F, F_el), 'per node: over the gross force', (err / gross).max(),
          'over its own force where firm', (err / own)[firm].max(), int(firm.sum()), 'everywhere', relerr_rows(F, F_el))
    assert ek <= TOL_K and relerr_rows(K, K_el) <= TOL_K_ROW
    assert firm.sum() >= 8
    assert relerr(F, F_el) <= TOL_K and (err / gross).max() <= TOL_K_ROW and (err / own)[firm].max() <= TOL_K_ROW


# ---------------------------------------------------------------------------------------
# the sum of the per-workgroup counters at its loop edges
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_blocks', [1024, 8192])
@pytest.mark.parametrize('model', ['dp', 'vm', 'mc'])
def test_block_counters_are_summed_past_one_load_and_one_round(fep, model, n_blocks):
    """sum_block_counts: 1024 lanes, 8 loads per lane and round.  n = 1024 * 256 + 1 points are 1025 workgroups (lane 0 takes
    a second load), n = 8192 * 256 + 1 are 8193 (lane 0 enters a second round).  The points are the 1000 of the mesh-free
    tests, tiled: every output of point i is that of point i mod 1000 bit for bit, and the counters are the classes'."""
    import torch
    n = n_blocks * 256 + 1
    e1, p1, mats1, ref, cls1 = _thousand(model)
    assert (np.bincount(cls1, minlength=3)[:2 if model == 'vm' else 3] > 0).all()
    idx = np.arange(n) % 1000
    dev = torch.device('cuda', 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64)[..., idx])).to(dev)     # noqa: E731
    ed, pd = up(e1), up(p1)
    md = [up(m) for m in mats1]
    S = torch.zeros((4, n), dtype=torch.float64, device=dev)
    ind = torch.zeros(n, dtype=torch.uint8, device=dev)
    cnt = torch.full((2,), -1, dtype=torch.int64, device=dev)
    rc = getattr(fep.lib(), DEV_ENTRY[model])(0, torch.cuda.current_stream().cuda_stream, n, ed.data_ptr(), 1, n, None,
                                              pd.data_ptr(), *(m.data_ptr() for m in md), 0, S.data_ptr(), None,
                                              ind.data_ptr(), cnt.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    s, ind_p, counts = S.cpu().numpy(), ind.cpu().numpy().astype(bool), cnt.cpu().numpy()
    assert np.array_equal(pd.cpu().numpy(), p1[:, idx])                     # not accepting: ep untouched
    per_class = np.bincount(cls1[idx], minlength=3)
    print(model, n, counts, per_class)
    assert counts[0] + counts[1] == int(ind_p.sum())
    assert (counts[0], counts[1]) == (per_class[1], per_class[2])
    assert np.array_equal(s, s[:, :1000][:, idx]) and np.array_equal(ind_p, ind_p[:1000][idx])
    assert np.array_equal(ind_p[:1000], ref['ind_p'])
    assert relerr(s[:, :1000], ref['s']) <= 1e-13 and relerr_points(s[:, :1000], ref['s']) <= 1e-12

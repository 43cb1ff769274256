"""
Meshes with one node of high degree (tests/fan_mesh.py: a closed fan of k triangles around a centre node, with an outer
ring) against the oracle, on the route the product picks for them and on the COO form, with the gather plan replayed
against the symbolic phase (FEP_VALIDATE_PLAN) at every context creation.

  P1 k = 15          node route (the centre's diagonal block has 15 contributions: the packed descriptor's limit)
  P1 k = 16, 64, 255 the node route's descriptors do not pack: element route, patch form; k = 255 fills a whole
                     256-block tile of the COO route with one node row, its diagonal block has 255 contributions
  P2 k = 85          a centre row of exactly 256 blocks
  P4 k = 25          251 blocks, the largest P4 fan below the limit
  P1 k = 256, P2 k = 86, P4 k = 26: more than 256 blocks in one row, FEP_ERANGE

Tolerances are those of the oracle tests of the same element type (test_parity_gpu.py: P4's are a decade above P1 / P2's);
per point and per row of K one decade above the array-wide bound, as there.
"""
import numpy as np
import pytest

from conftest import dp_materials, relerr, relerr_points, relerr_rows
from fan_mesh import centre_of, fan_mesh, row_blocks
from footprint import scrub
from oracle import fep_oracle as orc
from routes import assert_route

pytestmark = pytest.mark.gpu

NQ = {'P1': 1, 'P2': 7, 'P4': 12}
# E, s / ds / accepted ep against the array maximum, s / ds per point, K / F against the array maximum, K per row
TOL = {'P1': (1e-13, 1e-13, 1e-12, 1e-12, 1e-11), 'P2': (1e-13, 1e-13, 1e-12, 1e-12, 1e-11),
       'P4': (1e-12, 1e-12, 1e-11, 1e-11, 1e-10)}
# (type, k, route the product picks)
FANS = [('P1', 15, 'node'), ('P1', 16, 'patch'), ('P1', 64, 'patch'), ('P1', 255, 'patch'), ('P2', 85, 'patch'),
        ('P4', 25, 'patch')]


def _state(coord, n, seed=0):
    """A displacement with isotropic expansion on the right (apex returns), shear on the upper left (smooth returns) and
    little else (elastic points), plus a small random previous plastic strain."""
    rng = np.random.default_rng(seed)
    x, y = coord
    th = np.arctan2(y, x)
    w_apex = np.clip(np.cos(th), 0, None) ** 2
    w_shear = np.clip(np.cos(th - 2.2), 0, None) ** 2
    U = 4e-5 * w_apex * np.array([x, y]) + 4e-4 * w_shear * np.array([y, x])
    U += rng.normal(0, 2e-6, size=U.shape)
    return U, rng.normal(0, 5e-6, size=(4, n))


@pytest.mark.parametrize('route', ['default', 'coo'])
@pytest.mark.parametrize('t,k,picked', FANS, ids=[f'{t}_k{k}' for t, k, _ in FANS])
def test_fan_mesh_vs_oracle(fep, monkeypatch, t, k, picked, route):
    if route == 'coo':
        monkeypatch.setenv('FEP_ROUTE', 'coo')
    else:
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    elem, coord = fan_mesh(k, t, shuffle=k % 2 == 1)
    assert row_blocks(elem, centre_of(elem)) == {'P1': k + 1, 'P2': 3 * k + 1, 'P4': 10 * k + 1}[t]
    n = elem.shape[1] * NQ[t]
    sh, bu, eta, c = dp_materials(n)
    U, Ep = _state(coord, n)
    ctx = fep.MeshContext(elem, coord)
    assert_route(ctx, picked if route == 'default' else 'coo')
    ctx.set_materials(sh, bu, eta, c)
    full = ctx.step(U, Ep.copy(), want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    scrub(ctx, U, Ep)                         # between the forms: none passes with what the one before left on the device
    kf = ctx.step(U, Ep.copy(), want=('K', 'F'))                         # the node route's one-kernel step
    ep = Ep.copy()
    scrub(ctx, U, Ep)
    acc = ctx.step(U, ep, apply_plastic_strain=True, want=('s', 'K', 'F'))
    scrub(ctx, U, Ep)
    K2, F2 = ctx.assemble(full['ds'], full['s'])
    ctx.close()
    for r in (kf, acc):
        assert np.array_equal(r['K'].data, full['K'].data) and np.array_equal(r['F'], full['F'])
    assert np.array_equal(K2.data, full['K'].data) and np.array_equal(F2, full['F'])
    assert np.array_equal(acc['s'], full['s'])

    d1, d2, wf = fep.element_tables(t)
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, sh, bu, d1, d2, wf)
    ops = dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=sh, bulk=bu, eta=eta, c=c)
    E, cp, K_t, F = orc.hot_path(U, Ep.copy(), ops)
    ep_o = Ep.copy()
    orc.hot_path(U, ep_o, ops, apply_plastic_strain=True)
    tol_e, tol_pt, tol_pt_each, tol_k, tol_k_rows = TOL[t]
    assert cp['n_smooth'] > 0 and cp['n_apex'] > 0 and cp['n_smooth'] + cp['n_apex'] < n      # every return-map branch
    assert (full['n_smooth'], full['n_apex']) == (cp['n_smooth'], cp['n_apex'])
    assert np.array_equal(full['ind_p'], cp['ind_p'])
    assert relerr(full['E'], E) <= tol_e
    assert relerr(full['s'], cp['s']) <= tol_pt and relerr(full['ds'], cp['ds']) <= tol_pt
    assert relerr_points(full['s'], cp['s']) <= tol_pt_each and relerr_points(full['ds'], cp['ds']) <= tol_pt_each
    assert relerr(ep, ep_o) <= tol_pt
    assert np.abs((full['K'] - K_t).data).max() <= tol_k * np.abs(K_t.data).max()
    assert relerr_rows(full['K'], K_t) <= tol_k_rows
    assert relerr(full['F'], F) <= tol_k


@pytest.mark.parametrize('t,k', [('P1', 256), ('P2', 86), ('P4', 26)])
def test_node_row_over_256_blocks_is_erange(fep, monkeypatch, t, k):
    """More than 256 blocks in one node row (more than 255 neighbours) fit no tile of the COO route's reduce kernel:
    fep_ctx_create returns FEP_ERANGE on every route (include/fep.h).  A valid context made right after, in the same
    process, works: the largest fan that fits, checked against the oracle."""
    monkeypatch.setenv('FEP_VALIDATE_PLAN', '1')
    elem, coord = fan_mesh(k, t, shuffle=True)
    assert row_blocks(elem, centre_of(elem)) > 256
    for route in ('default', 'coo', 'patch'):
        if route == 'default':
            monkeypatch.delenv('FEP_ROUTE', raising=False)
        else:
            monkeypatch.setenv('FEP_ROUTE', route)
        with pytest.raises(fep.FepError) as err:
            fep.MeshContext(elem, coord)
        assert err.value.code == -5
    monkeypatch.delenv('FEP_ROUTE', raising=False)
    elem, coord = fan_mesh(k - 1, t, shuffle=True)
    n = elem.shape[1] * NQ[t]
    sh, bu, eta, c = dp_materials(n)
    U, Ep = _state(coord, n)
    ctx = fep.MeshContext(elem, coord)
    assert_route(ctx, 'patch')
    ctx.set_materials(sh, bu, eta, c)
    r = ctx.step(U, Ep.copy(), want=('ind_p', 'K', 'F'))
    ctx.close()
    d1, d2, wf = fep.element_tables(t)
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, sh, bu, d1, d2, wf)
    E, cp, K_t, F = orc.hot_path(U, Ep.copy(), dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=sh, bulk=bu,
                                                    eta=eta, c=c))
    tol_k = TOL[t][3]
    assert np.array_equal(r['ind_p'], cp['ind_p'])
    assert np.abs((r['K'] - K_t).data).max() <= tol_k * np.abs(K_t.data).max() and relerr(r['F'], F) <= tol_k

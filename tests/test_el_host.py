"""
Host side of the Elasticity2D flavour (CPU only): surface tables and the cut-out mesh bit for bit against arrays recorded
from the reference (tests/golden/make_golden_el.py -> el_loads.npz), and tests/loads_ref.py, the float64 restatement of the
two load vectors the GPU tests lean on, against the reference's own vectors with the rounding bound of loads_ref.bound.
"""
import hashlib

import numpy as np
import pytest

import loads_ref
from conftest import load_golden

MESH_KEYS = ('coordinates', 'elements', 'surface', 'neumann_nodes', 'dirichlet_nodes', 'Q')


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize('t', ['P1', 'P2', 'Q1', 'Q2'])
def test_surface_tables_bit_exact(fep, t):
    g = load_golden('el_loads')
    xi_s, wf_s = fep.get_quadrature_surface(fep.LagrangeElementType[t])
    hatp_s, dhatp1_s = fep.get_local_basis_surface(t, xi_s)
    for name, got in (('xi_s', xi_s), ('wf_s', wf_s), ('hatp_s', hatp_s), ('dhatp1_s', dhatp1_s)):
        assert _same_bits(got, g[f'{t}_{name}']), name
    h, dh, wf = fep.surface_tables(t)
    assert h.shape == dh.shape == (hatp_s.shape[0], wf.size) and h.flags.c_contiguous and dh.flags.c_contiguous
    assert np.array_equal(h, hatp_s) and np.array_equal(dh, np.broadcast_to(dhatp1_s, dh.shape))
    assert abs(h.sum(axis=0) - 1).max() <= 4 * loads_ref.U and abs(dh.sum(axis=0)).max() <= 4 * loads_ref.U    # partition of unity


def test_surface_tables_same_names_in_the_flavour_namespace(fep):
    el = fep.elasticity2d
    for name in ('assemble_mesh', 'get_vector_volume', 'get_vector_traction', 'get_quadrature_surface',
                 'get_local_basis_surface', 'get_quadrature_volume', 'get_local_basis_volume',
                 'get_elastic_stiffness_matrix', 'elasticity_fem', 'LagrangeElementType'):
        assert hasattr(el, name), name
    assert el.assemble_mesh is fep.assemble_mesh_el and callable(fep.solve_elasticity2d)


@pytest.mark.parametrize('t', ['P1', 'Q1', 'Q2'])
def test_cutout_mesh_level1_bit_exact(fep, t):
    g = load_golden('el_loads')
    mesh = fep.elasticity2d.assemble_mesh(1, fep.LagrangeElementType[t], 10, 5)
    assert set(mesh) == set(MESH_KEYS)
    for k in MESH_KEYS:
        assert _same_bits(mesh[k], g[f'{t}_l1_{k}']), k
    assert mesh['elements'].min() == 1 and mesh['neumann_nodes'].min() >= 0          # 1-based / 0-based, as generated


def test_cutout_mesh_level3_sha256(fep):
    g = load_golden('el_loads')
    mesh = fep.assemble_mesh_el(3, 'P1', 10, 5)
    for k in MESH_KEYS:
        a = np.ascontiguousarray(mesh[k])
        assert a.shape == tuple(g[f'P1_l3_{k}_shape']), k
        assert np.array_equal(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8), g[f'P1_l3_{k}_sha']), k
    e = load_golden('el_p1')                                                       # the arrays themselves, recorded earlier
    assert np.array_equal(mesh['elements'], e['l3_elements_1based']) and np.array_equal(mesh['coordinates'], e['l3_coordinates'])


def test_cutout_mesh_p2_names_the_reference_failure(fep):
    with pytest.raises(ValueError, match='EL:698'):
        fep.assemble_mesh_el(1, 'P2', 10, 5)


def _check(got, sabs, m, ref, extra=2):
    ref = np.asarray(ref)
    lim = loads_ref.bound(m, sabs, extra)
    bad = np.abs(got - ref) > lim
    worst = float((np.abs(got - ref) / np.where(lim > 0, lim, 1.0)).max())
    print(f'worst |delta| / bound = {worst:.3f}')
    assert not bad.any(), (np.argwhere(bad)[:5], worst)
    assert np.all(got[:, m == 0] == 0) and np.all(ref[:, m == 0] == 0)


@pytest.mark.parametrize('t', ['P1', 'Q1', 'Q2'])
def test_loads_ref_volume_vs_reference_cutout(fep, t):
    g = load_golden('el_loads')
    tag = f'{t}_l1_'
    elem = g[tag + 'elements'] - 1
    n_n = g[tag + 'coordinates'].shape[1]
    hatp = fep.get_local_basis_volume(t, fep.get_quadrature_volume(t)[0])[0]
    n_int = g[tag + 'weight'].size
    f, sabs, m = loads_ref.volume(elem, n_n, np.array([[0.0], [-1.0]]) * np.ones((1, n_int)), hatp, g[tag + 'weight'])
    _check(f, sabs, m, g[tag + 'f_V'])
    f, sabs, m = loads_ref.volume(elem, n_n, g[tag + 'jig_f_V_int'], hatp, g[tag + 'jig_weight'])
    _check(f, sabs, m, g[tag + 'jig_f_V'])


def test_loads_ref_volume_vs_reference_p2_p4(fep):
    g, md, tx = load_golden('el_loads'), load_golden('mesh_dp'), load_golden('tsx')
    for t, tag, elem, n_n in (('P2', 'P2sq_', md['P2_n4_elements'], md['P2_n4_coordinates'].shape[1]),
                              ('P4', 'P4tx_', tx['p4_elem'], tx['p4_coord'].shape[1])):
        hatp = fep.get_local_basis_volume(t, fep.get_quadrature_volume(t)[0])[0]
        n_int = g[tag + 'weight'].size
        f, sabs, m = loads_ref.volume(elem, n_n, np.array([[0.0], [-1.0]]) * np.ones((1, n_int)), hatp, g[tag + 'weight'])
        _check(f, sabs, m, g[tag + 'f_V_const'])
        f, sabs, m = loads_ref.volume(elem, n_n, g[tag + 'f_V_int'], hatp, g[tag + 'weight'])
        _check(f, sabs, m, g[tag + 'f_V_rand'])


@pytest.mark.parametrize('t', ['P1', 'Q1', 'Q2', 'P2sq'])
def test_loads_ref_traction_vs_reference(fep, t):
    """The reference's edges are horizontal, where its |dx/dxi| is the arc length; its last-point quirk (EL:352-353) is
    restated by broadcasting, as the library's Python wrapper does.  Extra roundings of the arc length: see
    test_loads_gpu (m + 6)."""
    g = load_golden('el_loads')
    if t == 'P2sq':
        edges, coord = g['P2sq_edges'], load_golden('mesh_dp')['P2_n4_coordinates']
        cases = [(np.array([[0.0], [450.0]]) * np.ones((1, 8)), g['P2sq_f_t_const']), (g['P2sq_ft_int_var'], g['P2sq_f_t_var'])]
        tt = 'P2'
    else:
        edges, coord = g[f'{t}_l1_neumann_nodes'], g[f'{t}_l1_coordinates']
        n_pts = g[f'{t}_l1_ft_int_var'].shape[1]
        cases = [(np.array([[0.0], [450.0]]) * np.ones((1, n_pts)), g[f'{t}_l1_f_t']),
                 (g[f'{t}_l1_ft_int_var'], g[f'{t}_l1_f_t_var'])]
        tt = t
    h, dh, wf = fep.surface_tables(tt)
    for t_int, ref in cases:
        last = np.repeat(t_int[:, -1:], t_int.shape[1], axis=1)
        f, sabs, m = loads_ref.traction(edges, coord, last, h, dh, wf)
        _check(f, sabs, m, ref, extra=6)


def test_load_totals_of_the_reference_vectors():
    """sum f_V = force * area (75), sum f_t = traction * length (10): the demo's -75 and 4500."""
    g = load_golden('el_loads')
    for t in ('P1', 'Q1', 'Q2'):
        fV, fT = g[f'{t}_l1_f_V'], g[f'{t}_l1_f_t']
        n = fV.shape[1]
        assert abs(fV[1].sum() + 75) <= 2 * n * loads_ref.U * np.abs(fV[1]).sum() + 75 * 64 * loads_ref.U
        assert abs(fT[1].sum() - 4500) <= 2 * n * loads_ref.U * np.abs(fT[1]).sum() + 4500 * 64 * loads_ref.U
        assert np.all(fV[0] == 0) and np.all(fT[0] == 0)

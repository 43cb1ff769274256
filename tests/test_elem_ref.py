"""
tests/elem_ref.py, the element-by-element float64 reference of the element route, against the oracle (CPU only).

The oracle builds the global B (DP:549-570) and forms B^T D B with SciPy; the reference sums per element and point.  Both
are float64 sums of the same terms in different orders, so they must agree entry by entry within a small multiple of
u * S (elem_ref's error scales).  Measured worst |delta| / (u S) over the cases of
test_reference_matches_the_oracle_per_entry, P1 / P2 / Q1 / Q2 / P4: K 3.8 / 4.8 / 2.9 / 4.6 / 7.5, F 3.7 / 6.0 / 4.3 / 6.3 /
5.2, E 2.4 / 3.3 / 3.6 / 2.6 / 3.8.
"""
import zlib

import numpy as np
import pytest

import meshes
from conftest import dp_materials
from elem_ref import ElemRef, U_RND, on_pattern, ratio, reverse_elements
from meshes import fep
from oracle import fep_oracle as orc

TYPES = ('P1', 'P2', 'Q1', 'Q2', 'P4')
C_REF = 32                      # K, F and E against the oracle (measured <= 7.5, see above)


def _mesh(t, kind, rng):
    n = {'P1': 9, 'P2': 6, 'Q1': 9, 'Q2': 5, 'P4': 4}[t]
    if kind == 'delaunay':
        return meshes.delaunay(t, n, rng)
    elem, coord = meshes.square(t, n)
    if kind in ('jittered', 'renumbered'):
        coord = meshes.jitter(elem, coord, 0.15, rng)
    if kind == 'renumbered':
        elem, coord = meshes.renumber(elem, coord, rng)
    return elem, coord


def _random_state(n_int, n_n, rng):
    A = rng.normal(size=(3, 3, n_int))
    ds = (A + A.transpose(1, 0, 2)).reshape(9, n_int)                     # symmetric, like every tangent of the return map
    ds[:, rng.random(n_int) < 0.1] = 0.0                                   # apex points: zero tangent
    s = rng.normal(size=(4, n_int)) * 10.0 ** rng.uniform(-3, 3, n_int)
    U = rng.normal(size=(2, n_n))
    return ds, s, U


def _oracle(elem, coord, tb, ds, s, U):
    n_int = elem.shape[1] * tb[2].size
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, np.ones(n_int), np.ones(n_int), *tb)
    Kt = orc.tangent(0 * K, B, 0 * D, w, ds, iD, jD)                     # B^T (w ds) B alone
    return Kt, orc.internal_force(B, w, s), orc.strain(B, U)


@pytest.mark.parametrize('t,kind', [(t, k) for t in TYPES for k in ('square', 'jittered', 'delaunay', 'renumbered')
                                     if not (k == 'delaunay' and t in ('Q1', 'Q2'))])
def test_reference_matches_the_oracle_per_entry(t, kind):
    rng = np.random.default_rng(zlib.crc32(f'{t} {kind}'.encode()))
    elem, coord = _mesh(t, kind, rng)
    tb = fep.element_tables(t)
    ref = ElemRef(elem, coord, tb, chunk=7)
    ds, s, U = _random_state(ref.n_int, ref.n_n, rng)
    Kt, F, E = _oracle(elem, coord, tb, ds, s, U)
    K, S_K, Fr, S_F = ref.assemble(ds, s)
    Er, S_E = ref.strain(U)
    ip, ix = ref.pattern()
    assert ratio(K, on_pattern(Kt, ip, ix), S_K) <= C_REF
    assert ratio(Fr, F, S_F) <= C_REF
    assert ratio(Er, E, S_E) <= C_REF
    # the geometry is the oracle's bit for bit (the kernels' too: test_elastic_setup_vs_reference_golden)
    d1, d2, w, det = orc.geometry(elem, coord, *tb)
    g1, g2, gw, gdet = ref.geometry(0, ref.n_e)
    assert np.array_equal(gdet.ravel(), det) and np.array_equal(gw.ravel(), w.ravel())
    assert np.array_equal(g1.reshape(-1, ref.n_p).T, d1) and np.array_equal(g2.reshape(-1, ref.n_p).T, d2)
    # the bound has teeth: one entry off by 1e-9 of its own scale is caught
    i = int(np.argmax(S_K))
    K[i] += 1e-9 * S_K[i]
    assert ratio(K, on_pattern(Kt, ip, ix), S_K) > 1e6


@pytest.mark.parametrize('t', TYPES)
def test_results_do_not_depend_on_the_chunk_size(t):
    rng = np.random.default_rng(3)
    elem, coord = meshes.renumber(*_mesh(t, 'jittered', rng), rng)
    tb = fep.element_tables(t)
    outs = []
    for chunk in (1, 5, 64, 100000):
        ref = ElemRef(elem, coord, tb, chunk=chunk)
        if not outs:
            ds, s, U = _random_state(ref.n_int, ref.n_n, rng)
        outs.append((ref.strain(U), ref.assemble(ds, s)))
    (E0, SE0), (K0, SK0, F0, SF0) = outs[0]
    for (E, SE), (K, SK, F, SF) in outs[1:]:
        assert np.array_equal(E, E0) and np.array_equal(SE, SE0)
        assert ratio(K, K0, SK0) <= 4 and ratio(F, F0, SF0) <= 4
        assert np.allclose(SK, SK0, rtol=1e-13, atol=0) and np.allclose(SF, SF0, rtol=1e-13, atol=0)


@pytest.mark.parametrize('t', TYPES)
def test_orientation_reversing_permutations(t):
    """elem_ref.REVERSE turns every element over (det < 0 at every point) and leaves K, F the same operator: the reversed
    mesh against the oracle on that mesh per entry, and against the unreversed mesh's K to round-off of the geometry (the
    geometry itself is not the same bits on the two meshes: P4 differs by ~2.5e-12 of max |K|)."""
    rng = np.random.default_rng(11)
    elem, coord = _mesh(t, 'jittered', rng)
    tb = fep.element_tables(t)
    fwd = ElemRef(elem, coord, tb)
    assert (fwd.det() > 0).all()
    rev_elem = reverse_elements(elem, np.ones(elem.shape[1], dtype=bool))
    rev = ElemRef(rev_elem, coord, tb)
    assert (rev.det() < 0).all()
    # the quadrature points of a reversed element lie elsewhere in it: point data constant per element, an affine U
    ds, s, _ = _random_state(fwd.n_e, fwd.n_n, rng)
    ds, s = np.repeat(ds, fwd.n_q, axis=1), np.repeat(s, fwd.n_q, axis=1)
    U = np.array([[1e-3, -2e-3], [3e-3, 5e-4]]) @ coord + np.array([[0.1], [-0.2]])
    Kt, F, E = _oracle(rev_elem, coord, tb, ds, s, U)
    K, S_K, Fr, S_F = rev.assemble(ds, s)
    ip, ix = rev.pattern()
    assert ratio(K, on_pattern(Kt, ip, ix), S_K) <= C_REF and ratio(Fr, F, S_F) <= C_REF
    K0, _, F0, _ = fwd.assemble(ds, s)
    assert np.abs(K - K0).max() <= 1e-11 * np.abs(K0).max() and np.abs(Fr - F0).max() <= 1e-11 * np.abs(F0).max()
    E0, _ = fwd.strain(U)
    E1, _ = rev.strain(U)
    assert np.abs(E1 - E0).max() <= 1e-11 * np.abs(E0).max()


def test_reference_reads_every_entry_of_ds():
    """The reference takes ds as the full 3x3 (a non-symmetric ds gives the non-symmetric K); the library reads the upper
    triangle only (include/fep.h), which test_element_route_gpu.py's contract test pins."""
    rng = np.random.default_rng(5)
    elem, coord = meshes.square('Q1', 3)
    ref = ElemRef(elem, coord, fep.element_tables('Q1'))
    ds = rng.normal(size=(9, ref.n_int))
    K, _, _, _ = ref.assemble(ds)
    Kt, _, _ = _oracle(elem, coord, fep.element_tables('Q1'), ds, np.zeros((4, ref.n_int)), np.zeros((2, ref.n_n)))
    ip, ix = ref.pattern()
    import scipy.sparse as ssp
    Km = ssp.csr_matrix((K, ix, ip))
    assert np.abs((Km - Km.T).data).max() > 1e-3 * np.abs(K).max()
    # the oracle's (iD, jD) place ds[3 i + j] at (j, i) of D_p (DP:589-590): its K is this one transposed; the two
    # readings agree exactly where they matter, on a symmetric ds
    assert np.abs(K - on_pattern(Kt.T, ip, ix)).max() <= 64 * U_RND * np.abs(K).max()


def test_node_block_pattern_is_the_oracles_symbolic_pattern():
    elem, coord = meshes.square('P2', 4)
    ref = ElemRef(elem, coord, fep.element_tables('P2'))
    n_int = ref.n_int
    sh, bu, _, _ = dp_materials(n_int)
    K, *_ = orc.elastic_setup(elem, coord, sh, bu, *fep.element_tables('P2'))
    ip, ix = ref.pattern()
    v = on_pattern(K, ip, ix)                      # every stored entry of the oracle's K is in the pattern
    assert (v != 0).mean() > 0.9 and ip[-1] == ix.size

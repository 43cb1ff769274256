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


# ---------------------------------------------------------------------------------------------------------------------------
# The P1 node route's 48-byte record: d[2] = -(d[0] + d[1]) (elem_ref's module docstring).
#
# Record form against exact form, worst |delta| / (u S) over RECORD_MESHES with a random symmetric ds (measured, CPU):
#   widened scale   K 2.85   F 1.88      bound C_RECORD = 4      (with the return map's ds, s of the GPU cases: K 3.29, F 2.67)
#   plain scale     K 21.9   F 26.6      (near-right mesh; the others: K <= 8.7, F <= 12.4)
#   widened / plain scale, worst entry: K 23.9 / 26.9 / 31.8 / 86.7, F 36.2 / 25.0 / 16.0 / 89.4  (jittered / mixed / Delaunay / near-right)
# Why 4: a term B_a^T (w ds) B_b carries the third gradient in at most two factors; each differs from the table gradient
# by the one rounding of the sum, u (|d0| + |d1|) (widened: u * its own magnitude), and by the table gradient's own
# roundings (two products and a sum: <= ~1 u of |d0| + |d1| in practice); 2 factors x (1 + 1) = 4 u of the widened term.
# ---------------------------------------------------------------------------------------------------------------------------
C_RECORD = 4
RECORD_MESHES = ('jittered24', 'mixed24', 'delaunay24r', 'nearright24', 'aniso')
STRUCTURED = ('square24', 'aniso', 'rect54x10', 'strip301x1', 'square7')


def _p1_refs(name):
    import p1_node_cases as cases
    elem, coord, _ = cases.mesh(name)
    tb = fep.element_tables('P1')
    return ElemRef(elem, coord, tb), ElemRef(elem, coord, tb, record=True)


def _symmetric_state(n_int, rng, decades=3):
    A = rng.normal(size=(3, 3, n_int))
    return (A + A.transpose(1, 0, 2)).reshape(9, n_int), rng.normal(size=(4, n_int)) * 10.0 ** rng.uniform(-decades, decades, n_int)


@pytest.mark.parametrize('name', RECORD_MESHES)
def test_record_form_against_exact_form_on_the_widened_scale(name):
    exact, rec = _p1_refs(name)
    ds, s = _symmetric_state(exact.n_int, np.random.default_rng(zlib.crc32(name.encode())))
    K, S_K, F, S_F = exact.assemble(ds, s)
    _, W_K, _, W_F = exact.assemble(ds, s, widened=True)
    Kr, R_K, Fr, R_F = rec.assemble(ds, s)
    rk, rf = ratio(Kr, K, W_K), ratio(Fr, F, W_F)
    print(f'[record] {name}: widened K {rk:.2f} F {rf:.2f}; plain K {ratio(Kr, K, S_K):.2f} F {ratio(Fr, F, S_F):.2f}; '
          f'widened / plain scale <= K {(W_K / S_K).max():.1f} F {(W_F / S_F).max():.1f}')
    assert rk <= C_RECORD and rf <= C_RECORD, (rk, rf)
    assert (W_K >= S_K * (1 - 1e-14)).all() and (W_F >= S_F * (1 - 1e-14)).all()
    # the record's own plain scale lies within a rounding of the widened one from below (|d0 + d1| <= |d0| + |d1|)
    assert (R_K <= W_K * (1 + 1e-14)).all() and (R_F <= W_F * (1 + 1e-14)).all()
    # the strain keeps the table gradients (p1_point_kernel does)
    U = np.random.default_rng(1).normal(size=(2, exact.n_n))
    assert all(np.array_equal(a, b) for a, b in zip(exact.strain(U), rec.strain(U)))
    # the values do not depend on the scale asked for
    assert np.array_equal(rec.assemble(ds, s, widened=True)[0], Kr)


@pytest.mark.parametrize('name', STRUCTURED)
def test_record_form_is_bit_identical_on_structured_meshes(name):
    """Un-jittered right triangles: d[0] + d[1] is exact (one of the two terms is 0 or they are equal and opposite in
    each direction), so the record loses nothing, at 1 : 1000 cells either."""
    exact, rec = _p1_refs(name)
    ds, s = _symmetric_state(exact.n_int, np.random.default_rng(2))
    a, b = exact.assemble(ds, s), rec.assemble(ds, s)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_near_right_mesh_exceeds_the_plain_bound():
    """Why the widened scale exists: on right triangles moved by 1e-9 the third gradient has components of ~1e-9 of the
    others, and -(d[0] + d[1]) gives them with the absolute error of the large ones.  Against the exact form the record
    form then misses the element route's bound C_K['P1'] on the PLAIN scale (measured 21.9 against 10) while it is
    within C_RECORD on the widened one.  If this test fails, the record no longer behaves as the node-route test assumes."""
    from test_element_route_gpu import C_K
    exact, rec = _p1_refs('nearright24')
    ds, s = _symmetric_state(exact.n_int, np.random.default_rng(zlib.crc32(b'nearright24')))
    K, S_K, _, _ = exact.assemble(ds, s)
    W_K = exact.assemble(ds, s, widened=True)[1]
    Kr = rec.assemble(ds, s)[0]
    assert ratio(Kr, K, S_K) > C_K['P1']
    assert ratio(Kr, K, W_K) <= C_RECORD
    assert (W_K / S_K).max() > 20


@pytest.mark.parametrize('name', RECORD_MESHES)
def test_record_form_matches_the_oracle_on_the_widened_scale(name):
    exact, rec = _p1_refs(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    ds, s, U = _random_state(rec.n_int, rec.n_n, rng)
    Kt, F, _ = _oracle(rec.elem, rec.coord, fep.element_tables('P1'), ds, s, U)
    K, W_K, Fr, W_F = rec.assemble(ds, s, widened=True)
    ip, ix = rec.pattern()
    assert ratio(K, on_pattern(Kt, ip, ix), W_K) <= C_REF
    assert ratio(Fr, F, W_F) <= C_REF


def test_record_form_is_p1_only():
    elem, coord = meshes.square('P2', 3)
    with pytest.raises(ValueError):
        ElemRef(elem, coord, fep.element_tables('P2'), record=True)
    with pytest.raises(ValueError):
        ElemRef(elem, coord, fep.element_tables('P2')).assemble(np.zeros((9, elem.shape[1] * 7)), widened=True)


# ---------------------------------------------------------------------------------------------------------------------------
# Sensitivity of the node-route criterion (reference side only, NumPy arrays): the faults a wrong gather plan produces,
# one at a time, must each push |delta| / (u S) above the GPU test's bounds in at least one entry.
# ---------------------------------------------------------------------------------------------------------------------------
FAULTS = ('dropped', 'twice', 'wrong_node', 'neighbours_w', 'rows_swapped', 'off_by_1e-12')


def _element_terms(rec, e, ds, s):
    """K_e (6, 6), f_e (6,), w of element e in the record form."""
    d1, d2, w, _ = rec.geometry(e, e + 1)
    d1, d2, _, _ = rec.assembly_gradients(d1, d2)
    B = rec._B(d1, d2)[0, 0]                                                  # (3, 6)
    D = w[0, 0] * ds[:, e].reshape(3, 3)
    return B.T @ D @ B, B.T @ (w[0, 0] * s[0:3, e]), w[0, 0]


def _placements(rec):
    """{'diag' | 'edge' | 'boundary': (element e, local a, local b, another element e2 at the block)}: the diagonal block
    of an interior node, the block of an interior edge (two contributions) and the block of a boundary edge (one)."""
    elem = rec.elem
    x, y = rec.coord
    on_edge = (x == x.min()) | (x == x.max()) | (y == y.min()) | (y == y.max())
    out = {}
    for e in range(rec.n_e):
        for a in range(3):
            b = (a + 1) % 3
            n, m = elem[a, e], elem[b, e]
            shared = np.flatnonzero((elem == n).any(axis=0) & (elem == m).any(axis=0))
            other = [int(v) for v in shared if v != e]
            if 'boundary' not in out and on_edge[n] and on_edge[m] and not other:
                out['boundary'] = (e, a, b, int(np.flatnonzero((elem == n).any(axis=0) & (np.arange(rec.n_e) != e))[0]))
            if 'edge' not in out and not on_edge[n] and not on_edge[m] and len(other) == 1:
                out['edge'] = (e, a, b, other[0])
            if 'diag' not in out and not on_edge[n] and other:
                out['diag'] = (e, a, a, other[0])
        if len(out) == 3:
            break
    return out


@pytest.mark.parametrize('name', ['renumbered24', 'delaunay24r'])
def test_node_route_criterion_detects_every_gather_fault(name):
    from test_element_route_gpu import C_F, C_K
    exact, rec = _p1_refs(name)
    # point data of one magnitude: a contribution that is 1e-6 of its entry's scale can be off by 1e-12 of itself unseen by
    # any criterion of this kind (first tried with s over six decades: the 1e-12 fault in F reached 6.7 against 12)
    ds, s = _symmetric_state(rec.n_int, np.random.default_rng(zlib.crc32(name.encode()) + 2), decades=0)
    K, S_K, F, S_F = rec.assemble(ds, s)
    Kx, _, Fx, _ = exact.assemble(ds, s)
    _, W_K, _, W_F = exact.assemble(ds, s, widened=True)
    assert ratio(K, Kx, W_K) <= C_RECORD and ratio(F, Fx, W_F) <= C_RECORD
    places = _placements(rec)
    assert set(places) == {'diag', 'edge', 'boundary'}
    for place, (e, a, b, e2) in places.items():
        Ke, fe, w = _element_terms(rec, e, ds, s)
        _, _, w2 = _element_terms(rec, e2, ds, s)
        assert w2 != w
        pos = rec._positions(rec.elem[:, e:e + 1].T)[0][2 * a:2 * a + 2, 2 * b:2 * b + 2]      # the block's four CSR positions
        dof = 2 * rec.elem[a, e] + np.arange(2)
        blk, f = Ke[2 * a:2 * a + 2, 2 * b:2 * b + 2], fe[2 * a:2 * a + 2]
        c = (a + 1) % 3 if a == b else None                        # diagonal block: the second gradient of a wrong node
        wrong = Ke[2 * a:2 * a + 2, 2 * c:2 * c + 2] if a == b else Ke[2 * b:2 * b + 2, 2 * a:2 * a + 2]
        for fault in FAULTS:
            Kf, Ff = K.copy(), F.copy()
            if fault == 'dropped':
                Kf[pos] -= blk; Ff[dof] -= f
            elif fault == 'twice':
                Kf[pos] += blk; Ff[dof] += f
            elif fault == 'wrong_node':
                Kf[pos] += wrong - blk; Ff[dof] += fe[2 * ((a + 1) % 3):2 * ((a + 1) % 3) + 2] - f
            elif fault == 'neighbours_w':
                Kf[pos] += (w2 / w - 1) * blk; Ff[dof] += (w2 / w - 1) * f
            elif fault == 'rows_swapped':
                Kf[pos] = Kf[pos][::-1]; Ff[dof] = Ff[dof][::-1]
            else:
                Kf[pos] += 1e-12 * blk; Ff[dof] += 1e-12 * f
            rk, rkx = ratio(Kf, K, S_K), ratio(Kf, Kx, W_K)
            rf, rfx = ratio(Ff, F, S_F), ratio(Ff, Fx, W_F)
            print(f'[fault] {name} {place} {fault}: K {rk:.3g} (exact form, widened {rkx:.3g}) F {rf:.3g} ({rfx:.3g})')
            assert rk > C_K['P1'] and rkx > C_K['P1'] + 4, (place, fault, rk, rkx)
            assert rf > C_F['P1'] and rfx > C_F['P1'] + 4, (place, fault, rf, rfx)

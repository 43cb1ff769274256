"""
Element-by-element float64 restatement of the element route (strain, K_e = sum_q B^T (w ds) B, f_e = sum_q B^T (w s))
with a per-entry error scale beside every value, for the tests that compare the kernels entry by entry
(test_element_route_gpu.py) and for its own checks against the oracle (test_elem_ref.py).

Written from the formulas (DP:506-546, 585, 1043-1058), not from the oracle's global B: that matrix does not fit in memory
for Q2 / P4 at a quarter of a million elements, and the oracle's K_elast + B^T (D_p - D_elast) B cancels in rows whose
points are at the apex.  Elements are processed in chunks, straight into the CSR value array of the given pattern, so
that memory stays O(nnz + chunk).

Error scales (u = 2^-53 below is the unit round-off):
  S_E[i, k]  = sum_a |dphi| |u|                        the terms of the strain component i of point k
  S_K[p]     = sum_e sum_q (|B|^T |w ds| |B|)_ij        over every contribution to CSR entry p = (i, j)
  S_F[i]     = sum_e sum_q (|B|^T |w s|)_i
Any summation order of the same terms in float64 lands within (number of terms) * u * S of the exact sum, so a kernel and
this reference must agree to a small multiple of u * S entry by entry, however small the entry is against its row.

The geometry is computed with the operations, order and rounding of geometry_kernel / geometry_at_q (no fused
multiply-adds), so dphi and w are bit-identical to the kernels' and B carries no error of its own.

The P1 node route does not assemble from those three gradients.  Its kernels read a 48-byte record per element: the
gradients of local nodes 0 and 1 and the weight, and form  d[2] = -(d[0] + d[1])  (fep_kernels.hip.h: p1_node_kernel,
p1_node_lds_kernel, p1_fused_kernel).  That is one rounding of a sum whose terms may cancel, so a term with local node 2
is accurate to u (|d[0]| + |d[1]|), not to u |d[2]|.  Two things state this here, for P1 only:
  ElemRef(..., record=True)      the record form: assemble() takes d[2] = -(d[0] + d[1]), that operation in float64, and
                                 its scales are the plain ones of the record's own |B|; strain() keeps the table
                                 gradients, as p1_point_kernel does
  assemble(..., widened=True)    the widened scales: S_K, S_F with |d[2]| replaced by |d[0]| + |d[1]|, the terms the
                                 record form really sums — the scale on which the record form and the exact form agree
"""
import numpy as np

U_RND = 2.0 ** -53

# local renumbering that reverses an element's orientation (det < 0) and keeps its shape: the vertices 1 and 2 (Q1: 1 and 3)
# swap, and every edge / interior node follows its edge or position
REVERSE = {'P1': [0, 2, 1], 'P2': [0, 2, 1, 3, 5, 4], 'Q1': [0, 3, 2, 1], 'Q2': [0, 3, 2, 1, 7, 6, 5, 4],
           'P4': [0, 2, 1, 5, 4, 3, 11, 10, 9, 8, 7, 6, 12, 14, 13]}
TYPE_OF_NP = {3: 'P1', 6: 'P2', 4: 'Q1', 8: 'Q2', 15: 'P4'}


def node_block_pattern(elem, n_n):
    """(indptr, indices) int64 of the DOF-level CSR pattern of K: every pair of nodes sharing an element, as 2x2 blocks
    with sorted columns — the symbolic pattern the library builds (MeshContext.pattern)."""
    elem = np.asarray(elem, dtype=np.int64)
    keys = np.unique((elem[:, None, :] * n_n + elem[None, :, :]).ravel())
    rows, cols = keys // n_n, keys % n_n
    deg = np.bincount(rows, minlength=n_n)
    # row 2n: the columns 2m, 2m+1 of every block (n, m); row 2n+1 the same
    start = np.concatenate([[0], np.cumsum(deg)])
    rowlen = np.repeat(2 * deg, 2)
    indptr = np.concatenate([[0], np.cumsum(rowlen)]).astype(np.int64)
    indices = np.empty(indptr[-1], dtype=np.int64)
    off = np.arange(keys.size) - start[rows]                                # block's place in its node row
    for i in range(2):
        base = indptr[2 * rows + i] + 2 * off
        indices[base] = 2 * cols
        indices[base + 1] = 2 * cols + 1
    return indptr, indices


class ElemRef:
    """The element route of one mesh in float64.  `elem` (n_p, n_e) 0-based, `coord` (2, n_n); `tables` = (dhatp1,
    dhatp2, wf) as element_tables(t) returns them; `pattern` = (indptr, indices) of the CSR values K is accumulated into
    (MeshContext.pattern(); default: node_block_pattern)."""

    def __init__(self, elem, coord, tables, pattern=None, chunk=4096, record=False):
        self.elem = np.ascontiguousarray(elem, dtype=np.int64)
        self.coord = np.ascontiguousarray(coord, dtype=np.float64)
        self.n_p, self.n_e = self.elem.shape
        self.n_n = self.coord.shape[1]
        self.t = TYPE_OF_NP[self.n_p]
        if record and self.t != 'P1':
            raise ValueError('the record form is the P1 node route\'s: no other element type has it')
        self.record = bool(record)
        d1, d2, wf = tables
        self.wf = np.asarray(wf, dtype=np.float64).ravel()
        self.n_q = self.wf.size
        self.h1 = np.broadcast_to(np.asarray(d1, dtype=np.float64), (self.n_p, self.n_q))
        self.h2 = np.broadcast_to(np.asarray(d2, dtype=np.float64), (self.n_p, self.n_q))
        self.n_int = self.n_e * self.n_q
        self.n_dof = 2 * self.n_n
        self.chunk = int(chunk)
        self._pattern = pattern
        self._blocks = None

    # -- geometry (DP:530-546, 585), chunk of elements e0 .. e1-1 -> dphi1, dphi2 (m, n_q, n_p), w (m, n_q), det (m, n_q)
    def geometry(self, e0, e1):
        el = self.elem[:, e0:e1]
        x, y = self.coord[0][el], self.coord[1][el]                          # (n_p, m)
        j11 = j12 = j21 = j22 = 0.0
        for a in range(self.n_p):                                            # same order as the kernels, no FMA
            h1, h2 = self.h1[a][None, :], self.h2[a][None, :]
            xa, ya = x[a][:, None], y[a][:, None]
            j11 = j11 + xa * h1
            j12 = j12 + ya * h1
            j21 = j21 + xa * h2
            j22 = j22 + ya * h2
        det = j11 * j22 - j12 * j21
        i11, i12, i21, i22 = j22 / det, -j12 / det, -j21 / det, j11 / det
        h1, h2 = self.h1.T[None], self.h2.T[None]                           # (1, n_q, n_p)
        d1 = i11[..., None] * h1 + i12[..., None] * h2
        d2 = i21[..., None] * h1 + i22[..., None] * h2
        w = np.abs(det) * self.wf[None, :]
        return d1, d2, w, det

    def det(self):
        """det of every point, (n_int,) in point order (k = e * n_q + q)."""
        return np.concatenate([self.geometry(e0, min(e0 + self.chunk, self.n_e))[3].ravel()
                               for e0 in range(0, self.n_e, self.chunk)]) if self.n_e else np.zeros(0)

    def assembly_gradients(self, d1, d2, widened=False):
        """(d1, d2, |d1|, |d2|) as assemble() uses them: the table gradients or, in the record form, d[2] = -(d[0] + d[1]);
        the magnitudes are those of the gradients used or, widened, |d[2]| replaced by |d[0]| + |d[1]|."""
        if self.record:
            d1 = np.concatenate([d1[..., :2], -(d1[..., 0:1] + d1[..., 1:2])], axis=-1)
            d2 = np.concatenate([d2[..., :2], -(d2[..., 0:1] + d2[..., 1:2])], axis=-1)
        a1, a2 = np.abs(d1), np.abs(d2)
        if widened:
            if self.t != 'P1':
                raise ValueError('the widened scale is the P1 node route\'s: no other element type has it')
            a1 = np.concatenate([a1[..., :2], a1[..., 0:1] + a1[..., 1:2]], axis=-1)
            a2 = np.concatenate([a2[..., :2], a2[..., 0:1] + a2[..., 1:2]], axis=-1)
        return d1, d2, a1, a2

    def _B(self, d1, d2):
        """B per point, (m, n_q, 3, 2 n_p): rows [11, 22, 12 (engineering)], columns 2a + [x, y]."""
        m = d1.shape[0]
        B = np.zeros((m, self.n_q, 3, 2 * self.n_p))
        B[:, :, 0, 0::2] = d1
        B[:, :, 1, 1::2] = d2
        B[:, :, 2, 0::2] = d2
        B[:, :, 2, 1::2] = d1
        return B

    # -- a1: strain, E = B u per point
    def strain(self, U):
        """(E, S_E), both (3, n_int).  `U` (2, n_n) or flat DOF order."""
        U = np.asarray(U, dtype=np.float64)
        ux, uy = (U[0], U[1]) if U.ndim == 2 else (U[0::2], U[1::2])
        E = np.empty((3, self.n_int))
        S = np.empty((3, self.n_int))
        for e0 in range(0, self.n_e, self.chunk):
            e1 = min(e0 + self.chunk, self.n_e)
            d1, d2, _, _ = self.geometry(e0, e1)
            el = self.elem[:, e0:e1].T[:, None, :]                           # (m, 1, n_p)
            x, y = ux[el], uy[el]
            sl = slice(e0 * self.n_q, e1 * self.n_q)
            E[0, sl] = (d1 * x).sum(-1).ravel()
            E[1, sl] = (d2 * y).sum(-1).ravel()
            E[2, sl] = (d1 * y + d2 * x).sum(-1).ravel()
            S[0, sl] = np.abs(d1 * x).sum(-1).ravel()
            S[1, sl] = np.abs(d2 * y).sum(-1).ravel()
            S[2, sl] = (np.abs(d1 * y) + np.abs(d2 * x)).sum(-1).ravel()
        return E, S

    # -- CSR positions of the node-pair blocks
    def pattern(self):
        if self._pattern is None:
            self._pattern = node_block_pattern(self.elem, self.n_n)
        return self._pattern

    def _block_table(self):
        """Sorted node-block keys n*n_n + m and, per key, the CSR position of its entry (2n, 2m) and the length of row 2n."""
        if self._blocks is None:
            ip, ix = self.pattern()
            ip = np.asarray(ip, dtype=np.int64)
            ix = np.asarray(ix, dtype=np.int64)
            rowlen = np.diff(ip)
            assert (rowlen[0::2] == rowlen[1::2]).all(), 'not a node-block pattern'
            row = np.repeat(np.arange(self.n_dof, dtype=np.int64), rowlen)
            pos = np.flatnonzero((row % 2 == 0) & (ix % 2 == 0))
            assert (ix[pos + 1] == ix[pos] + 1).all(), 'not a node-block pattern'
            keys = (row[pos] // 2) * self.n_n + ix[pos] // 2
            assert (np.diff(keys) > 0).all()
            self._blocks = (keys, pos, rowlen[row[pos]])
            self.nnz = ix.size
        return self._blocks

    def _positions(self, el):
        """CSR positions (m, 2 n_p, 2 n_p) of the element's DOF pairs (2a + i, 2b + j)."""
        keys, pos, rl = self._block_table()
        k = (el[:, :, None] * self.n_n + el[:, None, :])                     # (m, n_p, n_p)
        idx = np.searchsorted(keys, k)
        assert (idx < keys.size).all() and (keys[np.minimum(idx, keys.size - 1)] == k).all(), 'pair missing from the pattern'
        p0, r = pos[idx], rl[idx]
        out = np.empty(el.shape[:1] + (self.n_p, 2, self.n_p, 2), dtype=np.int64)
        for i in range(2):
            for j in range(2):
                out[:, :, i, :, j] = p0 + i * r + j
        return out.reshape(el.shape[0], 2 * self.n_p, 2 * self.n_p)

    @staticmethod
    def _scatter(dst, idx, val):
        """dst[idx] += val over duplicate indices, through a bincount over the chunk's index range only."""
        lo, hi = int(idx.min()), int(idx.max()) + 1
        dst[lo:hi] += np.bincount(idx.ravel() - lo, weights=val.ravel(), minlength=hi - lo)

    # -- a3 + a4, a5: assembly from given point data
    def assemble(self, ds=None, s=None, widened=False):
        """(K, S_K, F, S_F): K, S_K the CSR values (nnz,) of sum_e sum_q B^T (w ds) B and of its scale, F, S_F (n_dof,)
        of sum_e sum_q B^T (w s[0:3]); the pairs of an absent input are None.  `ds` (9, n_int) row-major 3x3 (all nine
        entries are used: a non-symmetric ds gives the non-symmetric K), `s` (>= 3, n_int).  `widened` (P1): the scales with
        |d[2]| replaced by |d[0]| + |d[1]| (module docstring); the values do not depend on it."""
        nq, npp = self.n_q, self.n_p
        K = S_K = F = S_F = None
        if ds is not None:
            self._block_table()
            K, S_K = np.zeros(self.nnz), np.zeros(self.nnz)
        if s is not None:
            F, S_F = np.zeros(self.n_dof), np.zeros(self.n_dof)
        for e0 in range(0, self.n_e, self.chunk):
            e1 = min(e0 + self.chunk, self.n_e)
            m = e1 - e0
            d1, d2, w, _ = self.geometry(e0, e1)
            d1, d2, a1, a2 = self.assembly_gradients(d1, d2, widened)
            B = self._B(d1, d2)                                              # (m, nq, 3, 2np)
            Bf = B.reshape(m, nq * 3, 2 * npp)
            absB = self._B(a1, a2)                                           # |B|, or its widened form
            aB = absB.reshape(m, nq * 3, 2 * npp)
            el = self.elem[:, e0:e1].T
            sl = slice(e0 * nq, e1 * nq)
            if ds is not None:
                D = (w[..., None, None] * np.asarray(ds)[:, sl].T.reshape(m, nq, 3, 3))
                DB = np.matmul(D, B).reshape(m, nq * 3, 2 * npp)             # (w ds) B per point
                aDB = np.matmul(np.abs(D), absB).reshape(m, nq * 3, 2 * npp)
                Ke = np.matmul(Bf.transpose(0, 2, 1), DB)                    # (m, 2np, 2np)
                Se = np.matmul(aB.transpose(0, 2, 1), aDB)
                p = self._positions(el)
                self._scatter(K, p, Ke)
                self._scatter(S_K, p, Se)
            if s is not None:
                ws = (w[..., None] * np.asarray(s)[0:3, sl].T.reshape(m, nq, 3)).reshape(m, nq * 3)
                fe = np.einsum('mka,mk->ma', Bf, ws)
                sf = np.einsum('mka,mk->ma', aB, np.abs(ws))
                dof = (2 * el[:, :, None] + np.arange(2)[None, None, :]).reshape(m, 2 * npp)
                self._scatter(F, dof, fe)
                self._scatter(S_F, dof, sf)
        return K, S_K, F, S_F


def ratio(got, ref, scale):
    """max |got - ref| / (u * scale) entry by entry; an entry of zero scale must agree exactly (its ratio is then 0 or inf)."""
    d = np.abs(np.asarray(got, dtype=float) - np.asarray(ref, dtype=float))
    sc = U_RND * np.asarray(scale, dtype=float)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(sc > 0, d / np.where(sc > 0, sc, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def on_pattern(A, indptr, indices):
    """The values of the SciPy matrix A at the positions of the CSR pattern (indptr, indices); every stored entry of A must
    lie in the pattern (explicit zeros may lie anywhere)."""
    import scipy.sparse as ssp
    A = ssp.coo_matrix(A)
    n = A.shape[1]
    ip = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(ip.size - 1, dtype=np.int64), np.diff(ip))
    keys = rows * n + np.asarray(indices, dtype=np.int64)
    ka = A.row.astype(np.int64) * n + A.col
    idx = np.searchsorted(keys, ka)
    hit = (idx < keys.size) & (keys[np.minimum(idx, keys.size - 1)] == ka)
    assert (hit | (A.data == 0)).all(), 'an entry of A is outside the pattern'
    out = np.zeros(keys.size)
    np.add.at(out, idx[hit], A.data[hit])
    return out


def reverse_elements(elem, which):
    """`elem` with the elements where `which` is true renumbered locally so that their orientation flips (REVERSE)."""
    elem = np.array(elem, copy=True)
    perm = REVERSE[TYPE_OF_NP[elem.shape[0]]]
    elem[:, which] = elem[perm][:, which]
    return elem

"""
High-precision reference of the external-load vectors (include/fep.h, fep_load_traction_* / fep_load_volume_*) in plain
Python `decimal` at 60 digits, and the rounding bounds of the two kernels against it.  No GPU, no library call (the pattern
of loads_ref.py, elem_ref.py, amg_ref.py).  Used by tests/test_loads_exact_host.py and tests/test_loads_shapes_gpu.py.

Why: loads_ref.traction is itself float64, and its j_c = sum_a x_a dhat_a cancels coordinates of the size of the mesh down
to half an edge length; on curved, high-order edges away from the origin that error is larger than the whole bound
2 (m + 6) u sum |terms| of tests/test_loads_gpu.py, so a float64 restatement cannot referee the kernel there.

The float64 inputs are taken as exact numbers (Decimal(float) is exact); every intermediate result is rounded to 60
significant digits, a relative 10^-60 against u = 2^-53 ~ 1.1e-16, also where j_c cancels (10^-60 of sum_a |x_a dhat_a|);
the result is rounded to float64 once at the end.

traction_bound -- derivation
----------------------------
load_traction_kernel works under `#pragma clang fp contract(off)`: every * and + is one IEEE rounding (relative error at
most u), sqrt is correctly rounded, every sum starts at 0.0 and adds in turn (the first addition, to 0.0, is exact).
One term of node n is  T = h * (w * t),  w = sqrt(j1 j1 + j2 j2) * wf,  j_c = sum_a x_{c,a} * dhat_a  (h = hatp_s[a, q],
x_{c,a} = coord[c, edges[a, e]], dhat_a = dhatp1_s[a, q], t = t_int[c', e n_q_s + q]).

 (a) j_c: n_p_s products and n_p_s - 1 additions, so each product passes through at most n_p_s roundings:
         |j_c^ - j_c| <= n_p_s u A_c (1 + O(u)),      A_c = sum_a |x_{c,a} dhat_a|.
     This is the cancellation term: A_c is of the size of |x| |dhat| while j_c is half an edge length.
 (b) with J(j) = sqrt(j1^2 + j2^2), the Euclidean norm:  |J(j^) - J(j)| <= |j^ - j|_2 <= |j1^ - j1| + |j2^ - j2|
     (triangle inequality, |dJ/dj_c| <= 1; no first-order approximation here), so
         |J(j^) - J(j)| <= n_p_s u (A_1 + A_2) (1 + O(u)).
 (c) the computed root of the computed j^: the two squares carry one rounding each, on two non-negative summands (together
     a relative u of their sum), the sum a second one, hence 2 u under the root = 1 u outside it; the root's own rounding
     1 u:  J^ = J(j^) (1 + 2 u).  Then * wf, w * t and h * (...) are three more:  T^ = h wf t J(j^) (1 + 5 u) to first order.
 (d) so  |T^ - T| <= |h wf t| [ 5 u J + n_p_s u (A_1 + A_2) ]  to first order.
 (e) the sum of the m terms of a node (m = incidences * n_q_s) in the kernel's fixed order: at most (m - 1) u sum |T^|.
 (f) the reference's single rounding to float64: u |f| <= u sum |T|.
 Together, to first order,
         |got - exact| <= u [ (m + 5) S_J + n_p_s S_A ],
         S_J = sum |h wf t| J,     S_A = sum |h wf t| (A_1 + A_2)          (sums over the terms of the node).
 The neglected products of two errors are at most (m + 4) u times the first-order part (d) plus O(u) times (a): one more u
 on each constant covers them for every m < 2^40.  Hence

         lim = u [ (m + 6) S_J + (n_p_s + 1) S_A ].

 The kernel must meet it whatever the edge order, duplicates included (every listed edge is a term).  A node on no edge has
 m = 0, lim = 0 and must hold exactly 0.  (No input of the tests is near the subnormal range.)

 lim itself is evaluated in float64 from float64 J and A_c: its own relative error, about (n_p_s + m) u, is far inside the
 extra u on each constant.  J and A_c in it are taken from the exact j_c rounded once, so the bound does not inherit the
 cancellation it accounts for.

volume_bound
------------
load_volume_kernel: T = h * (w * f), two roundings, then the sequential sum of the node's m = incidences * n_q terms, and
the reference's one rounding:  |got - exact| <= (m - 1 + 2 + 1) u sum |T| = (m + 2) u sum |T| to first order, which is
loads_ref.bound(m, sabs, 2) halved (that bound is for two rounded evaluations, here only one side is rounded).  `weight` is
an input, so there is no cancellation term.  The neglected second-order part is below 2 m u of the bound (2^-44 of it at the
fan's hub, m = 255).
"""
import decimal
from fractions import Fraction

import numpy as np

import loads_ref

U = loads_ref.U
PREC = 60
D = decimal.Decimal


def _dec(a):
    """Nested lists of exact Decimals from a float array."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return [D(float(v)) for v in a]
    return [_dec(r) for r in a]


def _tables(n_p_s, hatp_s, dhatp1_s, wf_s):
    wf = np.ascontiguousarray(np.asarray(wf_s, dtype=np.float64).ravel())
    n_q_s = wf.size
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(hatp_s, dtype=np.float64), (n_p_s, n_q_s)))
    dh = np.ascontiguousarray(np.broadcast_to(np.asarray(dhatp1_s, dtype=np.float64), (n_p_s, n_q_s)))
    return h, dh, wf, n_q_s


def _jacobians(edges, coord, dh, n_q_s):
    """Exact j_c(e, q) as Decimals [c][e][q], inside a decimal context of PREC digits."""
    n_p_s, n_e_s = edges.shape
    dd = _dec(dh)
    out = []
    for c in range(2):
        xc = coord[c]
        rows = []
        for e in range(n_e_s):
            xa = [D(float(xc[edges[a, e]])) for a in range(n_p_s)]
            rows.append([sum((xa[a] * dd[a][q] for a in range(n_p_s)), D(0)) for q in range(n_q_s)])
        out.append(rows)
    return out


def traction_exact(edges, coord, t_int, hatp_s, dhatp1_s, wf_s):
    """f[c, n] = sum over the (e, a) with edges[a, e] == n, over q, of hatp_s[a, q] sqrt(j1^2 + j2^2) wf_s[q] t[c, e n_q_s + q],
    j_c = sum_a coord[c, edges[a, e]] dhatp1_s[a, q]: the formula of include/fep.h at PREC digits, rounded to float64 once.
    -> (2, n_n) float64.  Only the loaded nodes are visited, so n_n may be large."""
    edges = np.asarray(edges).astype(np.int64)
    coord = np.asarray(coord, dtype=np.float64)
    n_p_s, n_e_s = edges.shape
    h, dh, wf, n_q_s = _tables(n_p_s, hatp_s, dhatp1_s, wf_s)
    t = np.asarray(t_int, dtype=np.float64).reshape(2, n_e_s, n_q_s)
    out = np.zeros((2, coord.shape[1]))
    acc = {}
    with decimal.localcontext() as ctx:
        ctx.prec = PREC
        hd, wd = _dec(h), _dec(wf)
        j = _jacobians(edges, coord, dh, n_q_s)
        for e in range(n_e_s):
            for q in range(n_q_s):
                w = (j[0][e][q] * j[0][e][q] + j[1][e][q] * j[1][e][q]).sqrt() * wd[q]
                wt = (w * D(float(t[0, e, q])), w * D(float(t[1, e, q])))
                for a in range(n_p_s):
                    s = acc.setdefault(int(edges[a, e]), [D(0), D(0)])
                    s[0] += hd[a][q] * wt[0]
                    s[1] += hd[a][q] * wt[1]
        for n, s in acc.items():
            out[0, n], out[1, n] = float(s[0]), float(s[1])                  # float(Decimal) rounds correctly
    return out


def traction_bound(edges, coord, t_int, hatp_s, dhatp1_s, wf_s):
    """-> (lim (2, n_n), m (n_n,)): lim = u [(m + 6) S_J + (n_p_s + 1) S_A] of the module docstring, m the number of
    (e, a, q) terms of each node."""
    edges = np.asarray(edges).astype(np.int64)
    coord = np.asarray(coord, dtype=np.float64)
    n_n = coord.shape[1]
    n_p_s, n_e_s = edges.shape
    h, dh, wf, n_q_s = _tables(n_p_s, hatp_s, dhatp1_s, wf_s)
    t = np.asarray(t_int, dtype=np.float64).reshape(2, n_e_s, n_q_s)
    J, A = jacobian_sizes(edges, coord, dhatp1_s, wf_s)
    nodes = np.repeat(edges[:, :, None], n_q_s, axis=2).ravel()
    m = np.bincount(nodes, minlength=n_n)
    lim = np.zeros((2, n_n))
    for c in range(2):
        hwt = np.abs(h[:, None, :] * (wf[None, :] * t[c])[None, :, :])      # (n_p_s, n_e_s, n_q_s)
        s_j = np.bincount(nodes, weights=(hwt * J[None]).ravel(), minlength=n_n)
        s_a = np.bincount(nodes, weights=(hwt * A[None]).ravel(), minlength=n_n)
        lim[c] = U * ((m + 6) * s_j + (n_p_s + 1) * s_a)
    return lim, m


def jacobian_sizes(edges, coord, dhatp1_s, wf_s):
    """(J (n_e_s, n_q_s), A_1 + A_2 (n_e_s, n_q_s)) in float64: J from the exact j_c rounded once, A_c = sum_a |x_{c,a} dhat_a|."""
    edges = np.asarray(edges).astype(np.int64)
    coord = np.asarray(coord, dtype=np.float64)
    n_p_s, n_e_s = edges.shape
    _, dh, _, n_q_s = _tables(n_p_s, dhatp1_s, dhatp1_s, wf_s)          # only the derivative table is needed here
    J = np.zeros((n_e_s, n_q_s))
    with decimal.localcontext() as ctx:
        ctx.prec = PREC
        j = _jacobians(edges, coord, dh, n_q_s)
        for e in range(n_e_s):
            for q in range(n_q_s):
                J[e, q] = float((j[0][e][q] * j[0][e][q] + j[1][e][q] * j[1][e][q]).sqrt())
    A = np.zeros((n_e_s, n_q_s))
    for c in range(2):
        A += np.abs(coord[c][edges][:, :, None] * dh[:, None, :]).sum(axis=0)
    return J, A


def volume_exact(elements, n_n, f_v_int, hatp, weight):
    """f[c, n] = sum over the (e, a) with elements[a, e] == n, over q, of hatp[a, q] weight[e n_q + q] f[c, e n_q + q] at PREC
    digits, rounded to float64 once.  -> (2, n_n) float64."""
    elements = np.asarray(elements).astype(np.int64)
    n_p, n_e = elements.shape
    hatp = np.asarray(hatp, dtype=np.float64)
    hatp = np.broadcast_to(hatp, (n_p, hatp.shape[1]))
    n_q = hatp.shape[1]
    w = np.asarray(weight, dtype=np.float64).reshape(n_e, n_q)
    f = np.asarray(f_v_int, dtype=np.float64).reshape(2, n_e, n_q)
    acc = [[D(0), D(0)] for _ in range(n_n)]
    out = np.zeros((2, n_n))
    with decimal.localcontext() as ctx:
        ctx.prec = PREC
        hd = _dec(hatp)
        for e in range(n_e):
            wf = [(D(float(w[e, q])) * D(float(f[0, e, q])), D(float(w[e, q])) * D(float(f[1, e, q]))) for q in range(n_q)]
            for a in range(n_p):
                s = acc[elements[a, e]]
                ha = hd[a]
                for q in range(n_q):
                    s[0] += ha[q] * wf[q][0]
                    s[1] += ha[q] * wf[q][1]
        for n in range(n_n):
            out[0, n], out[1, n] = float(acc[n][0]), float(acc[n][1])
    return out


def volume_bound(elements, n_n, f_v_int, hatp, weight):
    """-> (lim (2, n_n), m (n_n,)): (m + 2) u sum |terms| = loads_ref.bound(m, sabs, 2) / 2."""
    _, sabs, m = loads_ref.volume(elements, n_n, f_v_int, hatp, weight)
    return 0.5 * loads_ref.bound(m, sabs, 2), m


# ---- edge tables -----------------------------------------------------------------------------------------------------------
P2_NODES = (-1, 1, 0)                                                       # surf's (B, A, mid)
P3_NODES = (-1, 1, Fraction(-1, 3), Fraction(1, 3))
P4_NODES = (-1, 1, 0, Fraction(1, 2), Fraction(-1, 2))                      # surf's (B, A, mid, quarter nearer A, quarter nearer B)


def _lagrange(nodes, x):
    """(values, derivatives) of the Lagrange basis on `nodes` at x, all Fractions."""
    k = len(nodes)
    val, der = [], []
    for i in range(k):
        v = Fraction(1)
        for j in range(k):
            if j != i:
                v *= (x - nodes[j]) / (nodes[i] - nodes[j])
        d = Fraction(0)
        for j in range(k):
            if j != i:
                p = Fraction(1) / (nodes[i] - nodes[j])
                for l in range(k):
                    if l != i and l != j:
                        p *= (x - nodes[l]) / (nodes[i] - nodes[l])
                d += p
        val.append(v)
        der.append(d)
    return val, der


def edge_tables(nodes_xi, n_q):
    """(hatp_s (n_p_s, n_q), dhatp1_s (n_p_s, n_q), wf_s (n_q,)) of the Lagrange basis on the nodes `nodes_xi` of the
    reference edge [-1, 1] at the n_q Gauss-Legendre points of numpy.polynomial.legendre.leggauss.  The basis is evaluated
    in rational arithmetic AT the float points and rounded once per entry, so the tables are exact inputs up to u each."""
    nodes = [Fraction(v) for v in nodes_xi]
    xi, wf = np.polynomial.legendre.leggauss(n_q)
    h = np.zeros((len(nodes), n_q))
    dh = np.zeros((len(nodes), n_q))
    for q in range(n_q):
        v, d = _lagrange(nodes, Fraction(float(xi[q])))
        for a in range(len(nodes)):
            h[a, q], dh[a, q] = float(v[a]), float(d[a])                   # float(Fraction) rounds correctly
    return h, dh, np.ascontiguousarray(wf, dtype=np.float64)


def gauss_defect(nodes_xi, dhatp1_s, wf_s):
    """|E_a|, E_a = sum_q wf_s[q] dhatp1_s[a, q] - (L_a(1) - L_a(-1)), exactly from the float tables (Fractions), rounded up:
    what the rounded points, weights and derivative table leave of the rule's exactness on the integral of dL_a."""
    nodes = [Fraction(v) for v in nodes_xi]
    dh = np.asarray(dhatp1_s, dtype=np.float64)
    wf = np.asarray(wf_s, dtype=np.float64).ravel()
    out = []
    for a in range(len(nodes)):
        want = int(nodes[a] == 1) - int(nodes[a] == -1)
        e = sum((Fraction(float(wf[q])) * Fraction(float(dh[a, q])) for q in range(wf.size)), Fraction(0)) - want
        out.append(float(abs(e)) * (1 + 4 * U))
    return np.array(out)

"""
NumPy float64 restatement of the external-load vectors (EL:246-364), the test-side reference of tests/test_el_host.py and
tests/test_loads_gpu.py (the pattern of elem_ref.py / amg_ref.py: plain array code, no GPU, no library call).

Both functions return, per vector entry, the value, the sum of the ABSOLUTE values of its terms and the number m of
terms, so that a test can state the rounding bound of two differently ordered float64 sums of the same two-rounding
products:   |a - b| <= 2 (m + 2) u * sum |terms|,   u = 2^-53   (`bound`).
Each term carries two roundings (weight * f, then hatp * that): relative error <= 2 u + O(u^2) in either evaluation; a sum
of m such terms in any order adds at most (m - 1) u (1 + ...) relative to sum |terms|; two evaluations differ by at most
twice (m + 1) u sum |terms| to first order, and (m + 2) absorbs the second-order terms for every m < 2^40.
"""
import numpy as np

U = 2.0 ** -53


def bound(m, s_abs, extra=2):
    """2 (m + extra) u * sum |terms|, broadcast over the two components."""
    return 2.0 * (np.asarray(m, dtype=float) + extra) * U * s_abs


def volume(elements, n_n, f_v_int, hatp, weight):
    """f_V[c, n] = sum over (e, q) and the local node a with elements[a, e] == n of hatp[a, q] * (weight[e, q] * f[c, e, q]).
    `elements` (n_p, n_e) 0-based.  -> (f (2, n_n), sum_abs (2, n_n), m (n_n,))."""
    elements = np.asarray(elements)
    n_p, n_e = elements.shape
    hatp = np.broadcast_to(np.asarray(hatp, dtype=float), (n_p, np.asarray(hatp).shape[1]))
    n_q = hatp.shape[1]
    w = np.asarray(weight, dtype=float).ravel()
    f = np.asarray(f_v_int, dtype=float).reshape(2, n_e * n_q)
    nodes = np.repeat(elements, n_q, axis=1).ravel()                    # (n_p, n_int) flattened
    hat = np.tile(hatp, (1, n_e))
    out, sabs = np.zeros((2, n_n)), np.zeros((2, n_n))
    for c in range(2):
        terms = (hat * (w * f[c])[None, :]).ravel()
        out[c] = np.bincount(nodes, weights=terms, minlength=n_n)
        sabs[c] = np.bincount(nodes, weights=np.abs(terms), minlength=n_n)
    return out, sabs, np.bincount(nodes, minlength=n_n)


def traction(edges, coordinates, t_int, hatp_s, dhatp1_s, wf_s):
    """f_t[c, n] = sum over (edge e, point q) and the local node a with edges[a, e] == n of
    hatp_s[a, q] * (|J(e, q)| * wf_s[q] * t[c, e, q]),  |J| = sqrt(j1^2 + j2^2),  j_c = sum_a coord_c[edges[a, e]] * dhatp1_s[a, q]:
    a traction value per surface point, the full arc length.  -> (f (2, n_n), sum_abs (2, n_n), m (n_n,))."""
    edges = np.asarray(edges).astype(np.int64)
    coordinates = np.asarray(coordinates, dtype=float)
    n_n = coordinates.shape[1]
    n_p_s, n_e_s = edges.shape
    wf = np.asarray(wf_s, dtype=float).ravel()
    n_q_s = wf.size
    hat = np.broadcast_to(np.asarray(hatp_s, dtype=float), (n_p_s, n_q_s))
    dh = np.broadcast_to(np.asarray(dhatp1_s, dtype=float), (n_p_s, n_q_s))
    t = np.asarray(t_int, dtype=float).reshape(2, n_e_s, n_q_s)
    x, y = coordinates[0][edges], coordinates[1][edges]                 # (n_p_s, n_e_s)
    j1, j2 = np.zeros((n_e_s, n_q_s)), np.zeros((n_e_s, n_q_s))
    for a in range(n_p_s):
        j1 += x[a][:, None] * dh[a][None, :]
        j2 += y[a][:, None] * dh[a][None, :]
    w = np.sqrt(j1 * j1 + j2 * j2) * wf[None, :]                        # (n_e_s, n_q_s)
    nodes = np.repeat(edges[:, :, None], n_q_s, axis=2).ravel()
    out, sabs = np.zeros((2, n_n)), np.zeros((2, n_n))
    for c in range(2):
        terms = (hat[:, None, :] * (w * t[c])[None, :, :]).ravel()
        out[c] = np.bincount(nodes, weights=terms, minlength=n_n)
        sabs[c] = np.bincount(nodes, weights=np.abs(terms), minlength=n_n)
    return out, sabs, np.bincount(nodes, minlength=n_n)

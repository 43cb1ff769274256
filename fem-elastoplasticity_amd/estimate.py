"""
Recovered-stress (Zienkiewicz-Zhu) error indicator and bulk marking: the NumPy twin of the kernels behind
fep_recover_stress_*, fep_estimate_* and fep_mark_bulk_* (include/fep.h, "recovered-stress error indicator"), and the
wrapper that marks on the GPU.  The twin performs the operations of the header in the order written there, one IEEE double
operation each, so its arrays equal the kernels' byte for byte; it needs neither the library nor a GPU.

  tree_sum            T(v): the fixed-order sum (blocks of 256, pairs 128, 64, ..., 1, then the block sums)
  recover_stress_np   s (4, n_int) -> recovered nodal stress (4, n_n)
  estimate_np         -> {'eta2', 'total', 'max', 'n_nonfinite', 's_node'}
  indicator_stats     (total, max, n_nonfinite) of an eta2 array
  mark_bulk           Doerfler marking: the smallest set of largest indicators whose tree sum reaches theta * total, ties included
"""
import ctypes as C

import numpy as np

TREE_BLOCK = 256
VALUE_BITS = 63                                     # bits of a non-negative double: trial passes of the descent


def tree_sum(v):
    """T(v) of include/fep.h as a Python float: v padded with +0.0 to a multiple of 256; in every block of 256 values
    x[i] = x[i] + x[i + s] for s = 128, 64, ..., 1; then T of the block sums until one value is left.  T of nothing is 0.0."""
    x = np.asarray(v, dtype=np.float64).ravel()
    if x.size == 0:
        return 0.0
    while True:
        nb = -(-x.size // TREE_BLOCK)
        buf = np.zeros(nb * TREE_BLOCK)
        buf[:x.size] = x
        buf = buf.reshape(nb, TREE_BLOCK)
        s = TREE_BLOCK // 2
        with np.errstate(all='ignore'):
            while s:
                buf = buf[:, :s] + buf[:, s:2 * s]
                s //= 2
        x = buf[:, 0]
        if nb == 1:
            return float(x[0])


def tree_levels(n):
    """Launches of one pass over n values: the leaves and every level above them."""
    nb, levels = max(1, -(-n // TREE_BLOCK)), 1
    while nb > 1:
        nb, levels = -(-nb // TREE_BLOCK), levels + 1
    return levels


def mark_bulk_launches(n):
    """Kernel launches of fep_mark_bulk_dev on n values: the statistics, 63 trial passes (none for n = 0), the final pass."""
    return ((VALUE_BITS if n > 0 else 0) + 2) * tree_levels(n)


def _incidence(elem, n_n):
    """Node -> elements in the order of the context's lists: (element, local node) ascending.  (iptr, element of each entry)."""
    n_p = elem.shape[0]
    nodes = np.ascontiguousarray(elem.T).ravel()                       # entry e * n_p + a
    order = np.argsort(nodes, kind='stable')
    iptr = np.searchsorted(nodes[order], np.arange(n_n + 1))
    return iptr, order // n_p


def recover_stress_np(elem, weight, s, n_n=None):
    """Recovered nodal stress (4, n_n): per row the mean of `s` (4, n_int) over every integration point of every element
    that holds the node, weighted with `weight` (n_int), summed in the order of the node's incidence list, then q.  A node
    of no element gets 0/0 = NaN."""
    elem = np.asarray(elem, dtype=np.int64)
    n_p, n_e = elem.shape
    w = np.asarray(weight, dtype=np.float64).ravel()
    n_q = w.size // n_e if n_e else 1
    s = np.asarray(s, dtype=np.float64).reshape(4, n_e * n_q)
    n_n = int(elem.max()) + 1 if n_n is None else int(n_n)
    iptr, e_of = _incidence(elem, n_n)
    deg = np.diff(iptr)
    acc, ws = np.zeros((4, n_n)), np.zeros(n_n)
    with np.errstate(all='ignore'):
        for r in range(int(deg.max()) if n_n else 0):
            idx = np.flatnonzero(deg > r)
            e = e_of[iptr[idx] + r]
            for q in range(n_q):
                k = e * n_q + q
                acc[:, idx] = acc[:, idx] + w[k] * s[:, k]
                ws[idx] = ws[idx] + w[k]
        return acc / ws


def _cnorm(d, G, K):
    """c(d) = d : C^-1 : d for stress differences d (4, n), rows 11, 22, 12, 33."""
    tr = (d[0] + d[1]) + d[3]
    m = tr / 3.0
    e0, e1, e3 = d[0] - m, d[1] - m, d[3] - m
    dev = ((e0 * e0 + e1 * e1) + e3 * e3) + 2.0 * (d[2] * d[2])
    return dev / (2.0 * G) + (tr * tr) / (9.0 * K)


def indicator_stats(eta2):
    """(total, max, n_nonfinite) of fep_estimate_*: the tree sum and the largest positive of the finite values, and the number
    of values that are not finite."""
    x = np.asarray(eta2, dtype=np.float64).ravel()
    fin = np.isfinite(x)
    v = np.where(fin, x, 0.0)
    pos = v[v > 0]
    return tree_sum(v), (float(pos.max()) if pos.size else 0.0), int(x.size - np.count_nonzero(fin))


def estimate_np(elem, weight, shear, bulk, hatp, s, n_n=None):
    """The indicator of include/fep.h on host arrays: `elem` (n_p, n_e) 0-based, `weight` (n_int), `shear`, `bulk` scalars or
    (n_int), `hatp` (n_p, n_q) basis values (ignored for P1: n_q = 1), `s` (4, n_int).  Returns {'eta2' (n_e,), 'total',
    'max', 'n_nonfinite', 's_node' (4, n_n)}."""
    elem = np.asarray(elem, dtype=np.int64)
    n_p, n_e = elem.shape
    w = np.asarray(weight, dtype=np.float64).ravel()
    n_q = w.size // n_e
    n_int = n_e * n_q
    s = np.asarray(s, dtype=np.float64).reshape(4, n_int)
    G = np.broadcast_to(np.asarray(shear, dtype=np.float64).ravel(), (n_int,))
    K = np.broadcast_to(np.asarray(bulk, dtype=np.float64).ravel(), (n_int,))
    sn = recover_stress_np(elem, w, s, n_n)
    with np.errstate(all='ignore'):
        if n_q == 1:
            d = [sn[:, elem[a]] - s for a in range(3)]
            b = ((d[0] + d[1]) + d[2]) / 3.0
            c = [_cnorm(d[a] - b, G, K) for a in range(3)]
            eta2 = w * (_cnorm(b, G, K) + ((c[0] + c[1]) + c[2]) / 12.0)
        else:
            h = np.ascontiguousarray(np.broadcast_to(np.asarray(hatp, dtype=np.float64), (n_p, n_q)))
            r = np.zeros((n_q, 4, n_e))
            for a in range(n_p):
                v = sn[:, elem[a]]
                for q in range(n_q):
                    r[q] = r[q] + h[a, q] * v
            eta2 = np.zeros(n_e)
            for q in range(n_q):
                k = np.arange(n_e) * n_q + q
                eta2 = eta2 + w[k] * _cnorm(r[q] - s[:, k], G[k], K[k])
    total, vmax, n_bad = indicator_stats(eta2)
    return {'eta2': eta2, 'total': total, 'max': vmax, 'n_nonfinite': n_bad, 's_node': sn}


def _check_theta(theta):
    theta = float(theta)
    if not (0.0 < theta <= 1.0):
        raise ValueError(f'theta must lie in (0, 1], got {theta}')
    return theta


def _mark_bulk_np(x, theta):
    fin = np.isfinite(x)
    total, vmax, _ = indicator_stats(x)
    goal = theta * total
    with np.errstate(invalid='ignore'):
        def tail(t):
            return tree_sum(np.where(fin & (x >= t), x, 0.0))

        t_star = np.inf
        if total > 0:
            cand, top = 0, int(np.float64(vmax).view(np.uint64))
            for bit in range(VALUE_BITS - 1, -1, -1):
                trial = cand | (1 << bit)
                if trial <= top and tail(float(np.uint64(trial).view(np.float64))) >= goal:
                    cand = trial
            t_star = float(np.uint64(cand).view(np.float64))
        marked = fin & (x > 0) & (x >= t_star)
        return marked, np.array([t_star, tail(t_star), float(np.count_nonzero(marked)), total])


def mark_bulk(eta2, theta, device=None):
    """Bulk (Doerfler) marking of include/fep.h: with total = T(finite values), the elements with eta2 >= t*, t* the largest
    value whose tail sum tail(t*) = T(values >= t*) still reaches theta * total; ties at t* are all marked, non-finite and
    non-positive values never.  Returns (marked, out), out = [t*, tail(t*), number marked, total].
      device=None  the NumPy twin; `marked` a bool array
      device=k     fep_mark_bulk_host on GPU k (`eta2` a host array) — or, when `eta2` is a torch tensor of a GPU,
                   fep_mark_bulk_dev on that GPU's current stream: `marked` a uint8 tensor that DeviceMesh.mark(on_device=True)
                   takes as it is, `out` a float64 tensor of 4; nothing is read back or synchronised."""
    theta = _check_theta(theta)
    if type(eta2).__module__.split('.')[0] == 'torch':
        import torch
        from . import _lib
        if eta2.dtype != torch.float64 or eta2.dim() != 1 or not eta2.is_contiguous() or not eta2.is_cuda:
            raise ValueError('device indicators are a contiguous float64 tensor of (n,) on a GPU')
        dev = eta2.device.index
        marked = torch.empty(eta2.shape[0], dtype=torch.uint8, device=eta2.device)
        out = torch.empty(4, dtype=torch.float64, device=eta2.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().fep_mark_bulk_dev(dev, stream, int(eta2.shape[0]), C.c_void_p(eta2.data_ptr()), theta,
                                                C.c_void_p(marked.data_ptr()), C.c_void_p(out.data_ptr())), 'fep_mark_bulk_dev')
        return marked, out
    x = np.ascontiguousarray(eta2, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError(f'eta2: one value per element (n,), got {x.shape}')
    if device is None:
        return _mark_bulk_np(x, theta)
    from . import _lib
    marked, out = np.zeros(x.size, dtype=np.uint8), np.zeros(4)
    _lib.check(_lib.lib().fep_mark_bulk_host(int(device), x.size, _lib.ptr(x), theta, _lib.ptr(marked), _lib.ptr(out)),
               'fep_mark_bulk_host')
    return marked.view(np.bool_), out

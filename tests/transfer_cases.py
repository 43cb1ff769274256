"""
Cases shared by test_transfer_host.py and test_transfer_gpu.py: parent and child meshes with the children's parents and
corner codes, for P1, P2 and P4, and the helpers that say — independently of the twin's vectorised form — which pair owns
a child node and which parent point a child point copies.

A case is a dict: 'name', 'coord' / 'elem' (the P1 parent), 'marked' (None: uniform refinement), 'curves', 'coord_child' /
'elem_child' (the P1 child), 'parent', 'corners'.  `raised(case, t)` gives the element tables of type t on both meshes.
"""
import functools

import numpy as np

import marked_cases as mc

fep, mp = mc.fep, mc.mp

N_P = {'P1': 3, 'P2': 6, 'P4': 15}
N_Q = {'P1': 1, 'P2': 7, 'P4': 12}


def flower(slot):
    """marked_cases.ONE_TRIANGLE[slot] as element 0, with one neighbour across each of its edges (elements 1, 2, 3 across the
    edges 0, 1, 2: the opposite vertex mirrored in the edge's midpoint, so every neighbour's longest edge is the shared one or
    an outer one).  Marking neighbours alone gives element 0 every combination of edge flags its reference edge allows."""
    v = np.array(mc.ONE_TRIANGLE[slot], dtype=np.float64)
    coord, elem = [tuple(p) for p in v], [(0, 1, 2)]
    for k in range(3):
        a, b, c = k, (k + 1) % 3, (k + 2) % 3
        coord.append(tuple(v[a] + v[b] - v[c]))
        elem.append((b, a, 3 + k))
    return np.array(coord).T, np.array(elem, dtype=np.int64).T


def _case(name, coord, elem, marked, curves=None):
    coord, elem = np.asarray(coord, dtype=np.float64), np.asarray(elem, dtype=np.int64)
    if marked is None:
        cc, ec = fep.refine_uniform(coord, elem, curves=curves)
        corners, parent = fep.uniform_corners(elem.shape[1])
    else:
        marked = np.asarray(marked) != 0
        cc, ec, parent = fep.refine_marked(coord, elem, marked, curves=curves)
        corners = fep.child_corners(coord, elem, marked)
    return {'name': name, 'coord': coord, 'elem': elem, 'marked': marked, 'curves': curves, 'coord_child': cc, 'elem_child': ec,
            'parent': parent, 'corners': corners}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for slot in (0, 1, 2):
        coord, elem = flower(slot)
        r = slot                                                                        # the reference edge of element 0
        for p_on in (0, 1):
            for q_on in (0, 1):
                marked = np.zeros(4, dtype=bool)
                marked[1 + r] = True
                marked[1 + (r + 1) % 3], marked[1 + (r + 2) % 3] = p_on, q_on
                out.append(_case(f'flower{slot}-p{p_on}q{q_on}', coord, elem, marked))
    out.append(_case('pair-01', mc.PAIR_COORD, mc.PAIR_ELEM, [0, 1]))
    out.append(_case('pair-10', mc.PAIR_COORD, mc.PAIR_ELEM, [1, 0]))
    coord, elem = mc.chain(600)
    first, last = np.zeros(600, dtype=bool), np.zeros(600, dtype=bool)
    first[0], last[599] = True, True
    out.append(_case('chain-first', coord, elem, first))
    out.append(_case('chain-last', coord, elem, last))
    coord, elem = mc.unstructured()
    out.append(_case('unstructured', coord, elem, mc.round_marks(1, elem, np.random.default_rng(11))))
    coord, elem = mc.tunnel()
    out.append(_case('tunnel-curved', coord, elem, mc.near_tunnel(None, coord, elem), curves=(fep.tsx_tunnel.TSX_HOLE,)))
    out.append(_case('tunnel-identity', coord, elem, np.zeros(887, dtype=bool)))
    coord, elem = mc.perturbed_square()
    out.append(_case('square-uniform', coord, elem, None))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c['name'] == name)


#: the cases every element type runs on (all shapes; shared nodes; a curved wall with 887 parents; the uniform table) —
#: P1 runs on all of them
HIGH_ORDER = ('flower0-p1q1', 'flower1-p0q1', 'flower2-p1q0', 'flower0-p0q0', 'pair-10', 'tunnel-curved', 'square-uniform')


def names(t):
    return [c['name'] for c in cases()] if t == 'P1' else list(HIGH_ORDER)


@functools.lru_cache(maxsize=None)
def raised(name, t):
    """(elem_parent (n_p, n_e), n_n_parent, elem_child (n_p, n_child), n_n_child, coord_parent_ext, coord_child_ext) of type t."""
    c = case(name)
    if t == 'P1':
        return c['elem'], c['coord'].shape[1], c['elem_child'], c['coord_child'].shape[1], c['coord'], c['coord_child']
    curves = list(c['curves']) if c['curves'] else None
    hp = fep.create_midpoints(t, c['coord'], c['elem'], curves=curves)
    hc = fep.create_midpoints(t, c['coord_child'], c['elem_child'], curves=curves)
    return (hp['elem_ext'], hp['coord_ext'].shape[1], hc['elem_ext'], hc['coord_ext'].shape[1], hp['coord_ext'], hc['coord_ext'])


def nodal_field(n_n, n_comp, seed=5):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, size=(n_n, n_comp))


def point_field(n_rows, n_int, seed=6):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, size=(n_rows, n_int))


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def near_corner(hist, coord, elem):
    """Marks by geometry alone: centroids within 2 of the re-entrant corner (5, 5) of the cut-out square."""
    cx, cy = coord[0][elem].mean(axis=0), coord[1][elem].mean(axis=0)
    return (cx - 5) ** 2 + (cy - 5) ** 2 < 4.0


# Largest difference, relative to max |s|, between the point stresses of the transferred state and the parent's copied by
# `parent`, measured on the CPU restatement in cpu_adaptive_cycle(): 1.8e-15 (the strain of a child is its parent's up to the
# rounding of B u on other coordinates, the plastic strain is a copy).  The GPU sums in another order: a factor 8.
STRESS_TOL_CPU = 2e-15
STRESS_TOL_GPU = 8 * STRESS_TOL_CPU


@functools.lru_cache(maxsize=None)
def cpu_adaptive_cycle():
    """solve_cutout_cyclic at level 0 on the CPU restatement, refined after step 3 near the corner; never modified."""
    from vm_ref import VMRefContext
    return fep.solve_cutout_cyclic('P1', level=0, context_factory=VMRefContext, linear_solver='direct', adapt_at=(3,), mark=near_corner)


def stress_gap(row, make_context):
    """max |s_child - s_parent[:, parent]| / max |s_parent| of a row of hist['adapt'], s_child from a non-accepting step of a
    fresh context on the child mesh at the transferred state."""
    import vm_cases as vc
    ctx = make_context(row['elem'], row['coords'], *fep.element_tables('P1'))
    ctx.set_model('vm')
    ctx.set_materials(vc.SHEAR, vc.BULK, vc.HARDENING, vc.YIELD)
    s = np.asarray(ctx.step(row['U'], row['Ep'].copy(), want=('s',))['s'])
    ctx.close()
    want = row['s'][:, row['parent']]
    return float(np.abs(s - want).max() / np.abs(want).max())


# ---- ownership and sources, by plain loops ------------------------------------------------------------------------------------
def owner_pairs(elem_child, n_n_child):
    """owner child and local node of every child node (-1: a node of no element): the first pair in the lexicographic order."""
    n_p, n_child = elem_child.shape
    own_ch, own_j = np.full(n_n_child, -1, dtype=np.int64), np.full(n_n_child, -1, dtype=np.int64)
    for ch in range(n_child):
        for j in range(n_p):
            n = int(elem_child[j, ch])
            if own_ch[n] < 0:
                own_ch[n], own_j[n] = ch, j
    return own_ch, own_j


def point_sources(t, parent, corners):
    """The parent point each child point copies, (n_child n_q), from the tables alone."""
    tab = fep.transfer_tables(t)
    n_q = N_Q[t]
    src = np.empty(parent.size * n_q, dtype=np.int64)
    for ch in range(parent.size):
        s = int(tab['shape_of_code'][int(corners[0, ch]) + 6 * int(corners[1, ch]) + 36 * int(corners[2, ch])])
        assert s >= 0
        for k in range(n_q):
            src[ch * n_q + k] = int(parent[ch]) * n_q + int(tab['near'][s, k])
    return src


def same_but_nan_sign(a, b):
    """Bit-equal, but for the sign bit of a NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    ia, ib = a.view(np.uint64).copy(), b.view(np.uint64).copy()
    sign = np.uint64(1) << np.uint64(63)
    ia[np.isnan(a)] &= ~sign
    ib[np.isnan(b)] &= ~sign
    return bool((ia == ib).all())

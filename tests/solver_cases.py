"""
Meshes for the solver tests that leave the footing's squares (test_solver_cases_host.py, test_solver_shapes_gpu.py): the
tsx tunnel as P1 / P2 / P4, renumbered Delaunay triangulations, fans with one node of ~250 blocks and a mesh with nodes of
no element.  Per case: the mesh, the free-DOF mask, `coarse_nodes`, which form of amg_ref.VCycle the device must equal,
the nodes per level and whether tail_kernel runs (both pinned by the host test: they depend on the seeds and on the
order in which one generator serves the jitter and the renumbering), and the ulp
sensitivity of the restated iterates the host test measures (the GPU test's bound is derived from it).  No GPU here.

Free DOFs: tsx cases carry the rollers of newton._tsx_setup; Delaunay cases rollers on the bounding box; fan cases fix every
node of radius > 1.7 (the outer ring and, raised, the nodes between its vertices); the small rectangles pin the lower right
corner and put the lower left one on a roller (a 1 x 1 cell then keeps 5 free DOFs and, under this choice of the three, four
distinct CG iterates for every right-hand side: with rollers on the left edge the one-node right-hand side converges in
four); a node of no element is fixed in both DOFs whatever its case; the rectangles of FORMS (test_solver_forms_gpu.py) have
their bottom row fixed vertically and their left column horizontally (only the corner in both: a node fixed in both
directions is isolated on level 1 and below, fep_aggregate_host keeps it as an aggregate of its own on every level, and a
whole row of them would put the coarsest level beyond the refresh's 256 DOFs).

The displacement of `displacement()` gives a plastic tangent with dp_materials: with x, y the coordinates shifted to the
bounding box's corner and divided by its larger side L,
    U = amp * L * (-0.4 x + 1.5 x y [y > 0.4],  -0.5 y - 0.5 y [x >= 0.5]),     amp = 1e-4
(at 3e-4 the fan P2 tangent is indefinite and the restated CG itself breaks down).  The host test checks for every case
that this tangent has plastic points and that the restatement runs on it without breakdown; no case needed a lower amp.
"""
from importlib import import_module

import numpy as np
import scipy.sparse as ssp

import amg_ref
import fan_mesh
import meshes
from conftest import dp_materials, load_golden, relerr
from test_vcycle_gpu import K_ITERS, _rhs as rhs

AMP = 1e-4

# name: kind, element type, size parameter, coarse_nodes, refresh (the VCycle form the device must equal: False where the
# coarsest level exceeds the 256 DOFs fep_solver_amg_enable_refresh takes), nodes per level, tail_runs, amp,
# ulp sensitivity of x_1 .. x_4 under the V-cycle of that form and under block Jacobi (test_solver_cases_host.py measures
# them on K_elast and the tangent of the oracle, three right-hand sides each, and asserts that it finds these figures, to a factor of two).
CASES = {
    'tsx-P1':        dict(kind='tsx', et='P1', coarse_nodes=30, refresh=True, nodes=(476, 54, 9), tail=True, amp=AMP,
                          sens_vcycle=8.3e-15, sens_jacobi=9.6e-16),
    'tsx-P2':        dict(kind='tsx', et='P2', coarse_nodes=30, refresh=True, nodes=(1839, 72, 9), tail=True, amp=AMP,
                          sens_vcycle=3.2e-14, sens_jacobi=3.1e-15),
    'tsx-P4':        dict(kind='tsx', et='P4', coarse_nodes=30, refresh=True, nodes=(7226, 82, 9), tail=True, amp=AMP,
                          sens_vcycle=3.6e-14, sens_jacobi=1.2e-15),
    'delaunay40-P1': dict(kind='delaunay', et='P1', M=40, coarse_nodes=30, refresh=True, nodes=(1681, 172, 15), tail=True,
                          amp=AMP, sens_vcycle=2.6e-14, sens_jacobi=1.3e-15),
    'delaunay14-P2': dict(kind='delaunay', et='P2', M=14, coarse_nodes=30, refresh=True, nodes=(841, 46, 8), tail=True,
                          amp=AMP, sens_vcycle=9.6e-15, sens_jacobi=1.3e-15),
    'delaunay8-P4':  dict(kind='delaunay', et='P4', M=8, coarse_nodes=30, refresh=True, nodes=(1089, 23), tail=False,
                          amp=AMP, sens_vcycle=2.5e-14, sens_jacobi=1.9e-15),
    'delaunay50-P1': dict(kind='delaunay', et='P1', M=50, coarse_nodes=30, refresh=True, nodes=(2601, 263, 21), tail=True,
                          amp=AMP, sens_vcycle=1.3e-14, sens_jacobi=1.3e-15),
    'delaunay58-P1': dict(kind='delaunay', et='P1', M=58, coarse_nodes=30, refresh=True, nodes=(3481, 346, 25), tail=True,
                          amp=AMP, sens_vcycle=2.6e-14, sens_jacobi=1.2e-15),
    'delaunay62-P1': dict(kind='delaunay', et='P1', M=62, coarse_nodes=30, refresh=True, nodes=(3969, 392, 27), tail=False,
                          amp=AMP, sens_vcycle=3.0e-14, sens_jacobi=1.5e-15),
    'delaunay72-P1': dict(kind='delaunay', et='P1', M=72, coarse_nodes=30, refresh=True, nodes=(5329, 524, 32, 6), tail=True,
                          amp=AMP, sens_vcycle=5.3e-14, sens_jacobi=1.1e-15),
    'fan250-P1':     dict(kind='fan', et='P1', k=250, coarse_nodes=30, refresh=False, nodes=(501, 251), tail=False, amp=AMP,
                          sens_vcycle=2.0e-13, sens_jacobi=1.3e-14),
    'fan84-P2':      dict(kind='fan', et='P2', k=84, coarse_nodes=30, refresh=False, nodes=(589, 203, 169), tail=False,
                          amp=AMP, sens_vcycle=9.7e-14, sens_jacobi=8.4e-15),
    'fan24-P4':      dict(kind='fan', et='P4', k=24, coarse_nodes=30, refresh=False, nodes=(625, 205, 193), tail=False,
                          amp=AMP, sens_vcycle=2.9e-14, sens_jacobi=2.1e-15),
    'orphans-P1':    dict(kind='orphans', et='P1', M=20, coarse_nodes=30, refresh=True, nodes=(441, 59, 17), tail=True,
                          amp=AMP, sens_vcycle=1.1e-14, sens_jacobi=1.9e-15),
}
# The row-to-lane mapping of spmv_kernel and its kin (NODES_PER_BLOCK = 128, 8 lanes per node): exactly one workgroup, one node
# into the second, half a lane group's pass.  Block Jacobi and spmv only (no hierarchy on 4 nodes).
SMALL = {
    'rect-15x7': dict(kind='rect', et='P1', cells=(15, 7), n_nodes=128, amp=AMP, sens_jacobi=1.2e-15),
    'rect-42x2': dict(kind='rect', et='P1', cells=(42, 2), n_nodes=129, amp=AMP, sens_jacobi=1.2e-15),
    'rect-1x1':  dict(kind='rect', et='P1', cells=(1, 1), n_nodes=4, amp=AMP, sens_jacobi=4.3e-14),
}
ALL = dict(CASES, **SMALL)
FULL_SOLVES = ('tsx-P4', 'delaunay58-P1', 'fan250-P1', 'orphans-P1')
# The kernel forms the device picks by size (test_solver_forms_gpu.py): rectangles of fep.rect_mesh under
# amg_ref.singleton_hierarchy, whose level 1 has as many nodes as the mesh (the names give nodes per side for P1, cells for P2);
# four_pass: whether level 1 takes node3_kernel's four-nodes-per-lane-group form (from 128 * 2048 = 262 144 nodes);
# nodes, tail, sens_vcycle as above, on the oracle's matrices (test_solver_cases_host.py).  Not in ALL: block Jacobi and spmv have no such form.
FORMS = {
    'P1-511x513': dict(kind='form', et='P1', cells=(510, 512), n_nodes=262143, four_pass=False, amp=AMP,
                       nodes=(262143, 262143, 29242, 2431, 157, 12), tail=True, sens_vcycle=9.6e-13),
    'P1-512x512': dict(kind='form', et='P1', cells=(511, 511), n_nodes=262144, four_pass=True, amp=AMP,
                       nodes=(262144, 262144, 29242, 2491, 173, 13), tail=True, sens_vcycle=1.1e-12),
    'P1-517x508': dict(kind='form', et='P1', cells=(516, 507), n_nodes=262636, four_pass=True, amp=AMP,
                       nodes=(262636, 262636, 29410, 2441, 158, 13), tail=True, sens_vcycle=2.1e-12, sens_full=4.9e-13),
    'P2-256':     dict(kind='form', et='P2', cells=(256, 256), n_nodes=263169, four_pass=True, amp=AMP,
                       nodes=(263169, 263169, 16513, 703, 37), tail=False, sens_vcycle=2.8e-12),
}
FORMS_FULL_SOLVE = 'P1-517x508'              # sens_full: the same sensitivity of the full solve's last iterate
FORMS_COARSE_NODES = 64                      # (what setup_amg caps coarse_nodes at under the refresh)
EVERY = dict(ALL, **FORMS)

_MESH = {}


def mesh(name):
    """(elements (n_p, n_e) int64, coordinates (2, n_n), element type); cached, read-only."""
    if name not in _MESH:
        c = EVERY[name]
        et = c['et']
        if c['kind'] == 'tsx':
            g = load_golden('tsx')
            elem, coord = (g['elem'], g['coord']) if et == 'P1' else (g[et.lower() + '_elem'], g[et.lower() + '_coord'])
        elif c['kind'] == 'delaunay':                        # one generator for the jitter and then the numbering
            rng = np.random.default_rng(7)
            elem, coord = meshes.renumber(*meshes.delaunay(et, c['M'], rng), rng)
        elif c['kind'] == 'orphans':
            # the triangulation's last 40 elements dropped BEFORE the renumbering (they are neighbours there, so nodes lose
            # all their elements; after it the 40 would be scattered and leave at most one such node)
            rng = np.random.default_rng(7)
            elem, coord = meshes.delaunay(et, c['M'], rng)
            elem, coord = meshes.renumber(meshes.drop_last(elem, 40), coord, rng)
        elif c['kind'] == 'fan':
            elem, coord = fan_mesh.fan_mesh(c['k'], et, shuffle=True)
        elif c['kind'] == 'form':
            m = import_module('fem-elastoplasticity_amd').rect_mesh(*c['cells'], et)
            elem, coord = m['elements'], m['coordinates']
        else:
            elem, coord = meshes.rect(et, *c['cells'])
        elem = np.ascontiguousarray(elem, dtype=np.int64)
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        elem.setflags(write=False)
        coord.setflags(write=False)
        _MESH[name] = (elem, coord, et)
    return _MESH[name]


def orphan_nodes(name):
    elem, coord, _ = mesh(name)
    return np.flatnonzero(np.bincount(elem.ravel(), minlength=coord.shape[1]) == 0)


def free_dofs(name):
    """bool (n_dof,), DOF = 2 * node + component."""
    elem, coord, _ = mesh(name)
    kind = EVERY[name]['kind']
    x, y = coord
    Q = np.ones(coord.shape, dtype=bool)
    if kind == 'tsx':                                        # newton._tsx_setup, TSX:1695-1699
        Q[0, x < -49.99] = False
        Q[0, x > 49.99] = False
        Q[1, y < -49.99] = False
        Q[1, y > 49.99] = False
    elif kind in ('delaunay', 'orphans'):
        Q[0, (x == x.min()) | (x == x.max())] = False
        Q[1, (y == y.min()) | (y == y.max())] = False
    elif kind == 'fan':
        Q[:, np.hypot(x, y) > 1.7] = False
    elif kind == 'form':                                     # bottom row fixed vertically, left column horizontally
        Q[1, y == y.min()] = False
        Q[0, x == x.min()] = False
    else:                                                    # statically determinate: a pin and a roller
        Q[:, (x == x.max()) & (y == y.min())] = False
        Q[1, (x == x.min()) & (y == y.min())] = False
    Q[:, orphan_nodes(name)] = False
    return Q.flatten(order='F')


def displacement(name):
    """(n_dof,) in DOF order; see the module docstring."""
    _, coord, _ = mesh(name)
    lo = coord.min(axis=1)
    L = (coord.max(axis=1) - lo).max()
    x, y = (coord[0] - lo[0]) / L, (coord[1] - lo[1]) / L
    U = EVERY[name]['amp'] * L * np.stack([-0.4 * x + 1.5 * x * y * (y > 0.4), -0.5 * y - 0.5 * y * (x >= 0.5)])
    return U.flatten(order='F')


def row_blocks(name):
    """Node-pair blocks per node row of K (0 for a node of no element)."""
    elem, coord, _ = mesh(name)
    n_n = coord.shape[1]
    a = np.repeat(elem, elem.shape[0], axis=0).ravel()
    b = np.tile(elem, (elem.shape[0], 1)).ravel()
    return np.bincount(np.unique(a * n_n + b) // n_n, minlength=n_n)


def oracle_matrices(name):
    """{'elastic': K_elast, 'plastic': the tangent at `displacement`} from oracle.fep_oracle (sorted CSR), and the plastic
    points of the tangent as (smooth, apex, all points)."""
    from oracle import fep_oracle as orc
    fep = import_module('fem-elastoplasticity_amd')
    elem, coord, et = mesh(name)
    d1, d2, wf = fep.element_tables(et)
    n_int = elem.shape[1] * np.size(wf)
    shear, bulk, eta, c = dp_materials(n_int)
    K, B, w, iD, jD, D = orc.elastic_setup(elem, coord, shear, bulk, d1, d2, wf)
    ctx = dict(K_elast=K, B=B, D_elast=D, weight=w, iD=iD, jD=jD, shear=shear, bulk=bulk, eta=eta, c=c)
    U = displacement(name).reshape((2, -1), order='F')
    _, cp, K_t, _ = orc.hot_path(U, np.zeros((4, n_int)), ctx)
    out = {}
    for key, M in (('elastic', K), ('plastic', K_t)):
        M = ssp.csr_matrix(M)
        M.sum_duplicates()
        M.sort_indices()
        out[key] = M
    return out, (int(cp['n_smooth']), int(cp['n_apex']), n_int)


def hierarchy(name, K_el):
    _, coord, _ = mesh(name)
    return amg_ref.solver.build_amg_hierarchy(K_el, free_dofs(name), coord, coarse_nodes=min(ALL[name]['coarse_nodes'], 64))


def level_nodes(levels, n_dof):
    return (n_dof // 2,) + tuple(lv['size'][0] // 3 for lv in levels)


def level_sizes(K, levels):
    """KrylovSolver.amg_levels from a hierarchy built on the host."""
    return [(K.shape[0], K.nnz)] + [lv['size'] for lv in levels]


def perturbed(K, seed=23):
    """K with every value multiplied by 1 + 2.2e-16 uniform(-1, 1): one unit of double rounding on the operands."""
    Kp = ssp.csr_matrix(K, copy=True)
    Kp.data = Kp.data * (1.0 + 2.2e-16 * np.random.default_rng(seed).uniform(-1.0, 1.0, Kp.data.size))
    return Kp


def ulp_sensitivity(K, qf, make_M, cg):
    """Largest relerr of x_1 .. x_K_ITERS between the restatement on K and on `perturbed(K)` over the three right-hand
    sides.  make_M(K) -> the preconditioner of that matrix."""
    Kp = perturbed(K)
    M, Mp = make_M(K), make_M(Kp)
    worst = 0.0
    for b in rhs(qf).values():
        h = cg(K, qf, b, M, max_iter=K_ITERS, keep=True)['history']
        hp = cg(Kp, qf, b, Mp, max_iter=K_ITERS, keep=True)['history']
        if len(h) != K_ITERS or len(hp) != K_ITERS:
            return np.inf
        worst = max([worst] + [relerr(a[0], c[0]) for a, c in zip(hp, h)])
    return worst


def forms_full_solve_rhs(K, qf):
    """(x, b = Q K x) for a random x, 0 on constrained DOFs: the right-hand side of the forms' full solve (the restated CG
    takes 45 iterations to rtol 1e-10 on K_elast with it, against 300 with a random b on the plastic tangent)."""
    x = np.where(qf, np.random.default_rng(31).normal(size=qf.size), 0.0)
    return x, np.where(qf, K @ x, 0.0)


def bound(floor, sensitivity):
    """A case's bound: the larger of the squares' bound and 30 x its ulp sensitivity (the ratio the squares' bounds keep to
    their measured values, rounded down), never above 1e-9 (the restatement without the single-precision roundings is
    5e-8 to 2e-5 away)."""
    return min(max(floor, 30.0 * sensitivity), 1e-9)

#!/usr/bin/env python3
"""
Golden fixture of the external loads and of the Elasticity2D driver: `el_loads.npz`, recorded from the reference's
own functions (imported read-only, as make_golden.py does; arrays and scalars only, no reference text).

    python tests/golden/make_golden_el.py

Content, keys prefixed `<type>_l<level>_` for the cut-out square of EL:481-942 (P1, Q1, Q2 at level 1, P1 at level 3):
  mesh dictionary     level 1: every key as an array (`elements` 1-based as generated, `neumann_nodes` 0-based float);
                      level 3: SHA-256 and shape of every key (make_golden.sha; elements as int64)
  weight              second result of the reference's get_elastic_stiffness_matrix
  f_V, f_t            get_vector_volume / get_vector_traction of the driver's constant loads (0, -1) and (0, 450), dense (2, n_n)
  u, energy_replay    the driver EL:1052-1179 replayed with the reference's functions (it returns nothing): dense solve on
                      the free DOFs, stored energy 0.5 u.K u - (f_t + f_V).u
  energy              the number the driver itself prints as 'Stored energy' (equal to the replay's to ~1e-13 relative)
  level 1 only:
  jig_coordinates, jig_weight, jig_f_V_int, jig_f_V      seeded random body force on a copy of the mesh whose interior
                      nodes are moved by up to 8 % of a cell (as make_golden.gen_setup jiggles)
  ft_int_var, f_t_var a NON-constant f_t_int and what the reference makes of it (it applies the last point's value)
Surface tables `<type>_xi_s, _wf_s, _hatp_s, _dhatp1_s` for P1, P2, Q1, Q2.

Meshes without a cut-out counterpart (get_vector_volume does not care where a mesh comes from):
  P2sq_*   EL functions on the DP P2 square of mesh_dp.npz (`P2_n4_*`, 4 x 4 cells on [0, 4]^2, 0-based elements):
           weight, constant and random f_V_int -> f_V; traction on the TOP EDGES, composed here from the coordinates:
           the nodes with y == 4 sorted by x are n_0 .. n_8 and edge k = (n_2k, n_2k+2, n_2k+1), k = 0 .. 3 (end, end,
           middle); stored as `P2sq_edges` (3, 4) float 0-based like `neumann_nodes`, with a constant and a non-constant
           f_t_int
  P4tx_*   the TSX twin (TSX:311-357) on the P4 tunnel mesh of tsx.npz (`p4_coord`, `p4_elem`): weight, constant and
           random f_V_int -> f_V
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load_reference, save, sha                    # noqa: E402

YOUNG, POISSON = 206900, 0.29
VOLUME_FORCE, TRACTION_FORCE = np.array([[0, -1]]), np.array([[0, 450]])
MESH_KEYS = ('coordinates', 'elements', 'surface', 'neumann_nodes', 'dirichlet_nodes', 'Q')


def _dense(v):
    return np.asarray(v.todense())


def _el_case(m, t, level, arrs):
    et = m.LagrangeElementType[t]
    tag = f'{t}_l{level}_'
    mesh = m.assemble_mesh(level, et, 10, 5)
    for k in MESH_KEYS:
        a = np.asarray(mesh[k])
        if k == 'elements':
            a = a.astype(np.int64)
        if level == 1:
            arrs[tag + k] = a.copy()
        else:
            arrs[tag + k + '_sha'] = sha(a)
            arrs[tag + k + '_shape'] = np.array(a.shape)
    xi, wf = m.get_quadrature_volume(et)
    xi_s, wf_s = m.get_quadrature_surface(et)
    hatp, d1, d2 = m.get_local_basis_volume(et, xi)
    hatp_s, d1_s = m.get_local_basis_surface(et, xi_s)
    elem1 = np.asarray(mesh['elements']).astype(np.int64).copy()
    coord = np.asarray(mesh['coordinates'])
    n_int = elem1.shape[1] * wf.size
    shear = YOUNG / (2 * (1 + POISSON)) * np.ones(n_int)
    bulk = YOUNG / (3 * (1 - 2 * POISSON)) * np.ones(n_int)
    elem = elem1.copy()
    K, weight = m.get_elastic_stiffness_matrix(elem, coord, shear, bulk, d1, d2, wf)       # shifts `elem` to 0-based
    f_V_int = np.dot(VOLUME_FORCE.transpose(), np.ones((1, n_int)))
    f_V = m.get_vector_volume(elem, coord, f_V_int, hatp, weight)
    n_int_s = mesh['neumann_nodes'].shape[1] * len(wf_s)
    f_t_int = np.dot(TRACTION_FORCE.transpose(), np.ones((1, n_int_s)))
    f_t = m.get_vector_traction(mesh['neumann_nodes'], coord, f_t_int, hatp_s, d1_s, wf_s)
    # the driver's processing, with the free block taken densely
    ud = 0.5 * mesh['dirichlet_nodes']
    fV, fT = f_V.reshape((-1, 1), order='F'), f_t.reshape((-1, 1), order='F')
    f = np.asarray(fT + fV - (K @ ud.reshape((-1, 1), order='F'))).ravel()
    q = np.asarray(mesh['Q']).reshape(-1, order='F')
    Kqq = K.tocsr()[q][:, q].toarray()
    u = ud.copy()
    u.transpose()[mesh['Q'].transpose()] = np.linalg.solve(Kqq, f[q])
    uf = u.flatten(order='F')
    energy = float(0.5 * uf @ (K @ uf) - np.asarray((fT + fV).todense()).ravel() @ uf)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.elasticity_fem(et, level, False)                                  # prints 'Stored energy: <repr>'
    printed = float(buf.getvalue().strip().splitlines()[-1].split(':')[1])
    print(f'  {t} level {level}: n_n {coord.shape[1]}  stored energy: replay {energy!r}, driver {printed!r}')
    arrs.update({tag + 'weight': np.asarray(weight), tag + 'f_V': _dense(f_V), tag + 'f_t': _dense(f_t),
                 tag + 'u': u, tag + 'energy': np.array(printed), tag + 'energy_replay': np.array(energy)})
    if level != 1:
        return
    rng = np.random.default_rng({'P1': 21, 'Q1': 22, 'Q2': 23}[t])
    h = 10 / (10 * 2 ** level)
    x, y = coord
    boundary = np.logical_or.reduce([x == 0, x == 10, y == 0, y == 10, np.logical_and(x == 5, y <= 5),
                                     np.logical_and(y == 5, x <= 5)])
    interior = np.logical_not(boundary)
    jig = coord.copy()
    jig[:, interior] += rng.uniform(-0.08, 0.08, size=(2, int(interior.sum()))) * h
    _, jw = m.get_elastic_stiffness_matrix(elem1.copy(), jig, shear, bulk, d1, d2, wf)
    jf = rng.normal(0, 1, size=(2, n_int))
    arrs.update({tag + 'jig_coordinates': jig, tag + 'jig_weight': np.asarray(jw), tag + 'jig_f_V_int': jf,
                 tag + 'jig_f_V': _dense(m.get_vector_volume(elem, jig, jf, hatp, jw))})
    tv = rng.normal(0, 100, size=(2, n_int_s))
    arrs.update({tag + 'ft_int_var': tv,
                 tag + 'f_t_var': _dense(m.get_vector_traction(mesh['neumann_nodes'], coord, tv, hatp_s, d1_s, wf_s))})


def gen_el_loads(R):
    m = R['el']
    arrs = {}
    for t in ('P1', 'P2', 'Q1', 'Q2'):
        et = m.LagrangeElementType[t]
        xi_s, wf_s = m.get_quadrature_surface(et)
        hatp_s, d1_s = m.get_local_basis_surface(et, xi_s)
        arrs.update({f'{t}_xi_s': xi_s, f'{t}_wf_s': wf_s, f'{t}_hatp_s': hatp_s, f'{t}_dhatp1_s': d1_s})
    for t, level in (('P1', 1), ('Q1', 1), ('Q2', 1), ('P1', 3)):
        _el_case(m, t, level, arrs)

    # P2: EL functions on the DP square
    z = np.load(os.path.join(OUT, 'mesh_dp.npz'))
    et = m.LagrangeElementType.P2
    coord, elem0 = z['P2_n4_coordinates'], z['P2_n4_elements'].astype(np.int64)
    xi, wf = m.get_quadrature_volume(et)
    hatp, d1, d2 = m.get_local_basis_volume(et, xi)
    n_int = elem0.shape[1] * wf.size
    rng = np.random.default_rng(31)
    _, w = m.get_elastic_stiffness_matrix(elem0 + 1, coord, np.ones(n_int), np.ones(n_int), d1, d2, wf)
    fc = np.dot(VOLUME_FORCE.transpose(), np.ones((1, n_int)))
    fr = rng.normal(0, 1, size=(2, n_int))
    top = np.flatnonzero(coord[1] == 4)
    top = top[np.argsort(coord[0, top])]
    edges = np.array([top[0:-2:2], top[2::2], top[1::2]], dtype=float)
    xi_s, wf_s = m.get_quadrature_surface(et)
    hatp_s, d1_s = m.get_local_basis_surface(et, xi_s)
    n_int_s = edges.shape[1] * len(wf_s)
    tc = np.dot(TRACTION_FORCE.transpose(), np.ones((1, n_int_s)))
    tv = rng.normal(0, 100, size=(2, n_int_s))
    arrs.update({'P2sq_weight': np.asarray(w), 'P2sq_f_V_const': _dense(m.get_vector_volume(elem0, coord, fc, hatp, w)),
                 'P2sq_f_V_int': fr, 'P2sq_f_V_rand': _dense(m.get_vector_volume(elem0, coord, fr, hatp, w)),
                 'P2sq_edges': edges, 'P2sq_f_t_const': _dense(m.get_vector_traction(edges, coord, tc, hatp_s, d1_s, wf_s)),
                 'P2sq_ft_int_var': tv, 'P2sq_f_t_var': _dense(m.get_vector_traction(edges, coord, tv, hatp_s, d1_s, wf_s))})

    # P4: the TSX twin on the tunnel mesh
    x = R['tsx']
    z = np.load(os.path.join(OUT, 'tsx.npz'))
    et = x.LagrangeElementType.P4
    coord, elem0 = z['p4_coord'], z['p4_elem'].astype(np.int64)
    xi, wf = x.get_quadrature_volume(et)
    hatp, d1, d2 = x.get_local_basis_volume(et, xi)
    n_int = elem0.shape[1] * wf.size
    w = x.get_elastic_stiffness_matrix(elem0.copy(), coord, np.ones(n_int), np.ones(n_int), d1, d2, wf)[2]
    fc = np.dot(VOLUME_FORCE.transpose(), np.ones((1, n_int)))
    fr = rng.normal(0, 1, size=(2, n_int))
    arrs.update({'P4tx_weight': np.asarray(w), 'P4tx_f_V_const': _dense(x.get_vector_volume(elem0, coord, fc, hatp, w)),
                 'P4tx_f_V_int': fr, 'P4tx_f_V_rand': _dense(x.get_vector_volume(elem0, coord, fr, hatp, w))})
    save('el_loads', **arrs)


if __name__ == '__main__':
    gen_el_loads(_load_reference())

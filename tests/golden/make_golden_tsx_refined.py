#!/usr/bin/env python3
"""
Golden fixture of the TSX driver on the tunnel mesh refined once: `tsx_refined1_trace.npz`, recorded from the
reference's own functions (imported read-only, as make_golden.py does; arrays and scalars only, no reference text).

    python tests/golden/make_golden_tsx_refined.py

The reference has no refinement.  The level-1 mesh is made here from the reference's create_midpoints_P2 on the mesh
of tsx.npz: new vertices = its midside nodes, and with its rows (V1, V2, V3, m23, m31, m12) the children 4i .. 4i + 3 of
element i are (V1, m12, m31), (m12, V2, m23), (m31, m23, V3), (m12, m23, m31) — the definition refine_uniform follows.
On that P1 mesh (3 548 triangles, 1 839 nodes, 3 678 DOFs) the load-step sequence TSX:1729-1832 is replayed exactly as
make_golden.gen_tsx replays it on the level-0 mesh: the reference's get_elastic_stiffness_matrix and
construct_constitutive_problem, dense solves on the free DOFs.

Keys: coord (2, 1839), elem (3, 3548) int64, zeta, nplast, n_calls, U_mon (U[0, 40] per accepted step), U_final, F0.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load_reference, _tsx_replay, _tsx_setup, save      # noqa: E402


def main():
    m = _load_reference()['tsx']
    g = np.load(os.path.join(OUT, 'tsx.npz'))
    p2 = m.create_midpoints_P2(g['coord'], g['elem'])
    V1, V2, V3, m23, m31, m12 = p2['elem_ext']
    elem = np.stack([np.stack([V1, m12, m31]), np.stack([m12, V2, m23]), np.stack([m31, m23, V3]),
                     np.stack([m12, m23, m31])], axis=2).reshape(3, -1).astype(np.int64)
    coord = p2['coord_ext']
    t0 = time.time()
    K, B, w, iD, jD, D, Q, n_int = _tsx_setup(m, 'P1', coord, elem)
    hist, nplast, Us, F0, calls = _tsx_replay(m, K, B, w, iD, jD, D, Q, n_int, coord, progress=print)
    print(f'  tsx P1 level-1 replay: {time.time() - t0:.0f}s steps {len(hist)} calls {calls} n_plast {nplast.tolist()} '
          f'U[0,40] {Us[-1][0, 40]!r}')
    save('tsx_refined1_trace', coord=coord, elem=elem, zeta=hist, nplast=nplast, n_calls=np.array(calls),
         U_mon=Us[:, 0, 40], U_final=Us[-1], F0=F0)


if __name__ == '__main__':
    main()

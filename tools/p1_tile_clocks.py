#!/usr/bin/env python3
"""Phase stamps of the two P1 tile kernels (p1_node_lds_kernel, p1_fused_kernel) on square(n) P1, n = 708 by default: full-output
and K,F-only steps in turn; the measurement build prints the per-workgroup means of the last launch of each kernel when the
context is closed (fep_api.hip, fep_ctx_destroy).  Needs the -DFEP_ABLATION library:
    python fem-elastoplasticity_amd/build.py --ablation
    FEP_LIB_PATH=$PWD/fem-elastoplasticity_amd/csrc/libfep_hip_abl.so FEP_P1_CLK=1 python tools/p1_tile_clocks.py [n]
Recorded in profiles/r05_tile_record_stamps.txt."""
import importlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fep = importlib.import_module('fem-elastoplasticity_amd')
n = int(sys.argv[1]) if len(sys.argv) > 1 else 708
m = fep.square_mesh(n, 'P1', 10)
elem, coord = m['elements'], m['coordinates']
ctx = fep.MeshContext(elem, coord)
n_int = ctx.n_int
young, nu, c0, phi = 1e7, 0.48, 450, np.pi / 9
sh = young / (2 * (1 + nu)) * np.ones(n_int); bu = young / (3 * (1 - 2 * nu)) * np.ones(n_int)
eta = 3 * np.tan(phi) / np.sqrt(9 + 12 * np.tan(phi) ** 2) * np.ones(n_int); c = 3 * c0 / np.sqrt(9 + 12 * np.tan(phi) ** 2) * np.ones(n_int)
ctx.set_materials(sh, bu, eta, c)
x, y = coord
rng = np.random.default_rng(0)
U = np.array([2.5e-4 * y * (x / 10) + 1.2e-4 * x * (y > 5), -1.5e-4 * y * (x < 5) + 2.0e-4 * y * (x >= 5)])
Ep = rng.normal(0, 1e-5, size=(4, n_int))
for rep in range(3):
    full = ctx.step(U, Ep.copy(), want=('E', 's', 'ds', 'ind_p', 'K', 'F'))
    kf = ctx.step(U, Ep.copy(), want=('K', 'F'))
assert np.array_equal(kf['K'].data, full['K'].data) and np.array_equal(kf['F'], full['F'])
print('n_e', elem.shape[1], 'counts', full['n_smooth'], full['n_apex'], flush=True)
ctx.close()

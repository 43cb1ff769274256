#!/usr/bin/env python3
"""Step times of the material models side by side, per element type: the fused Drucker-Prager step against the von
Mises (plane strain, and plane stress with its per-point Newton loop) and the Mohr-Coulomb step (point kernel + the route's assembly from ds / s), each as the K,F-only step of a Newton iterate
and with every point output.  A fourth row, "DP, field" (keys dp_field_*) beside "DP, uniform" (dp_*): the same Drucker-Prager context
stepped with an initial strain per point (a field of zeros, so the same points yield), which runs staged like the von Mises and
Mohr-Coulomb rows it is to be compared with.  'vmi' (von Mises with isotropic hardening on an eight-segment Voce curve, the materials
of 'vm') runs beside 'vm', and 'vm' is timed a second time in every pass ('vm_repeat'): the spread between the two is what a
difference between 'vmi' and 'vm' has to exceed to mean anything.  HIP events around batches of steps, the ten variants of a type interleaved pass
by pass in one process (what differs between them is then not the box or the session).  Prints one JSON line.
    python tools/model_bench.py [--types P1,P2,Q1,Q2,P4] [--steps 20] [--passes 5] [--scale 1.0]
Mesh sizes as tools/elem_bench.py is run (cells per side: 708, P4 354); --scale shrinks them for a quick look."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import torch  # noqa: E402

fep = importlib.import_module('fem-elastoplasticity_amd')
MODELS = ('dp', 'vm', 'mc', 'vmps', 'vmi')
CELLS = {'P1': 708, 'P2': 708, 'Q1': 708, 'Q2': 708, 'P4': 354}


def mesh_of(t, N):
    if t == 'P4':
        m1 = fep.square_mesh(N, 'P1', 10)
        mp = fep.create_midpoints_P4(m1['coordinates'], m1['elements'])
        return np.asarray(mp['elem_ext'], dtype=np.int64), mp['coord_ext']
    m = fep.square_mesh(N, t, 10)
    return m['elements'], m['coordinates']


def time_type(t, N, steps, passes):
    elem, coord = mesh_of(t, N)
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    sh, bu, eta, c = bench.dp_materials()
    Uh = bench.displacement(coord)
    U = torch.from_numpy(np.ascontiguousarray(Uh.reshape(-1, order='F'))).to(dev)
    ctxs = {}
    # the same shear and bulk; the von Mises radius sqrt(2) c is the Drucker-Prager cone's at zero pressure, the Mohr-Coulomb
    # friction angle and cohesion are those the cone was matched to (bench.dp_materials)
    third_fourth = {'dp': (eta, c), 'vm': (0.05 * sh, np.sqrt(2) * c), 'mc': (np.sin(np.pi / 9), 450.0),
                    'vmps': (0.05 * sh, np.sqrt(2) * c), 'vmi': (0.05 * sh, np.sqrt(2) * c)}
    sigma_0 = float(np.sqrt(1.5) * np.sqrt(2) * np.min(c))               # the yield stress of the radius sqrt(2) c
    for model in MODELS:
        ctx = fep.MeshContext(elem, coord)
        ctx.set_model(model)
        ctx.set_materials(sh, bu, *third_fourth[model])
        if model == 'vmi':
            ctx.set_hardening(*fep.voce_curve(sigma_0, 1.5 * sigma_0, 60.0)[1:])
        ctxs[model] = ctx
    n = ctxs['dp'].n_int
    f64 = dict(dtype=torch.float64, device=dev)
    Ep = torch.zeros((4, n), **f64); S = torch.empty((4, n), **f64); DS = torch.empty((9, n), **f64)
    ind = torch.empty(n, dtype=torch.uint8, device=dev)
    Kd = torch.empty(ctxs['dp'].nnz, **f64); F = torch.empty(ctxs['dp'].n_dof, **f64)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    Fld = torch.zeros((4, n), **f64)

    def step(model, full):
        kw = dict(s=S.data_ptr(), ds=DS.data_ptr(), ind_p=ind.data_ptr()) if full else {}
        if model == 'dp_field':
            model, kw = 'dp', dict(kw, e0_field=Fld.data_ptr(), e0_scale=1.0)
        if model == 'vm_repeat':
            model = 'vm'
        ctxs[model].step_dev(st, U.data_ptr(), ep=Ep.data_ptr(), k_data=Kd.data_ptr(), f_out=F.data_ptr(),
                             counts=cnt.data_ptr(), **kw)
    variants = [(m, full) for m in MODELS + ('dp_field', 'vm_repeat') for full in (False, True)]
    plastic = {}
    for m, full in variants:
        for _ in range(3):
            step(m, full)
        torch.cuda.synchronize()
        plastic[m] = int(cnt.cpu().sum()) / n
    best = {v: float('inf') for v in variants}
    for _ in range(passes):
        for v in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step(*v)
            b.record()
            b.synchronize()
            best[v] = min(best[v], a.elapsed_time(b) / steps)
    out = {'cells': N, 'n_e': ctxs['dp'].n_e, 'n_int': n, 'plastic_share': {m: round(p, 3) for m, p in plastic.items()},
           'kernels': {m: ctxs[m].kernel_names(0) for m in ctxs}}
    for (m, full), ms in best.items():
        out[f'{m}_{"full" if full else "kf"}_ms'] = round(ms, 4)
    for ctx in ctxs.values():
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--types', default='P1,P2,Q1,Q2,P4')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--scale', type=float, default=1.0)
    a = ap.parse_args()
    res = {'tool': 'model_bench', 'steps': a.steps, 'passes': a.passes, 'device': torch.cuda.get_device_name(0), 'types': {}}
    for t in a.types.split(','):
        res['types'][t] = time_type(t, max(4, int(round(CELLS[t] * a.scale))), a.steps, a.passes)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""
Times the volume-load kernel (MeshContext.load_volume_dev, field and uniform forms) and, as its yardstick, the sibling
that walks the same node -> (element, local node) lists, nodal_average_kernel (MeshContext.transform_dev), on the bench
mesh (1 002 528 P1 elements) and on ~1 M-point P2 / Q2 meshes.

HIP events around one replay of a graph that holds `--reps` launches of a kernel (no host launch path inside the timed
window), `--passes` passes after a warm-up, the kernels alternating; the median pass is reported, with the fastest and
slowest.  Back-to-back launches keep a small working set in L2 from one launch to the next: a single cold call is slower.  Share of HBM bandwidth = algorithmic bytes / time / 8 TB/s, bytes counted from shapes:
    load, field    24 B per point (weight, f_x, f_y) + 16 B per node written + 4 B per incidence entry + 4 B (n_n + 1) iptr
    load, uniform   8 B per point (weight)           + the same
    transform      16 B per point (weight, q)        + 8 B per node written + the same lists
Each point is re-read once per node of its element through L2; the model counts it once.

    python tools/load_bench.py [--reps 200] [--passes 7] [--out FILE.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--cells', default='P1:708,P2:267,Q2:333', help='element type : cells per side')
    a = ap.parse_args()
    import torch
    fep = importlib.import_module('fem-elastoplasticity_amd')
    fep.build()
    if not torch.cuda.is_available():
        raise SystemExit('load_bench: no GPU')
    dev = torch.device('cuda', 0)
    rows = []
    for spec in a.cells.split(','):
        t, n = spec.split(':')
        mesh = fep.square_mesh(int(n), t, 10)
        ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'])
        n_inc = ctx.n_p * ctx.n_e
        rng = np.random.default_rng(5)
        f = torch.from_numpy(rng.normal(size=(2, ctx.n_int))).to(dev)
        q = torch.from_numpy(rng.normal(size=ctx.n_int)).to(dev)
        out = torch.empty(ctx.n_dof, dtype=torch.float64, device=dev)
        qn = torch.empty(ctx.n_n, dtype=torch.float64, device=dev)
        lists = 4 * n_inc + 4 * (ctx.n_n + 1)
        cases = {
            'load_field': (lambda st: ctx.load_volume_dev(st, out.data_ptr(), f_v_int=f.data_ptr()), 24 * ctx.n_int + 16 * ctx.n_n + lists),
            'load_uniform': (lambda st: ctx.load_volume_dev(st, out.data_ptr(), uniform=(0.0, -9.81)), 8 * ctx.n_int + 16 * ctx.n_n + lists),
            'transform': (lambda st: ctx.transform_dev(st, q.data_ptr(), qn.data_ptr()), 16 * ctx.n_int + 8 * ctx.n_n + lists),
        }
        res = {}
        # `reps` launches captured into one graph per kernel: a replay is free of the host's launch path (a ctypes call takes
        # as long as the P1 kernel runs), so the event pair brackets device time only
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            st_side = torch.cuda.current_stream().cuda_stream
            for fn, _b in cases.values():
                fn(st_side)
        torch.cuda.synchronize()
        graphs = {}
        for k, (fn, _b) in cases.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st_cap = torch.cuda.current_stream().cuda_stream
                for _ in range(a.reps):
                    fn(st_cap)
            graphs[k] = g
        for _ in range(a.warmup):
            for g in graphs.values():
                g.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(a.passes):                               # the three kernels alternate inside every pass
            for k, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e-3 / a.reps)
        for k, (_fn, nbytes) in cases.items():
            ts = sorted(times[k])
            med = ts[len(ts) // 2]
            res[k] = {'us': med * 1e6, 'us_min': ts[0] * 1e6, 'us_max': ts[-1] * 1e6, 'bytes': nbytes,
                      'share_of_8TBs': nbytes / med / PEAK}
        per_byte = {k: res[k]['us'] / res[k]['bytes'] for k in res}
        row = {'element_type': t, 'n_e': ctx.n_e, 'n_n': ctx.n_n, 'n_int': ctx.n_int, **res,
               'time_per_byte_vs_transform': {k: per_byte[k] / per_byte['transform'] for k in ('load_field', 'load_uniform')}}
        rows.append(row)
        print(json.dumps(row))
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump({'reps': a.reps, 'passes': a.passes, 'rows': rows}, fh, indent=1)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""
Times the mesh kernels (fep_mesh_*: P1 -> P2 / P4 enrichment, uniform refinement) against the host functions they
replace, in one process and one session, on the tunnel mesh of tests/golden/tsx.npz refined `refine` times (4: 227 072
triangles):

  a  host         create_midpoints_P2 / _P4, the Python loop (one run: it is the slow side)
  b  device_host  the device path, host arrays in -> the host functions' dict out (create_midpoints_*(device=...)):
                  upload, analysis, kernels, download, dtype conversions; best and median of `--passes` after a warm-up
  c  resident     device tensors in -> device tensors out, HIP events after a warm-up: fep_mesh_create (analysis: lists,
                  matching, prefix sums; it synchronises) and the enrichment kernel alone; `copy` = a plain device copy
                  of the enrichment's output bytes, timed the same way in the same run — the yardstick of the fill
  d  refine       refine_uniform host and device (levels chained on the GPU) for the same depth from the 887-triangle mesh

`--curved` runs the device passes a second time with the tunnel wall's ellipse set (tsx_tunnel.TSX_HOLE; key 'curved'), so that
both sit in one record, and writes profiles/mesh_bench_curved.json unless `--out` says otherwise; with `--solve R` it also
solves levels 0..R on the wall's polygon and on its ellipse and prints U[0, 40] of both.  Every run also times the refinement
kernel alone and fep_mesh_area_stats_dev on its children (HIP events).

`--marked` adds refine_marked (conforming longest-edge bisection of marked elements) on the same refined mesh with the
elements within 4 of the tunnel's centre marked: the NumPy form (one run), the device path host arrays in / out, and,
device-resident with HIP events, fep_mesh_mark (closure, scans; it synchronises) and the emit kernel alone; and the monitored
displacement U[0, 40] of the P1 tunnel run unrefined, with adapt=2 and with refine=2 (direct solver).  Key 'marked';
profiles/mesh_bench_marked.json unless `--out` says otherwise.

`--estimate` (meant for `--refine 5`: 908 288 triangles) runs nothing of the above: it times the error indicator — recovery,
indicator, statistics, bulk marking — resident on the device (HIP events) against its NumPy twin in the same process, checks
that they agree bit for bit, and records next to each time the bytes the pass has to move (s, the node gathers, 8 B per
element per tail pass) and the launches the marking took.  Key 'estimate'; profiles/estimate_bench.json unless `--out`.

`--solve R` adds the end-to-end TSX run solve_tsx_tunnel(refine=R, 'P1', linear_solver='amg', pcg_inexact_rtol=1e-2) with
its set-up split, without and with renumbering.  One JSON line (and `--out FILE`).

    python tools/mesh_bench.py [--refine 4] [--type P2] [--passes 5] [--solve 5] [--curved] [--marked] [--out profiles/mesh_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(f, passes):
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return {'best_ms': 1e3 * min(ts), 'median_ms': 1e3 * float(np.median(ts))}


def events(torch, f, passes):
    ts = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {'best_ms': min(ts), 'median_ms': float(np.median(ts))}


def measure(fep, torch, a, coord0, elem0, curves, host=True):
    """Passes a-d on the tunnel mesh refined a.refine times; `curves` (None or [TSX_HOLE]) go to every call.  host=False
    leaves out the host loops (a, and d's host side)."""
    dev = a.device
    kw = {} if curves is None else {'curves': curves}
    res = {}
    # d: refinement, host and device, same depth
    if host:
        t0 = time.perf_counter()
        coord, elem = fep.refine_uniform(coord0, elem0, levels=a.refine, **kw)
        res['refine_host_ms'] = 1e3 * (time.perf_counter() - t0)
    fep.refine_uniform(coord0, elem0, levels=a.refine, device=dev, **kw)              # warm-up
    res['refine_device'] = wall(lambda: fep.refine_uniform(coord0, elem0, levels=a.refine, device=dev, **kw), a.passes)
    cd, ed = fep.refine_uniform(coord0, elem0, levels=a.refine, device=dev, **kw)
    if host:
        res['refine_bit_equal'] = bool(np.array_equal(cd, coord) and np.array_equal(ed, elem))
    else:
        coord, elem = cd, ed
    res['n_e'], res['n_n'] = int(elem.shape[1]), int(coord.shape[1])

    tdev = torch.device('cuda', dev)
    coord_d = torch.from_numpy(coord).to(tdev)
    elem_d = torch.from_numpy(elem.astype(np.int32)).to(tdev)
    # the refinement kernel alone (one level from this mesh) and the area statistics of its children, HIP events
    with fep.DeviceMesh(coord_d, elem_d, dev, on_device=True) as m:
        m.set_curves(curves)
        c1, e1 = m.refine_dev()                                                       # warm-up
        torch.cuda.synchronize(dev)
        res['resident_refine'] = events(torch, m.refine_dev, a.passes)
        out = fep.area_stats_dev(c1, e1, dev)                                         # warm-up: makes the partials' block
        res['area_stats'] = events(torch, lambda: fep.area_stats_dev(c1, e1, dev, out=out), a.passes)
        res['area_stats_out'] = [float(v) for v in out.cpu().numpy()]
        del c1, e1
    for t in a.type.split(','):
        r = {}
        if host:
            t0 = time.perf_counter()
            h = fep.create_midpoints(t, coord, elem, **kw)
            r['host_ms'] = 1e3 * (time.perf_counter() - t0)                            # a
        d = fep.create_midpoints(t, coord, elem, device=dev, **kw)                    # warm-up
        if host:
            r['bit_equal'] = bool(all(np.array_equal(h[k], d[k]) and h[k].dtype == d[k].dtype for k in h))
        r['device_host'] = wall(lambda: fep.create_midpoints(t, coord, elem, device=dev, **kw), a.passes)   # b
        if host:
            r['speedup_device_host'] = r['host_ms'] / r['device_host']['median_ms']
        meshes = []

        def analyse():
            meshes.append(fep.DeviceMesh(coord_d, elem_d, dev, on_device=True))
            meshes[-1].set_curves(curves)
        analyse()
        m = meshes[0]
        out = m.enrich_dev(t)                                                          # warm-up
        torch.cuda.synchronize(dev)
        r['resident_create'] = events(torch, analyse, a.passes)                        # c
        r['resident_enrich'] = events(torch, lambda: m.enrich_dev(t), a.passes)
        r['output_bytes'] = int(sum(o.numel() * o.element_size() for o in out))
        copies = [torch.empty_like(o) for o in out]

        def copy():
            for dst, src in zip(copies, out):
                dst.copy_(src)
        copy()
        r['copy'] = events(torch, copy, a.passes)
        r['enrich_over_copy'] = r['resident_enrich']['median_ms'] / r['copy']['median_ms']
        for mm in meshes:
            mm.close()
        res[t] = r
    return res


def measure_marked(fep, torch, a, coord0, elem0):
    dev = a.device
    coord, elem = fep.refine_uniform(coord0, elem0, levels=a.refine, device=dev)
    cx, cy = coord[0][elem].mean(axis=0), coord[1][elem].mean(axis=0)
    marked = cx * cx + cy * cy < 16.0
    res = {'n_e': int(elem.shape[1]), 'n_marked': int(marked.sum())}
    t0 = time.perf_counter()
    h = fep.refine_marked(coord, elem, marked)
    res['host_ms'] = 1e3 * (time.perf_counter() - t0)
    d = fep.refine_marked(coord, elem, marked, device=dev)                            # warm-up
    res['bit_equal'] = bool(all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(h, d)))
    res['n_child'], res['n_new_nodes'] = int(d[1].shape[1]), int(d[0].shape[1] - coord.shape[1])
    res['device_host'] = wall(lambda: fep.refine_marked(coord, elem, marked, device=dev), a.passes)
    res['speedup_device_host'] = res['host_ms'] / res['device_host']['median_ms']
    tdev = torch.device('cuda', dev)
    coord_d, elem_d = torch.from_numpy(coord).to(tdev), torch.from_numpy(elem.astype(np.int32)).to(tdev)
    marked_d = torch.from_numpy(marked.view(np.uint8)).to(tdev)
    with fep.DeviceMesh(coord_d, elem_d, dev, on_device=True) as m:
        res['sweeps'] = m.mark(marked_d, on_device=True)['n_sweeps']                  # warm-up: makes the scratch
        m.refine_marked_dev()
        torch.cuda.synchronize(dev)
        res['resident_mark'] = events(torch, lambda: m.mark(marked_d, on_device=True), a.passes)
        res['resident_emit'] = events(torch, m.refine_marked_dev, a.passes)
    runs = {'unrefined': {}, 'adapt2': {'adapt': 2}, 'refine2': {'refine': 2}}
    res['displ'] = {}
    for name, kw in runs.items():
        r = fep.solve_tsx_tunnel(coord0, elem0, 'P1', device=dev, **kw)
        res['displ'][name] = {'U_0_40': float(r['displ'][-1]), 'n_e': int(r['elem'].shape[1]) if 'elem' in r else int(elem0.shape[1]),
                              'accepted_steps': len(r['zeta']), 'n_plast_last': int(r['n_plast'][-1])}
        if 'adapt' in r:
            res['displ'][name]['rounds'] = [{k: row[k] for k in ('n_e', 'n_n', 'n_marked', 'n_child', 'displ', 'n_steps', 'n_plast')}
                                            for row in r['adapt']]
    return res


def measure_estimate(fep, torch, a, coord0, elem0):
    """Recovery, indicator and bulk marking (include/fep.h, "recovered-stress error indicator") on the P1 tunnel mesh refined
    a.refine times, with the stress of one elastic step of a smooth displacement: resident on the device (HIP events)
    against the NumPy twin in the same process, the bytes every pass has to move and the launches of the marking."""
    from contextlib import closing
    est = importlib.import_module('fem-elastoplasticity_amd.estimate')
    dev = a.device
    coord, elem = fep.refine_uniform(coord0, elem0, levels=a.refine, device=dev)
    n_e, n_n = int(elem.shape[1]), int(coord.shape[1])
    shear, bulk = 60000 / (2 * 1.2), 60000 / (3 * 0.6)
    res = {'n_e': n_e, 'n_n': n_n, 'theta': 0.5}
    tdev = torch.device('cuda', dev)
    with closing(fep.MeshContext(elem, coord, *fep.element_tables('P1'), device=dev)) as ctx:
        ctx.set_materials(shear, bulk, 0.5, 1e9)
        w = np.asarray(ctx.geometry()[2], dtype=float).ravel()
        u = 1e-3 * np.stack([np.sin(coord[0] / 7) * np.cos(coord[1] / 9), np.cos(coord[0] / 5) * np.sin(coord[1] / 11)])
        u_d = torch.from_numpy(np.ascontiguousarray(u.T).ravel()).to(tdev)
        s_d = torch.empty((4, n_e), dtype=torch.float64, device=tdev)
        ind_d = torch.empty(n_e, dtype=torch.uint8, device=tdev)
        ctx.step_dev(torch.cuda.current_stream(dev).cuda_stream, u_d.data_ptr(), s=s_d.data_ptr(), ind_p=ind_d.data_ptr())
        sn_d = ctx.recover_stress_dev(s_d)                                            # warm-ups: make the scratch
        eta2_d, st_d, _ = ctx.estimate_dev(s_d, s_node=sn_d)
        marked_d, out_d = fep.mark_bulk(eta2_d, 0.5)
        torch.cuda.synchronize(dev)
        res['resident_recover'] = events(torch, lambda: ctx.recover_stress_dev(s_d, out=sn_d), a.passes)
        res['resident_indicator'] = events(torch, lambda: ctx.estimate_dev(s_d, s_node=sn_d, stats=False), a.passes)
        res['resident_indicator_stats'] = events(torch, lambda: ctx.estimate_dev(s_d, s_node=sn_d), a.passes)
        res['resident_mark_bulk'] = events(torch, lambda: fep.mark_bulk(eta2_d, 0.5), a.passes)
        s = s_d.cpu().numpy()
    t0 = time.perf_counter()
    sn = est.recover_stress_np(elem, w, s, n_n)
    t1 = time.perf_counter()
    twin = est.estimate_np(elem, w, shear, bulk, None, s, n_n)
    t2 = time.perf_counter()
    marked, out = est.mark_bulk(twin['eta2'], 0.5)
    t3 = time.perf_counter()
    res['twin_ms'] = {'recover': 1e3 * (t1 - t0), 'indicator': 1e3 * ((t2 - t1) - (t1 - t0)), 'mark_bulk': 1e3 * (t3 - t2)}
    res['bit_equal'] = {'s_node': sn_d.cpu().numpy().tobytes() == sn.tobytes(), 'eta2': eta2_d.cpu().numpy().tobytes() == twin['eta2'].tobytes(),
                        'stats': st_d.cpu().numpy().tolist() == [twin['total'], twin['max'], float(twin['n_nonfinite']), float(n_e)],
                        'marked': marked_d.cpu().numpy().tobytes() == marked.view(np.uint8).tobytes(),
                        'out': out_d.cpu().numpy().tobytes() == out.tobytes()}
    res['eta'], res['n_marked'], res['t_star'] = float(np.sqrt(twin['total'])), int(marked.sum()), float(out[0])
    passes = est.VALUE_BITS + 2
    res['launches'] = {'mark_bulk': est.mark_bulk_launches(n_e), 'tree_levels': est.tree_levels(n_e), 'passes': passes,
                       'recover': 1, 'indicator': 1, 'stats': est.tree_levels(n_e)}
    # what each pass has to move at the least (every array once) and what its lanes ask for (the gathers, served by the caches)
    res['bytes'] = {'recover': {'once': 40 * n_e + 32 * n_n + 4 * (3 * n_e + n_n + 1), 'gathers': 3 * n_e * 40},
                    'indicator': {'once': (32 + 8 + 12 + 8) * n_e + 32 * n_n, 'gathers': 3 * n_e * 32},
                    'mark_bulk': {'per_tail_pass': 8 * n_e, 'all_passes': passes * 8 * n_e + n_e}}
    for k, b in (('resident_recover', res['bytes']['recover']['once']), ('resident_indicator', res['bytes']['indicator']['once']),
                 ('resident_mark_bulk', res['bytes']['mark_bulk']['all_passes'])):
        res[k]['GB_per_s_of_least_bytes'] = b / (1e6 * res[k]['median_ms'])
    # the tunnel driven by the indicator: two rounds from the 887-triangle mesh, next to the default marking (mark_plastic)
    res['tunnel'] = {}
    for name, kw in (('zz', {'mark': 'zz', 'theta': 0.5}), ('plastic', {})):
        r = fep.solve_tsx_tunnel(coord0, elem0, 'P1', device=dev, adapt=2, **kw)
        res['tunnel'][name] = [{k: (row[k] if row[k] is None else float(row[k]) if k in ('displ', 'eta') else int(row[k]))
                                for k in ('n_e', 'n_marked', 'displ', 'n_plast', 'eta') if k in row} for row in r['adapt']]
    return res


def solve(fep, a, mesh_dir, refine, renumber, curves):
    t0 = time.perf_counter()
    h = fep.solve_tsx_tunnel(mesh_dir=mesh_dir, element_type='P1', refine=refine, renumber=renumber, linear_solver='amg',
                             pcg_inexact_rtol=1e-2, device=a.device, curves=curves,
                             log=lambda s: print(s, file=sys.stderr, flush=True))
    return {'wall_s': time.perf_counter() - t0, 'n_e': int(h['elem'].shape[1]) if 'elem' in h else None, 'n_n': int(h['U'][-1].shape[1]),
            'accepted_steps': len(h['zeta']), 'zeta_last': float(h['zeta'][-1]), 'displ_last': float(h['displ'][-1]),
            'n_plast_last': int(h['n_plast'][-1]), 'n_calls': int(h['n_calls']),
            'pcg_iters': int(np.sum(h['pcg_iters'])) if h['pcg_iters'] is not None else None,
            'setup_s': {k: float(v) for k, v in h['t_setup'].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--refine', type=int, default=4)
    ap.add_argument('--type', default='P2,P4')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--solve', type=int, default=None)
    ap.add_argument('--curved', action='store_true')
    ap.add_argument('--marked', action='store_true')
    ap.add_argument('--estimate', action='store_true')
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    fep = importlib.import_module('fem-elastoplasticity_amd')
    fep.build()
    dev = a.device
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'tsx.npz'))
    coord0, elem0 = g['coord'], g['elem']
    hole = [fep.tsx_tunnel.TSX_HOLE]
    res = {'tool': 'mesh_bench', 'refine': a.refine, 'device_name': torch.cuda.get_device_name(dev)}
    if a.estimate:                                                                    # a record of its own: none of the passes a-d
        res['estimate'] = measure_estimate(fep, torch, a, coord0, elem0)
        line = json.dumps(res)
        print(line)
        with open(a.out or os.path.join(ROOT, 'profiles', 'estimate_bench.json'), 'w') as fh:
            fh.write(line + '\n')
        return
    res.update(measure(fep, torch, a, coord0, elem0, None))
    if a.curved:
        res['curved'] = measure(fep, torch, a, coord0, elem0, hole, host=False)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'mesh_bench_curved.json')

    if a.marked:
        res['marked'] = measure_marked(fep, torch, a, coord0, elem0)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'mesh_bench_marked.json')

    if a.solve is not None:
        d = tempfile.mkdtemp(prefix='tsx_csv_')
        np.savetxt(os.path.join(d, 'coord.csv'), coord0, delimiter=',', fmt='%.17g')
        np.savetxt(os.path.join(d, 'elem.csv'), elem0 + 1, delimiter=',', fmt='%d')
        res['solve'] = {'refine': a.solve}
        for renumber in (False, True):
            res['solve']['renumber' if renumber else 'as_refined'] = solve(fep, a, d, a.solve, renumber, None)
        if a.curved:
            # U[0, 40] (the tunnel's crown) per level, on the wall's polygon and on its ellipse
            res['solve']['levels'] = []
            for lv in range(a.solve + 1):
                row = {'refine': lv, 'polygon': solve(fep, a, d, lv, False, None), 'ellipse': solve(fep, a, d, lv, False, hole)}
                res['solve']['levels'].append(row)
                print('refine %d: U[0, 40] polygon %.10e, ellipse %.10e' % (lv, row['polygon']['displ_last'],
                                                                           row['ellipse']['displ_last']), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The launch sequence of every step form, taken from the launches themselves.

Walks a fixed matrix of step_dev / assemble_dev calls on two tiny meshes -- P1 square_mesh(20) and Q1 square_mesh(4); the
default route, FEP_ROUTE=patch and FEP_ROUTE=coo; the five material models; with and without an initial-strain field;
accepting or not; every output, K+F, K, F, the point outputs, each with and without the branch counters; assemble_dev
with K+F, K, F -- through the public Python API only, so that it runs unchanged on any commit, and prints one label
line per case.  Every case lies between two launches of nodal_average_kernel (transform_dev), which no step launches.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/step_trace.py --labels DIR/labels.txt
    python3 tools/step_trace.py --reduce DIR [--grids] > launches.json

--reduce cuts the kernel trace under DIR at the delimiters and prints {case label: [kernel names]} as JSON (--grids:
[[name, workgroups], ...], for comparing two builds); tests/golden/step_launches.json is the names of such a run.
"""
import argparse
import csv
import glob
import importlib
import json
import os
import sys

MESHES = (('P1', 20), ('Q1', 4))
ROUTES = ('default', 'patch', 'coo')
MODELS = ('dp', 'vm', 'mc', 'vmps', 'vmi')
WANTS = {'all': ('e', 's', 'ds', 'ind_p', 'K', 'F'), 'KF': ('K', 'F'), 'K': ('K',), 'F': ('F',),
         'points': ('e', 's', 'ds', 'ind_p')}
ASSEMBLE = {'KF': ('K', 'F'), 'K': ('K',), 'F': ('F',)}
DELIMITER = 'nodal_average_kernel'


def labels():
    """The matrix in the order it is walked"""
    for t, n in MESHES:
        for route in ROUTES:
            for model in MODELS:
                head = f'{t}-{n}/{route}/{model}'
                for field in (0, 1):
                    for accept in (0, 1):
                        for w in WANTS:
                            for counts in (0, 1):
                                yield head, f'{head}/field{field}/accept{accept}/step:{w}/counts{counts}', (field, accept, WANTS[w], counts)
                for w in ASSEMBLE:
                    yield head, f'{head}/assemble:{w}', (None, None, ASSEMBLE[w], 0)


def walk(labels_path):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    fep = importlib.import_module('fem-elastoplasticity_amd')
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    out = open(labels_path, 'w') if labels_path else None
    ctx, ctx_head, buf = None, None, None
    for head, label, (field, accept, want, counts) in labels():
        if head != ctx_head:
            if ctx is not None:
                torch.cuda.synchronize()
                ctx.close()
            t, n = head.split('/')[0].split('-')
            route, model = head.split('/')[1:3]
            if route == 'default':
                os.environ.pop('FEP_ROUTE', None)
            else:
                os.environ['FEP_ROUTE'] = route           # read at context creation
            mesh = fep.square_mesh(int(n), t, 10)
            ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'])
            ctx.set_model(model)
            ones = np.ones(ctx.n_int)
            ctx.set_materials(1e4 * ones, 2e4 * ones, 0.3 * ones, 50.0 * ones)
            f64 = dict(dtype=torch.float64, device=dev)
            ni = ctx.n_int
            buf = {'u': torch.zeros(ctx.n_dof, **f64), 'ep': torch.zeros((4, ni), **f64), 'field': torch.zeros((4, ni), **f64),
                   'e': torch.zeros((3, ni), **f64), 's': torch.zeros((4, ni), **f64), 'ds': torch.zeros((9, ni), **f64),
                   'ind_p': torch.zeros(ni, dtype=torch.uint8, device=dev), 'K': torch.zeros(ctx.nnz, **f64),
                   'F': torch.zeros(ctx.n_dof, **f64), 'counts': torch.zeros(2, dtype=torch.int64, device=dev),
                   'q': torch.zeros(ni, **f64), 'qn': torch.zeros(ctx.n_n, **f64)}
            ctx_head = head
        p = {k: v.data_ptr() for k, v in buf.items()}
        print('case', label, flush=True)
        if out:
            out.write(label + '\n')
        ctx.transform_dev(st, p['q'], p['qn'])
        if field is None:
            ctx.assemble_dev(st, ds=p['ds'] if 'K' in want else 0, s=p['s'] if 'F' in want else 0,
                             k_data=p['K'] if 'K' in want else 0, f_out=p['F'] if 'F' in want else 0)
        else:
            w = {k: (p[k] if k in want else 0) for k in ('e', 's', 'ds', 'ind_p', 'K', 'F')}
            ctx.step_dev(st, p['u'], ep=p['ep'], accept=bool(accept), e_out=w['e'], s=w['s'], ds=w['ds'], ind_p=w['ind_p'],
                         k_data=w['K'], f_out=w['F'], counts=p['counts'] if counts else 0,
                         e0_field=p['field'] if field else None, e0_scale=1.0)
        ctx.transform_dev(st, p['q'], p['qn'])
        torch.cuda.synchronize()
    if ctx is not None:
        ctx.close()
    if out:
        out.close()


def kernel_name(signature):
    """'void fep::p1_node_lds_kernel<256, true, 1, true>(long, ...)' -> 'p1_node_lds_kernel<256, true, 1, true>': the name as
    rocprofv3 --stats and fep_ctx_kernel_names print it (no return type, namespace or parameter list)"""
    name = signature[:-3] if signature.endswith('.kd') else signature
    name = name[5:] if name.startswith('void ') else name
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == '<') - (ch == '>')
        if ch == '(' and depth == 0:
            name = name[:i]
            break
    return name.replace('fep::', '')


def reduce_trace(directory, grids):
    with open(os.path.join(directory, 'labels.txt')) as f:
        names = [ln.strip() for ln in f if ln.strip()]
    traces = sorted(glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True))
    if len(traces) != 1:
        raise SystemExit(f'expected one *kernel_trace.csv under {directory}, found {traces}')
    with open(traces[0], newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r['Start_Timestamp']), int(r.get('Dispatch_Id', 0))))
    segments, inside = [], False
    for r in rows:
        name = kernel_name(r['Kernel_Name'])
        if name.startswith(DELIMITER):
            inside = not inside
            if inside:
                segments.append([])
        elif inside:
            wg = [max(1, int(r[f'Grid_Size_{a}']) // max(1, int(r[f'Workgroup_Size_{a}']))) for a in 'XYZ']
            segments[-1].append([name, wg[0] * wg[1] * wg[2]] if grids else name)
    if inside or len(segments) != len(names):
        raise SystemExit(f'{len(names)} labels but {len(segments)} delimited segments (open: {inside})')
    json.dump(dict(zip(names, segments)), sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write('\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--labels', help='also write the label lines to this file (read by --reduce)')
    ap.add_argument('--reduce', metavar='DIR', help='reduce the kernel trace under DIR instead of walking the matrix')
    ap.add_argument('--grids', action='store_true', help='--reduce: keep the number of workgroups of every launch')
    a = ap.parse_args()
    if a.reduce:
        reduce_trace(a.reduce, a.grids)
    else:
        walk(a.labels)

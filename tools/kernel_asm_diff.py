#!/usr/bin/env python3
"""Which kernels does a source change alter?  `python tools/kernel_asm_diff.py TREE_A TREE_B [--ablation] [--only UNIT]`.

Compiles the four .hip translation units of both trees (repository roots) with build.py's flags plus
--cuda-device-only -S, splits the device assembly at the kernel symbols, drops comment and metadata lines and prints the
demangled name of every kernel whose text differs or that exists on one side only.  Exit code 1 if there is any, else 0.
Compares text only; cross-compiles, no GPU needed.  --ablation compares the measurement build (-DFEP_ABLATION)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fem-elastoplasticity_amd'))
import build as fep_build  # noqa: E402

PKG = 'fem-elastoplasticity_amd'


def device_asm(tree, unit, defs, out):
    csrc = os.path.join(os.path.abspath(tree), PKG, 'csrc')
    cmd = [fep_build.hipcc_path(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC'] + defs + \
          ['--cuda-device-only', '-S', '-o', out, unit]
    res = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError(f'{tree}: hipcc failed on {unit}:\n{res.stdout}')
    with open(out) as f:
        return f.read()


def kernels(asm):
    """{symbol: text} of every kernel (.amdhsa_kernel names it; its text runs from `symbol:` to its .Lfunc_end)."""
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, flags=re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r'^([A-Za-z_.$][\w.$]*):', s)
        if m and m.group(1) in names:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if s.startswith('.Lfunc_end'):
            cur = None
            continue
        s = re.sub(r'\s*;.*$', '', s)                   # comments (they carry source positions and symbol offsets)
        s = re.sub(r'\.L([A-Za-z]+)\d+_(\d+)', r'.L\1_\2', s)     # local labels carry the function's number in its unit (.LBB78_2):
                                                        # the order in which the host code instantiates the kernels, not code
        if s:
            out[cur].append(s)
    return {k: '\n'.join(v) for k, v in out.items()}


def demangle(sym):
    return subprocess.run(['c++filt', sym], stdout=subprocess.PIPE, text=True).stdout.strip() or sym


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('tree_a')
    ap.add_argument('tree_b')
    ap.add_argument('--ablation', action='store_true')
    ap.add_argument('--only', default='', help='one translation unit, e.g. fep_api.hip')
    a = ap.parse_args()
    defs = ['-DFEP_ABLATION'] if a.ablation else []
    units = [u for u in fep_build.SOURCES if not a.only or u == a.only]
    differing = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as pool:
        jobs = {(u, i): pool.submit(device_asm, t, u, defs, os.path.join(tmp, f'{i}_{u}.s'))
                for u in units for i, t in enumerate((a.tree_a, a.tree_b))}
        for u in units:
            ka, kb = kernels(jobs[(u, 0)].result()), kernels(jobs[(u, 1)].result())
            for sym in sorted(set(ka) | set(kb)):
                if sym not in ka or sym not in kb:
                    print(f'{u}: only in {a.tree_b if sym in kb else a.tree_a}: {demangle(sym)}')
                elif ka[sym] != kb[sym]:
                    print(f'{u}: differs: {demangle(sym)}')
                else:
                    continue
                differing += 1
            print(f'{u}: {len(ka)} / {len(kb)} kernels compared', file=sys.stderr)
    print(f'{differing} kernel(s) differ')
    return 1 if differing else 0


if __name__ == '__main__':
    sys.exit(main())

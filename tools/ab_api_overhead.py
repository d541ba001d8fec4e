#!/usr/bin/env python3
"""Host cost of uniformQuantization in the training loops' configuration (small tensor, eager): this tree's per-call binding
against ANOTHER build of it -- the parent commit's _qd_glue.so, say -- both loaded in one process and timed interleaved.

    python tools/ab_api_overhead.py OTHER_GLUE_SO [repetitions, default 9] > profiles/<name>.txt

The timing functions (host_only: sync every 64 calls, sync time excluded; wall: best of five full-queue loops) are those of
docs/history/tools/profile_api_overhead.py, the probe behind DESIGN.md section 1's 4.5 us, taken from its source.  The other
build must be compiled for the same include/qd_hip.h; copy it next to libqd_hip.so (its rpath is $ORIGIN)."""
import ast
import importlib.machinery
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import quantization  # noqa: E402
from quantization import quant_functions as qf  # noqa: E402
from quantized_distillation_amd import _lib  # noqa: E402


def probe_functions():
    src = open(os.path.join(ROOT, 'docs', 'history', 'tools', 'profile_api_overhead.py')).read()
    ns = {'time': time, 'torch': torch}
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name in ('wall', 'host_only'):
            exec(compile(ast.Module([node], []), 'profile_api_overhead.py', 'exec'), ns)
    return ns['wall'], ns['host_only']


def load_other(path):
    """A second _qd_glue module from `path` (the module's init function is found by the last component of the name)."""
    name = 'qd_other._qd_glue'
    loader = importlib.machinery.ExtensionFileLoader(name, path)
    mod = importlib.util.module_from_spec(importlib.util.spec_from_loader(name, loader, origin=path))
    loader.exec_module(mod)
    assert mod.abi_version() == _lib.ABI_VERSION, 'the other binding was compiled for another ABI version'
    return mod


def main():
    other_path = os.path.abspath(sys.argv[1])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    wall, host_only = probe_functions()
    here = _lib.glue()
    other = load_other(other_path)
    for g in (here, other):
        g.register(qf.ScalingFunction)
    x500 = torch.randn(500, device='cuda:0')
    quantization.uniformQuantization(x500, 16, bucket_size=256)            # binds the module's entry points
    variants = (('other', other), ('this', here))
    res = {name: {'host': [], 'wall': []} for name, _ in variants}

    def fn():
        quantization.uniformQuantization(x500, 16, bucket_size=256)

    for rep in range(reps):
        for name, g in (variants if rep % 2 == 0 else variants[::-1]):
            qf._glue_uniform, qf._glue_uniform_common = g.uniform, g.uniform_common
            res[name]['host'].append(host_only(fn, 6400))
            res[name]['wall'].append(wall(fn, 3000))
    qf._glue_uniform, qf._glue_uniform_common = here.uniform, here.uniform_common
    print("Host cost of uniformQuantization(500 el, s=16, bucket_size=256) -- the training loops' configuration, eager, default")
    print('stream -- through this tree\'s binding ("this") and through %s ("other"), both loaded in ONE' % os.path.basename(other_path))
    print('process, %d repetitions each, interleaved (order swapped every repetition).  host: host_only, 6400 calls; wall: best of' % reps)
    print('5 x 3000 calls (docs/history/tools/profile_api_overhead.py).  torch %s, %s' % (torch.__version__, torch.cuda.get_device_name(0)))
    print()
    print('%-8s %-8s %10s %10s %10s   %s' % ('binding', 'metric', 'median us', 'min us', 'max us', 'all'))
    for name, _ in variants:
        for metric in ('host', 'wall'):
            v = res[name][metric]
            print('%-8s %-8s %10.3f %10.3f %10.3f   %s' % (name, metric, statistics.median(v), min(v), max(v), ' '.join('%.3f' % t for t in v)))
    for metric in ('host', 'wall'):
        o, t = res['other'][metric], res['this'][metric]
        apart = min(t) > max(o) or min(o) > max(t)
        print('%s: this median - other median = %+.3f us; min-max ranges %s' % (metric, statistics.median(t) - statistics.median(o),
                                                                            'DO NOT overlap' if apart else 'overlap'))
    if hasattr(here, 'capture_query_probe'):
        q = [here.capture_query_probe(200000)[0] for _ in range(reps)]
        print()
        print('The capture query of uniform_common alone (hipStreamIsCapturing on the current stream, 200000 calls in a native loop,')
        print('%d repetitions): median %.4f us, min %.4f, max %.4f' % (reps, statistics.median(q), min(q), max(q)))


if __name__ == '__main__':
    main()

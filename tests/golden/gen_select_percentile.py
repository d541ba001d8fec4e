"""Runs the REFERENCE's initialize_quantization_points (quantization/help_functions.py:140-154, the staged copy under
oracle/_ref/) on the percentile cases of tests/select_cases.py -- a NaN of each sign, +inf and -inf at the first, a middle and
the last element, and the clean tensor, for n = 2000 / 70001, bucket 256 / None, k = 4 / 16 / 33 -- and writes what it returned
to tests/golden/select_percentile.json.  Data only: per case its id, a CRC-32 of the input's bytes (the inputs are rebuilt from
their seed by select_cases.percentile_input, so the fixture notices if that ever changes) and the bit patterns of the points.

What the fixture pins: once the scaled tensor holds one NaN, np.percentile returns NaN for EVERY point, and one +-inf makes
the scaled values of its bucket NaN, so it is the same case.  tests/test_oracle_golden.py holds the oracle's restatement
(oracle_np.init_points_percentile) to it; tests/test_select_host.py and tests/test_hip_select.py hold the package to the
reference and to np.percentile directly.

NOT SETTLED by this file: the all-NaN answer is numpy's, not the reference's own code.  It was observed with numpy 2.2.6 (the
version the fixture records under 'numpy'): np.percentile partitions, looks at the largest element and, if that is a NaN,
overwrites every result with NaN.  The reference calls whatever numpy is installed, so the fixture records what the staged
reference returned with THAT numpy; the docstring of help_functions.percentile_ranks already ties this package to numpy's
arithmetic, and a numpy that decided otherwise would show up here first when the file is regenerated.  CPU only, seconds:

    python tests/golden/gen_select_percentile.py
"""
import importlib
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import select_cases as S  # noqa: E402
from oracle import ref_stage  # noqa: E402


def main():
    refq = ref_stage.load()
    assert refq is not None, 'oracle/_ref is not staged: run __graft_entry__.build() where the reference exists'
    refh = importlib.import_module(refq.__name__ + '.help_functions')
    cases = []
    for shape in S.PCT_SHAPES:
        for cid, x, bucket, k in S.percentile_cases(shape):
            with np.errstate(invalid='ignore'):
                p = refh.initialize_quantization_points(torch.from_numpy(x), refq.ScalingFunction('linear', False, False, bucket), k)
            assert p.dtype == torch.float32 and p.shape == (k,)
            cases.append(dict(id=cid, n=int(x.size), bucket=bucket, k=k, input_crc32=zlib.crc32(x.tobytes()),
                              points_bits=[int(b) for b in p.numpy().view(np.uint32)]))
    head = dict(source='the staged reference: initialize_quantization_points(x, ScalingFunction("linear", False, False, bucket), k)',
                numpy=np.__version__, torch=torch.__version__.split('+')[0])
    path = os.path.join(ROOT, 'tests', 'golden', 'select_percentile.json')
    with open(path, 'w') as f:                                             # one case per line
        f.write(json.dumps(head)[:-1] + ', "cases": [\n' + ',\n'.join(json.dumps(c) for c in cases) + '\n]}\n')
    print('wrote', path, len(cases), 'cases,', sum(bool(np.isnan(np.array(c['points_bits'], np.uint32).view(np.float32)).all())
                                                 for c in cases), 'of them all-NaN')


if __name__ == '__main__':
    main()

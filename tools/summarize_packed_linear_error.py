#!/usr/bin/env python3
"""profiles/packed_linear_error.txt from the log tests/errlog.py writes while tests/test_hip_packed_layers.py runs on the device:
the largest |y - y64| / sum|terms| of the packed Linear layer per width, next to the bound.

    python tools/summarize_packed_linear_error.py [LOG.jsonl] [profiles/packed_linear_error.txt]

LOG defaults to errlog.LOG, the file that module appends to."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import errlog
    log = sys.argv[1] if len(sys.argv) > 1 else errlog.LOG
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'packed_linear_error.txt')
    rows = [r for r in (json.loads(l) for l in open(log) if l.strip()) if r['kind'] == 'packed_linear']
    if not rows:
        raise SystemExit('%s holds no packed_linear record: run tests/test_hip_packed_layers.py on the device first' % log)
    per = {}
    for r in rows:
        m = re.search(r'bits (\d)', r['case'])
        key = 'bits %s' % m.group(1) if m else 'modules (PackedLinear against unpack())'
        cur = per.setdefault(key, [0, 0.0, ''])
        cur[0] += 1
        if r['err_over_sum_abs_terms'] >= cur[1]:
            cur[1], cur[2] = r['err_over_sum_abs_terms'], r['case']
    worst = max(v[1] for v in per.values())
    lines = ['qdi_linear_packed_f32 / PackedLinear: |y - y64| / (sum_c |x w| + |bias|), y64 the float64 dot product with the bit-exact w',
             'bound %.1e; %d checks of tests/test_hip_packed_layers.py; largest ratio %.3e (%.1f x below the bound)'
             % (rows[0]['tol'], len(rows), worst, rows[0]['tol'] / worst if worst else float('inf')), '']
    for key in sorted(per):
        n, ratio, case = per[key]
        lines.append('%-40s %4d checks   max %.3e   at %s' % (key, n, ratio, case))
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Every header under csrc/ includes what it uses: a translation unit that includes ONLY that header passes hipcc's syntax check
for gfx950 with the build's own compile flags.  No GPU, nothing is launched; skipped where hipcc is not installed.  The pin of
the include hygiene of the bucket-transform headers (qd_launch.h, qd_points.h, qd_element.h, qd_bucket_*_kernels.h,
qd_single_kernels.h, qd_transform.h): a unit may take the launch helpers without the kernels, or one kernel family without the
others, and a header that leans on what its includer happened to include before it fails here."""
import os
import subprocess

import pytest

from quantized_distillation_amd import _lib
from quantized_distillation_amd import build as qb

HEADERS = sorted(f for f in os.listdir(_lib.CSRC) if f.endswith('.h'))


def test_the_list_has_the_headers_of_the_split():
    assert {'qd_common.h', 'qd_plan.h', 'qd_launch.h', 'qd_points.h', 'qd_element.h', 'qd_single_kernels.h',
            'qd_transform.h'} <= set(HEADERS)


@pytest.mark.parametrize('header', HEADERS)
def test_header_compiles_alone(header, tmp_path):
    try:
        hipcc = qb.hipcc()
    except RuntimeError as e:
        pytest.skip(str(e))
    tu = tmp_path / 'only_this_header.hip'
    tu.write_text('#include "%s"\n' % os.path.join(_lib.CSRC, header))
    r = subprocess.run([hipcc] + qb._compile_flags() + ['-fsyntax-only', str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

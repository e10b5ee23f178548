"""Build-time audit of the node-graph SPN query kernels (no GPU needed: hipcc cross-compiles
csrc/flat_spn_queries.hip): no scratch memory, no compare-and-swap loops."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
KERNELS = {'flat_topdown_kernel': 4, 'flat_backward_kernel': 1, 'flat_em_tables_kernel': 1, 'flat_em_update_kernel': 1}


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    src = os.path.join(ROOT, 'deeprob-kit_amd', 'csrc', 'flat_spn_queries.hip')
    out = str(tmp_path_factory.mktemp('fq') / 'flat_spn_queries.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(ROOT, 'include'),
                    '-S', '--cuda-device-only', src, '-o', out], check=True, cwd=os.path.dirname(src),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _bodies(text, prefix):
    names = re.findall(r'^(_ZN3dpk2fq\d+' + prefix + r'\w*):', text, re.M)
    return {n: re.search(r'^' + n + r':.*?^\s*s_endpgm', text, re.S | re.M).group(0) for n in names}


def _scratch(text, name):
    m = re.search(r'^\s*\.private_segment_fixed_size:\s*(\d+)', text.split('.name:           ' + name)[-1], re.M)
    return None if m is None else int(m.group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
@pytest.mark.parametrize('kernel', sorted(KERNELS))
def test_no_scratch_no_cas(asm, kernel):
    bodies = _bodies(asm, kernel)
    assert len(bodies) == KERNELS[kernel], sorted(bodies)
    for name, body in bodies.items():
        assert 'scratch_' not in body, name
        assert 'cmpswap' not in body, name
        assert _scratch(asm, name) == 0, name

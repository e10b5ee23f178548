"""Build-time audit of the MAF kernels' ISA (no GPU needed: hipcc cross-compiles csrc/maf.hip): the fused density
kernel multiplies on the fp32 matrix cores, and neither it nor the sampling kernel touches scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.fixture(scope='module')
def maf_asm(tmp_path_factory):
    src = os.path.join(ROOT, 'deeprob-kit_amd', 'csrc', 'maf.hip')
    out = str(tmp_path_factory.mktemp('maf') / 'maf.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(ROOT, 'include'),
                    '-S', '--cuda-device-only', src, '-o', out], check=True, cwd=os.path.dirname(src),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _bodies(text, prefix):
    names = re.findall(r'^(_ZN3dpk\d+' + prefix + r'\w*):', text, re.M)
    return {n: re.search(r'^' + n + r':.*?^\s*s_endpgm', text, re.S | re.M).group(0) for n in names}


def _scratch(text, name):
    m = re.search(r'^\s*\.private_segment_fixed_size:\s*(\d+)', text.split('.name:           ' + name)[-1], re.M)
    return None if m is None else int(m.group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_density_kernel_mfma_and_no_scratch(maf_asm):
    bodies = _bodies(maf_asm, 'maf_density_kernel')
    assert len(bodies) == 10, sorted(bodies)         # 5 activations x 2 hidden-tile counts
    for name, body in bodies.items():
        assert 'v_mfma_f32_32x32x2_f32' in body, name
        assert 'scratch_' not in body, name
        assert _scratch(maf_asm, name) in (0, None), name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sampling_kernel_no_scratch(maf_asm):
    bodies = _bodies(maf_asm, 'maf_sample_kernel')
    assert len(bodies) == 20, sorted(bodies)         # 5 activations x 4 widths
    for name, body in bodies.items():
        assert 'scratch_' not in body, name
        assert _scratch(maf_asm, name) in (0, None), name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_deep_sampling_kernel_no_scratch(maf_asm):
    bodies = _bodies(maf_asm, 'maf_sample_deep_kernel')
    assert len(bodies) == 1, sorted(bodies)
    for name, body in bodies.items():
        assert 'scratch_' not in body, name
        assert _scratch(maf_asm, name) in (0, None), name

"""Build-time audit of the slice kernel's steady K loop (csrc/ratspn_gemm_slice.hip; no GPU needed: hipcc cross-compiles).

The K-step's f16 split (split8_mix, csrc/ratspn_gemm_common.h) takes the low half's difference x - float(xh) from one
v_fma_mix_f32 per value instead of a v_cvt_f32_f16 and a subtract.  The work-group is paced by its own instruction stream
(DESIGN 3.3), so the budget is pinned where it was won: the steady loop -- the instructions between the first and the last
MFMA of the kernel's second group of 42 (7 K-steps x 6) -- converts nothing back to fp32 and holds at most 160 vector-ALU
instructions beside its MFMAs (205 before), in no more registers than before (253) and without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
KERNEL = r'_ZN3dpk24ratspn_gemm_slice_kernelILi\d+ELi\d+ELi\d+EEEv\w+'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_steady_k_loop_budget(tmp_path):
    src = os.path.join(ROOT, 'deeprob-kit_amd', 'csrc', 'ratspn_gemm_slice.hip')
    out = str(tmp_path / 'slice.s')
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(ROOT, 'include'),
                        '-S', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', src, '-o', out],
                       cwd=os.path.dirname(src), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    blocks = [b for b in re.split(r'remark: [^\n]*Function Name: ', r.stdout)[1:] if re.match(KERNEL, b.split()[0])]
    assert len(blocks) == 1, [b.split()[0] for b in blocks]
    vgprs = int(re.search(r' VGPRs: (\d+)', blocks[0]).group(1))
    scratch = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', blocks[0]).group(1))

    text = open(out).read()
    names = re.findall(r'^(' + KERNEL + r'):', text, re.M)
    assert len(names) == 1, names
    body = re.search(r'^' + names[0] + r':.*?^\s*s_endpgm', text, re.S | re.M).group(0)
    ins = [l.strip() for l in body.split('\n')]
    ins = [l for l in ins if l and not l.startswith(';') and not l.startswith('.') and not l.endswith(':')]
    mfma = [i for i, l in enumerate(ins) if l.startswith('v_mfma')]
    assert len(mfma) == 84, len(mfma)              # the first block's unrolled K-steps, then the steady loop's
    loop = ins[mfma[42]:mfma[83] + 1]
    valu = [l for l in loop if l.startswith('v_') and not l.startswith('v_mfma')]
    back = [l for l in loop if l.startswith('v_cvt_f32_f16')]
    mix = [l for l in loop if l.startswith('v_fma_mix_f32')]
    print('steady K loop: {} instructions, {} vector-ALU beside 42 MFMAs, {} v_fma_mix_f32, {} v_cvt_f32_f16; '
          '{} VGPRs, {} bytes of scratch'.format(len(loop), len(valu), len(mix), len(back), vgprs, scratch))
    assert not back, back
    assert len(valu) <= 160, len(valu)
    assert vgprs <= 253 and scratch == 0, (vgprs, scratch)
    # the mixed instruction's result goes through the compiler's own packed conversion, never straight into an MFMA
    # (in program order: the last vector-ALU writer of every register an MFMA takes its A and B operands from)
    assert mix
    last = {}
    for i, l in enumerate(loop):
        if not l.startswith('v_mfma'):
            if l.startswith('v_'):
                last[l.split()[1].rstrip(',')] = l.split()[0]
            continue
        for a, b in re.findall(r'v\[(\d+):(\d+)\]', l)[1:3]:
            for k in range(int(a), int(b) + 1):
                assert last.get('v{}'.format(k)) != 'v_fma_mix_f32', (i, l)

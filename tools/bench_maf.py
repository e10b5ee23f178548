#!/usr/bin/env python3
"""MAF(784) measurements on one GPU; prints one JSON line.

For the sequential and the random-degree (random_state=42) constructions:
  * eval log_prob at B = 65536 (step time);
  * one AutoregressiveLayer's density pass at B = 65536 on the fused kernel and on the chained route, same call;
    the fused kernel's share of the fp32 matrix-core bound over the non-zero K blocks it multiplies;
  * sample(n) for n = 100 and 65536 on the sampling kernel and on the step loop (the same conditioner op, D passes
    per layer), same call.
  * depth 2 (both constructions): sample(100) on the deep sampling kernel and on the step loop, sample(65536) on the
    kernel.
--trace: one sample(100) per construction only (for a rocprofv3 --kernel-trace run that counts launches).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deeprob-kit_amd'))
sys.path.insert(0, ROOT)

FP32_MATRIX_TFLOPS = 157.3


def _time(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _nonzero_block_flops(layer, B):
    """FLOPs the fused kernel multiplies: per 32-row tile, the packed K extent (8-wide groups) up to its last non-zero
    mask entry, in the packing order of ops_maf._orders."""
    from deeprob.hip import ops_maf
    m1 = layer.network[0].mask.cpu().numpy() != 0
    m2 = layer.network[2].mask.cpu().numpy() != 0
    D = m1.shape[1]
    i_ord, h_ord, o_ord = ops_maf.packing_orders(m1, m2, np.asarray(layer.inv_ordering))
    p1 = m1[h_ord][:, i_ord]
    p2 = (m2[:D] | m2[D:])[o_ord][:, h_ord]
    flops = 0
    for p in (p1, p2):
        for t in range(0, p.shape[0], 32):
            cols = np.nonzero(p[t:t + 32].any(0))[0]
            ext = 0 if len(cols) == 0 else (cols[-1] // 8 + 1) * 8
            flops += 2 * B * 32 * ext * (2 if p is p2 else 1)
    return flops


def run(seq, args, depth=1):
    from deeprob.flows.models import MAF
    from deeprob.hip import ops_maf
    torch.manual_seed(0)
    kw = dict(depth=depth) if seq else dict(sequential=False, random_state=42, depth=depth)
    m = MAF(784, **kw)
    from tests.util import randomise_flow
    randomise_flow(m, 1)
    m = m.cuda().eval()
    res = {}
    if args.trace:
        with torch.no_grad():
            m.sample(100)
        torch.cuda.synchronize()
        return res
    B = args.batch
    if depth > 1:       # the deep sampling kernel against the step loop
        with torch.no_grad():
            res['sample100_kernel_ms'] = _time(lambda: m.sample(100), 3, warm=1)
            loop = ops_maf.deep_sample_envelope
            ops_maf.deep_sample_envelope = lambda layer: False
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.sample(100)
                torch.cuda.synchronize()
                res['sample100_steploop_ms'] = (time.perf_counter() - t0) * 1e3
            finally:
                ops_maf.deep_sample_envelope = loop
            res['sample100_speedup'] = res['sample100_steploop_ms'] / res['sample100_kernel_ms']
            res['sample{}_kernel_ms'.format(B)] = _time(lambda: m.sample(B), 3, warm=1)
        return res
    x = torch.randn(B, 784, device='cuda')
    with torch.no_grad():
        res['logprob_ms'] = _time(lambda: m(x), 10)
        layer = m.layers[0]
        res['density_fused_ms'] = _time(lambda: ops_maf.density_fused(x, layer), 10)
        res['density_chain_ms'] = _time(lambda: ops_maf.density_chain(x, layer), 10)
        res['density_ratio'] = res['density_fused_ms'] / res['density_chain_ms']
        fl = _nonzero_block_flops(layer, B)
        res['density_nonzero_gflop'] = fl / 1e9
        res['density_fp32_bound_share'] = (fl / (FP32_MATRIX_TFLOPS * 1e12) * 1e3) / res['density_fused_ms']
        for n in (100, B):
            res['sample{}_kernel_ms'.format(n)] = _time(lambda: m.sample(n), 3, warm=1)
            env = ops_maf.sample_envelope
            ops_maf.sample_envelope = lambda layer: False
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.sample(n)
                torch.cuda.synchronize()
                res['sample{}_steploop_ms'.format(n)] = (time.perf_counter() - t0) * 1e3
            finally:
                ops_maf.sample_envelope = env
            res['sample{}_speedup'.format(n)] = res['sample{}_steploop_ms'.format(n)] / res['sample{}_kernel_ms'.format(n)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'batch': args.batch}
    for seq in (True, False):
        for k, v in run(seq, args).items():
            out[('seq_' if seq else 'rand_') + k] = round(v, 4) if isinstance(v, float) else v
    for seq in (True, False):
        for k, v in run(seq, args, depth=2).items():
            out[('depth2_seq_' if seq else 'depth2_rand_') + k] = round(v, 4) if isinstance(v, float) else v
    print(json.dumps(out))


if __name__ == '__main__':
    main()

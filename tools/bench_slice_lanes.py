"""Same-process A/B of the slice mapping's lane count (dps_slice_lanes, include/deeprob_slice.h): every launch on the whole
chip (1) against auto mode / the stated value (0), alternating, on the two loops that run slice launches side by side
(a window is captured under each setting: 0 = what its chains state):

  * the eager two-stream loop of `bench.py --gpus 1` (two evaluation streams, a model replica each, 65 536 samples);
  * the graphed evaluation window on three chains (`bench.py --graph-window`, the shard entries of `--full`) at 65 536,
    32 768, 16 384 and 8 192 samples: one window captured under each setting, replayed in turn.

    python tools/bench_slice_lanes.py [--rounds 5] [--steps 200] [--fixed 2]

Prints one JSON line per case: ms per step of every round, median and range per setting.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 784


def summary(v):
    return {'median': round(statistics.median(v), 5), 'min': round(min(v), 5), 'max': round(max(v), 5),
            'runs': [round(t, 5) for t in v]}


def eager_two_streams(model, xs, rounds, steps, settings, sl, sync_every=0):
    from deeprob.parallel import ShardedLogLikelihood
    dev = xs[0].device
    replicas = [model, copy.deepcopy(model)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    evs = [ShardedLogLikelihood(m, static_inputs=True, static_params=False) for m in replicas]

    hist = {}

    def loop(n, count=None):
        for i in range(n):
            with torch.cuda.stream(streams[i % 2]):
                evs[i % 2].step(xs[i % len(xs)])
            if count is not None:
                g = sl.last_grid()
                count[g] = count.get(g, 0) + 1
            if sync_every and (i + 1) % sync_every == 0:      # (a caller that synchronises now and then: DPS_AUTO_REENTRY)
                torch.cuda.synchronize()

    def drain():
        torch.cuda.synchronize()
        return [e.drain() for e in evs]

    for _ in range(3):          # (the runtime's per-queue pool growth: outside the timed windows)
        loop(256)
        drain()
    out = {s: [] for s in settings}
    grids, means = {}, {}
    for _ in range(rounds):
        for s in settings:
            sl.lanes(s)
            loop(16)
            drain()
            t0 = time.perf_counter()
            loop(steps, hist.setdefault(s, {}))
            torch.cuda.synchronize()
            out[s].append((time.perf_counter() - t0) / steps * 1e3)
            grids[s] = dict(hist[s])
            means[s] = drain()[0][-1]
    sl.lanes(0)
    ref = means[settings[0]]
    assert all(abs(m - ref) <= 1e-9 * abs(ref) for m in means.values()), means
    return {'case': 'eager two streams', 'B': xs[0].shape[0], 'steps': steps, 'sync_every': sync_every,
            'reentry': os.environ.get('DPK_SLICE_REENTRY', 'DPS_AUTO_REENTRY'),
            'ms_per_step': {str(s): dict(summary(v), grids=grids[s]) for s, v in out.items()}}


def window(model, xs, rounds, settings, sl, chains=3, reps=4):
    from deeprob.parallel import ShardedLogLikelihood, GraphedEvaluationWindow
    wins, means = {}, {}
    for s in settings:
        sl.lanes(s)
        wins[s] = GraphedEvaluationWindow(ShardedLogLikelihood(model, static_inputs=True), list(xs) * reps, chains=chains)
        means[s] = wins[s].replay()
    sl.lanes(0)
    ref = means[settings[0]]
    assert all(abs(a - b) <= 1e-9 * abs(b) for m in means.values() for a, b in zip(m, ref)), means
    n = reps * len(xs)
    out = {s: [] for s in settings}
    for s in settings:          # (an untimed round)
        for _ in range(10):
            wins[s].graph.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for s in settings:
            g = wins[s].graph
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[s].append(e0.elapsed_time(e1) / (5 * n))
    for w in wins.values():
        w.close()
    return {'case': 'graphed window, {} chains'.format(chains), 'B': xs[0].shape[0], 'steps_per_replay': n,
            'ms_per_step': {str(s): summary(v) for s, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--fixed', type=int, default=0, help='also measure this fixed lane count in the eager loop (0: no)')
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--sync-every', type=int, default=0, help='synchronise after every this many steps of the eager loop (0: never)')
    ap.add_argument('--window-lanes', type=int, nargs='*', default=[], help='further fixed lane counts for the windows')
    args = ap.parse_args()
    from deeprob.hip import slice as sl
    from deeprob.spn.models import GaussianRatSpn
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = GaussianRatSpn(D, rg_depth=2, rg_repetitions=8, rg_batch=2, rg_sum=2, random_state=42).eval().to(dev)
    with torch.no_grad():
        xs = [torch.randn(65536, D, device=dev) for _ in range(4)]
        settings = [1, 0] + ([args.fixed] if args.fixed > 1 else [])
        print(json.dumps(eager_two_streams(model, xs, args.rounds, args.steps, settings, sl, args.sync_every)), flush=True)
        for B in (() if args.no_window else (65536, 32768, 16384, 8192)):
            nb = max(2, -(-(320 << 20) // (B * D * 4)))
            xb = xs[:nb] if B == 65536 else [torch.randn(B, D, device=dev) for _ in range(nb)]
            print(json.dumps(window(model, xb, args.rounds, [1, 0] + args.window_lanes, sl, reps=max(1, -(-32 // nb)))), flush=True)


if __name__ == '__main__':
    main()

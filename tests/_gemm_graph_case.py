"""Body of tests/test_gemm_f32_gpu.py::test_split_k_fallback_inside_a_graph_capture, run as a child process
(``python -m tests._gemm_graph_case``): the FIRST library call of the process is a MaskedLinear forward and backward
captured into a graph, so that launch_gemm cannot allocate its per-device pool of partial tiles and the split-K products
take the atomicAdd fallback (C zeroed, partial sums added by atomics, gemm_epilogue_kernel) -- all of it captured.
The graph is one chain on one stream.  Prints one line per replay: MARK + json of y, grad_x, grad_W, grad_b."""
import json

import numpy as np
import torch

MARK = 'GEMM-GRAPH-REPLAY '
REPLAYS = 2
SHAPE = (130, 200, 70)       # forward 6 tiles x 4 slices (the last 8 wide), grad_W 8 tiles x 3 slices (the last 2 wide)


def inputs(replay: int):
    """Integer data (-4 .. 4: exact in fp32 in any summation order) of a replay; the mask is the same for all."""
    B, fin, fout = SHAPE
    rs = np.random.RandomState(77 + replay)
    draw = lambda *s: rs.randint(-4, 5, size=s).astype(np.float32)
    return dict(x=draw(B, fin), W=draw(fout, fin), b=draw(fout), gy=draw(B, fout),
                mask=np.random.RandomState(76).rand(fout, fin) < 0.5)


def main():
    from deeprob.torch.utils import MaskedLinear
    B, fin, fout = SHAPE
    dev = torch.device('cuda', 0)
    lin = MaskedLinear(fin, fout, inputs(0)['mask']).to(dev)
    x = torch.zeros(B, fin, device=dev, requires_grad=True)
    gy = torch.zeros(B, fout, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = lin(x)
        gx, gW, gb = torch.autograd.grad(y, (x, lin.weight, lin.bias), gy)
    for replay in range(REPLAYS):
        d = inputs(replay)
        with torch.no_grad():
            x.copy_(torch.from_numpy(d['x']))
            gy.copy_(torch.from_numpy(d['gy']))
            lin.weight.copy_(torch.from_numpy(d['W']))
            lin.bias.copy_(torch.from_numpy(d['b']))
        graph.replay()           # (right behind the copies, no synchronisation in between: as a training loop replays)
        torch.cuda.synchronize()
        print(MARK + json.dumps(dict(y=y.detach().cpu().reshape(-1).tolist(), gx=gx.cpu().reshape(-1).tolist(),
                                     gW=gW.cpu().reshape(-1).tolist(), gb=gb.cpu().reshape(-1).tolist())), flush=True)
    del graph
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()

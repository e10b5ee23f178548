"""Posterior marginals of Chow-Liu trees and cutset networks on the device (``dpc_mar_clt`` / ``dpc_mar_cnet``,
``deeprob.hip.clt.marginals`` / ``deeprob.hip.cnet.marginals``, ``BinaryCLT.marginals`` / ``BinaryCNet.marginals``) against the
float64 numpy restatement (tests/marginals_ref.py), on poisoned, guard-banded memory (tests/buffer_contract.py).

The bar is an absolute 1e-5 on a probability: the project's log-likelihood parity bar carried over to values in [0, 1].
The float32 restatement stays within 2.5e-6 of the float64 one on every fixture and the device differs from it only by
its ``expf`` / ``log1pf``.  No rows are set aside: there are no ties and no draws in this query."""
import numpy as np
import pytest
import torch

from tests import clt_ref
from tests import cnet_ref
from tests import marginals_ref as mref
from tests.buffer_contract import PATTERNS, contract
from tests.test_clt_gpu import fitted as fitted_tree
from tests.test_cnet_gpu import as_ref_model, fitted as fitted_net
from tests.test_marginals_host import deterministic_chain

pytestmark = pytest.mark.gpu
BAR = 1e-5
TREES = ['d10', 'd16', 'd33', 'd130', 'drawn24']
NETS = list(cnet_ref.CONFIGS)
_want = {}


def device(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def here():
    return torch.device('cuda', torch.cuda.current_device())


def run(op, tables, x):
    """``op(tables, x)`` as numpy under both poison patterns: x and the model's buffer frozen, every element of the output
    written, the same bytes both times."""
    xd = device(x)
    results = []
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, tables._buf)
            out = op(tables, xd)
            c.expect_written(out)
        results.append(out.cpu().numpy())
    assert results[0].tobytes() == results[1].tobytes()
    assert results[0].shape == x.shape and results[0].dtype == np.float32
    return results[0]


def tree_run(m, x):
    from deeprob.hip import clt
    return run(clt.marginals, m._on_device(here()), x)


def net_run(m, x):
    from deeprob.hip import cnet
    return run(cnet.marginals, m._on_device(here()), x)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def wanted(kind, name):
    """``(query rows, float64 restatement, float32 restatement)`` of the package's model of a fixture; once."""
    if (kind, name) not in _want:
        if kind == 'tree':
            m, q = fitted_tree(name), clt_ref.golden(name)['q']
            both = [mref.tree_marginals(m.bfs, m.tree, m.params, q, dtype) for dtype in (np.float64, np.float32)]
        else:
            model, q = as_ref_model(fitted_net(name)), cnet_ref.queries(name, n=128 if name in ('d5', 'd10') else 256)
            both = [mref.cnet_marginals(model, q, dtype) for dtype in (np.float64, np.float32)]
        _want[kind, name] = (q, both[0], both[1].astype(np.float64))
    return _want[kind, name]


def check(kind, name, m, out):
    q, want, single = wanted(kind, name)
    obs = ~np.isnan(q)
    assert same_bits(out[obs], q[obs])
    assert not np.isnan(out).any() and out.min() >= 0.0 and out.max() <= 1.0
    public = m.marginals(q)
    assert isinstance(public, np.ndarray) and public.tobytes() == out.tobytes()
    on_device = m.marginals(device(q))
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and on_device.cpu().numpy().tobytes() == out.tobytes()
    print('%s %s: device %.3g, float32 restatement %.3g from the float64 restatement' % (
        kind, name, np.abs(out - want).max(), np.abs(single - want).max()))
    assert np.abs(out - want).max() <= BAR


# ---- against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TREES)
def test_tree_marginals_match_the_restatement(name):
    m = fitted_tree(name)
    check('tree', name, m, tree_run(m, wanted('tree', name)[0]))


@pytest.mark.parametrize('name', NETS)
def test_network_marginals_match_the_restatement(name):
    m = fitted_net(name)
    out = net_run(m, wanted('net', name)[0])
    check('net', name, m, out)
    q, want, _ = wanted('net', name)
    assert np.isnan(q[0]).all() and not np.isnan(q[1]).any()
    assert same_bits(out[1], q[1])                                              # the complete row, unchanged
    prior = mref.cnet_marginals(as_ref_model(m), np.full((1, q.shape[1]), np.nan, np.float32), np.float64)
    assert np.abs(out[0] - prior[0]).max() <= BAR                               # the all-NaN row: the prior marginals


def test_an_all_nan_row_of_a_tree_gives_the_priors_and_a_complete_row_comes_back():
    m = fitted_tree('d33')
    x = np.stack([np.full(33, np.nan, np.float32), clt_ref.golden('d33')['x'][0]])
    out = tree_run(m, x)
    prior = mref.tree_marginals(m.bfs, m.tree, m.params, x[:1], np.float64)
    assert np.abs(out[0] - prior[0]).max() <= BAR and 0.0 < out[0].min() and out[0].max() < 1.0
    assert same_bits(out[1], x[1])


# ---- the batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 63, 65])
def test_rows_do_not_depend_on_the_batch(b):
    m, q = fitted_tree('d130'), wanted('tree', 'd130')[0]
    assert tree_run(m, q[:b]).tobytes() == tree_run(m, q)[:b].tobytes()
    m, q = fitted_net('d33'), wanted('net', 'd33')[0]
    assert net_run(m, q[:b]).tobytes() == net_run(m, q)[:b].tobytes()


def test_a_long_batch_in_pieces_gives_the_same_bytes(monkeypatch):
    from deeprob.hip import clt, cnet
    tree, g = fitted_tree('d16'), clt_ref.golden('d16')
    qt = np.concatenate([g['q'], g['q'], g['q'][:100]])
    net = fitted_net('d24')
    qn = np.concatenate([cnet_ref.queries('d24', n=512, seed=s) for s in (5, 6, 7, 8)] + [cnet_ref.queries('d24', n=52, seed=9)])
    assert len(qt) == len(qn) == 2100
    whole = tree_run(tree, qt), net_run(net, qn)
    monkeypatch.setattr(clt, 'WORK_FLOATS', 0)
    monkeypatch.setattr(cnet, 'WORK_BYTES', 0)
    assert clt.query_rows(16) == 1024 and cnet.query_rows(net._on_device(here()).marginals_row_bytes) == 1024
    pieces = tree_run(tree, qt), net_run(net, qn)
    for a, b in zip(whole, pieces):
        assert a.tobytes() == b.tobytes()


# ---- hand-built models -------------------------------------------------------------------------------------------------------
def test_the_smallest_models():
    from deeprob.hip import clt, cnet
    nan = np.nan
    # one variable
    one = clt.DeviceTree([0], [-1], np.log(np.array([[[0.3, 0.7], [0.3, 0.7]]], np.float32)), here())
    out = run(clt.marginals, one, np.array([[nan], [1.0], [0.0]], np.float32))
    assert abs(out[0, 0] - 0.7) <= 1e-6 and out[1:, 0].tolist() == [1.0, 0.0]
    # M = 1: a lone leaf over two columns; column 1 follows column 0 with probability 0.9
    params = np.log(np.array([[[0.3, 0.7], [0.3, 0.7]], [[0.9, 0.1], [0.1, 0.9]]], np.float32))
    lone = cnet.DeviceCNet(2, [-1], [[0, -1]], [[0.0, 0.0]], [([0, 1], [0, 1], [-1, 0], params)], here())
    assert (lone.n_nodes, lone.levels, lone.covered) == (1, 1, True)
    model = [dict(or_id=-1, weights=None, children=None, scope=[0, 1], bfs=np.array([0, 1]), tree=np.array([-1, 0]), params=params)]
    x = np.array([[nan, nan], [nan, 1.0], [0.0, nan], [1.0, 0.0]], np.float32)
    out = run(cnet.marginals, lone, x)
    assert np.abs(out - mref.cnet_by_enumeration(model, x)).max() <= BAR and same_bits(out[3], x[3])
    # one-variable leaves under one cut
    half = np.full((1, 2, 2), np.log(0.5), np.float32)
    skew = np.log(np.array([[[0.2, 0.8], [0.2, 0.8]]], np.float32))
    net = cnet.DeviceCNet(2, [0, -1, -1], [[1, 2], [0, -1], [1, -1]], np.log([[0.4, 0.6], [0.5, 0.5], [0.5, 0.5]]),
                          [([1], [0], [-1], half), ([1], [0], [-1], skew)], here())
    assert net.covered and net.max_leaf_d == 1
    x = np.array([[nan, nan], [nan, 0.0], [1.0, nan], [nan, 1.0]], np.float32)
    out = run(cnet.marginals, net, x)
    want = [[0.6, 0.4 * 0.5 + 0.6 * 0.8], [0.6 * 0.2 / (0.6 * 0.2 + 0.4 * 0.5), 0.0], [1.0, 0.8],
            [0.6 * 0.8 / (0.6 * 0.8 + 0.4 * 0.5), 1.0]]
    assert np.abs(out - np.array(want)).max() <= 1e-6


def test_a_deterministic_table_and_evidence_that_cannot_happen():
    from deeprob.spn.structure.cltree import BinaryCLT
    bfs, tree, params, x = deterministic_chain()
    with np.errstate(divide='ignore'):
        want = mref.tree_by_enumeration(tree, params, x)
    out = tree_run(BinaryCLT([0, 1, 2], tree=tree, params=params), x)
    obs = ~np.isnan(x)
    assert same_bits(out[obs], x[obs])
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(out).sum() == 1 and np.isnan(out[2, 2])
    assert np.nanmax(np.abs(out - want)) <= BAR
    assert np.abs(out[0] - [1.0, 1.0, 0.7]).max() <= 1e-6
    # the same leaf under a cut whose left side cannot happen: the weight -inf leaves the right side alone
    from deeprob.hip import cnet
    with np.errstate(divide='ignore'):
        net = cnet.DeviceCNet(4, [3, -1, -1], [[1, 2], [0, -1], [1, -1]], np.log([[0.0, 1.0], [0.5, 0.5], [0.5, 0.5]]),
                              [([0, 1, 2], bfs, tree, params)] * 2, here())
    nan = np.nan
    rows = np.array([[nan, 1, nan, nan], [0, 1, nan, nan], [nan, nan, nan, 0]], np.float32)
    out = run(cnet.marginals, net, rows)
    assert np.abs(out[0] - [1.0, 1.0, 0.7, 1.0]).max() <= 1e-6
    assert same_bits(out[1, :2], rows[1, :2]) and np.isnan(out[1, 2:]).all()
    assert np.isnan(out[2, :3]).all() and out[2, 3] == 0.0


def deep_tables():
    """Three levels: column 0 cut at the root, column 1 cut on its right side, one-variable leaves."""
    half = np.full((1, 2, 2), np.log(0.5), np.float32)
    two = np.full((2, 2, 2), np.log(0.5), np.float32)
    return dict(d=3, node_col=[0, -1, 1, -1, -1], node_child=[[1, 2], [0, -1], [3, 4], [1, -1], [2, -1]],
                node_logw=np.log(np.full((5, 2), 0.5)),
                leaves=[([1, 2], [0, 1], [-1, 0], two), ([2], [0], [-1], half), ([2], [0], [-1], half)])


def deep_rows():
    nan = np.nan
    return np.array([[nan, nan, nan], [1.0, nan, 0.0], [0.0, nan, 1.0], [1.0, 0.0, 1.0], [nan, 1.0, nan]], np.float32)


def test_tables_deeper_than_levels_give_nan_rows_and_stay_inside_the_stack():
    from deeprob.hip import clt, cnet
    lib = clt.load_library()
    net = cnet.DeviceCNet(device=here(), **deep_tables())
    assert net.levels == 3 and net.covered
    x = deep_rows()
    want = run(cnet.marginals, net, x)
    assert np.abs(want - [[.5, .5, .5], [1, .5, 0], [0, .5, 1], [1, 0, 1], [.5, 1, .5]]).max() <= 1e-6
    xd = device(x)
    for levels in (2, 1):
        for pattern in PATTERNS:
            with contract(pattern) as c:
                c.frozen(xd, net._buf)
                codes = clt.pack_query(xd)
                work = torch.empty(len(x) * (20 * levels + 8 * net.max_leaf_d + 8 * 3), dtype=torch.uint8, device=xd.device)
                out = torch.empty((len(x), 3), dtype=torch.float32, device=xd.device)
                clt.call(lib.dpc_mar_cnet, xd.data_ptr(), codes.data_ptr(), len(x), 3, net.n_nodes, net.node_col.data_ptr(),
                         net.node_child.data_ptr(), net.node_logw.data_ptr(), net.leaf_meta.data_ptr(),
                         net.leaf_ints.data_ptr(), net.leaf_params.data_ptr(), levels, net.max_leaf_d, work.data_ptr(),
                         out.data_ptr(), None)
                c.expect_written(out)
            out = out.cpu().numpy()
            obs = ~np.isnan(x)
            assert same_bits(out[obs], x[obs])
            # levels = 2 still holds the path root -> node 1 (x0 = 0); everything else needs the third level
            fits = np.array([False, False, levels == 2, True, False])
            assert np.isnan(out[~fits][np.isnan(x[~fits])]).all()
            assert same_bits(out[fits], want[fits])


@pytest.mark.parametrize('entry', ['dpc_cnet_log_likelihood', 'dpc_cnq_mpe', 'dpc_cnq_sample'])
def test_the_other_network_queries_keep_the_same_guard(entry):
    """The walk is one piece of code (or_walk, clt_common.h) and its guard must hold at every entry point that runs it:
    with ``work`` sized for the declared ``levels`` only, a row whose walk needs a deeper stack is answered with NaN (the
    fills: the whole row, observed entries included, and ``choice`` = -1), every other row with the bits of the
    full-``levels`` answer, and nothing is written outside the buffers.  The likelihood answers the complete row 3 at any
    ``levels`` (its stack-free path); the fills send it through the stack."""
    from deeprob.hip import clt, cnet
    lib = clt.load_library()
    net = cnet.DeviceCNet(device=here(), **deep_tables())
    x = deep_rows()
    xd = device(x)
    b, fill, seed = len(x), entry != 'dpc_cnet_log_likelihood', 12345
    if entry == 'dpc_cnet_log_likelihood':
        want, want_choice = cnet.log_likelihood(net, xd).cpu().numpy(), None
    elif entry == 'dpc_cnq_mpe':
        want, want_choice = (t.cpu().numpy() for t in cnet.mpe(net, xd, return_choice=True))
    else:
        want, want_choice = (t.cpu().numpy() for t in cnet.sample(net, xd, seed, return_choice=True))
    assert np.isfinite(want).all()
    for levels in (2, 1):
        for pattern in PATTERNS:
            with contract(pattern) as c:
                c.frozen(xd, net._buf)
                codes = clt.pack_query(xd)
                work = torch.empty(b * ((16 if fill else 12) * levels + 8 * net.max_leaf_d), dtype=torch.uint8, device=xd.device)
                out = torch.empty((b, 3) if fill else b, dtype=torch.float32, device=xd.device)
                choice = torch.empty(b, dtype=torch.int32, device=xd.device) if fill else None
                tables = (net.leaf_meta.data_ptr(), net.leaf_ints.data_ptr(), net.leaf_params.data_ptr(), levels, net.max_leaf_d)
                if not fill:
                    clt.call(lib.dpc_cnet_log_likelihood, codes.data_ptr(), b, 3, net.n_nodes, net.node_col.data_ptr(),
                             net.node_child.data_ptr(), net.node_logw.data_ptr(), *tables, work.data_ptr(), out.data_ptr(), None)
                else:
                    head = (xd.data_ptr(), codes.data_ptr(), b, 3, net.n_nodes, net.node_col.data_ptr(),
                            net.node_child.data_ptr(), net.node_parent.data_ptr(), net.node_logw.data_ptr()) + tables
                    tail = (work.data_ptr(), out.data_ptr(), choice.data_ptr(), None)
                    clt.call(getattr(lib, entry), *head, *((seed, 0) if entry == 'dpc_cnq_sample' else ()), *tail)
                c.expect_written(out)       # (not `choice`: its -1 is the bytes of the poison 0xFF)
            out = out.cpu().numpy()
            if fill:
                # levels = 2 still holds the path root -> node 1 (x0 = 0); the complete row 3 goes through node 2
                fits = np.array([False, False, levels == 2, False, False])
                choice = choice.cpu().numpy()
                assert (choice[~fits] == -1).all() and np.array_equal(choice[fits], want_choice[fits])
            else:
                fits = np.array([False, False, levels == 2, True, False])
            assert np.isnan(out[~fits]).all()
            assert same_bits(out[fits], want[fits])


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_what_the_header_excludes():
    from deeprob.hip import clt as C
    lib = C.load_library()
    buf = torch.zeros(64, dtype=torch.int64, device='cuda')
    p = buf.data_ptr()

    def net(x=p, codes=p, b=4, d=4, n_nodes=1, col=p, child=p, logw=p, meta=p, ints=p, params=p, levels=1, max_leaf_d=1,
            work=p, out=p):
        return (x, codes, b, d, n_nodes, col, child, logw, meta, ints, params, levels, max_leaf_d, work, out, None)

    def tree(x=p, codes=p, b=4, d=4, bfs=p, parent=p, params=p, child_off=p, child_idx=p, work=p, out=p):
        return (x, codes, b, d, bfs, parent, params, child_off, child_idx, work, out, None)

    net_cases = [dict(d=0), dict(d=C.DPC_MAX_D + 1), dict(b=-1), dict(b=2 ** 31), dict(n_nodes=0), dict(n_nodes=1 << 29),
                 dict(levels=6), dict(levels=0), dict(max_leaf_d=5), dict(max_leaf_d=0), dict(work=p + 4), dict(x=None),
                 dict(codes=None), dict(col=None), dict(child=None), dict(meta=None), dict(ints=None), dict(params=None),
                 dict(work=None), dict(out=None), dict(logw=None, n_nodes=3)]
    for case in net_cases:
        assert lib.dpc_mar_cnet(*net(**case)) == C.DPC_EINVAL and b'dpc_mar_cnet' in lib.dpc_last_error(), case
    tree_cases = [dict(d=0), dict(d=C.DPC_MAX_D + 1), dict(b=-1), dict(b=2 ** 31), dict(x=None), dict(codes=None), dict(bfs=None),
                  dict(parent=None), dict(params=None), dict(child_off=None), dict(child_idx=None), dict(work=None),
                  dict(out=None)]
    for case in tree_cases:
        assert lib.dpc_mar_clt(*tree(**case)) == C.DPC_EINVAL and b'dpc_mar_clt' in lib.dpc_last_error(), case
    before = buf.clone()
    assert lib.dpc_mar_cnet(*net(b=0)) == C.DPC_OK and lib.dpc_mar_clt(*tree(b=0)) == C.DPC_OK
    assert lib.dpc_mar_cnet(*net(b=0, logw=None)) == C.DPC_OK                   # a lone leaf has no weights
    assert lib.dpc_mar_clt(*tree(b=0, d=1, child_idx=None)) == C.DPC_OK         # a one-variable tree has no children
    torch.cuda.synchronize()
    assert torch.equal(buf, before)

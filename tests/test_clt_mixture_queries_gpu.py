"""The posterior queries of a mixture of Chow-Liu trees on the device (``dpc_mixq_marginals`` / ``dpc_mixq_sample`` /
``dpc_mixq_mpe``, ``deeprob.hip.clt.mixture_marginals`` / ``mixture_sample`` / ``mixture_mpe``, ``BinaryCLTMixture.marginals``
/ ``sample`` / ``mpe``) against the numpy restatement and the enumeration of tests/clt_mixture_queries_ref.py, on poisoned,
guard-banded memory (tests/buffer_contract.py): inputs frozen, every output element written, the same bytes under both
poison patterns.

Bars.  Marginals: an absolute 1e-5 on a probability against the float64 restatement (the project's bar; the float32
restatement's own distance is printed beside the device's).  Sampling: replayed draw by draw; a row in which a draw lies
within 1e-5 of its probability may fall either way and is set aside (at most 2 % of the rows; the restatement alone sets
aside about 0.3 %, tests/test_clt_mixture_queries_host.py), and the frequencies of 20 000 draws lie within 4 binomial
standard errors of the enumerated posterior.  MPE: by value, ``log(w_k p_k(out))`` of the returned pair in float64 within
1e-5 * max(1, |want|) of the restated and of the enumerated maximum, so that two pairs that tie to float32 rounding are
both right."""
import numpy as np
import pytest
import torch

from tests import clt_mixture_queries_ref as qref
from tests import clt_ref
from tests.buffer_contract import PATTERNS, contract
from tests.cnet_queries_ref import N_DRAWS, PATTERNS_D5

pytestmark = pytest.mark.gpu
BAR = 1e-5
CASES = [(d, k) for d in qref.DS for k in qref.KS]
_want = {}


def here():
    return torch.device('cuda', torch.cuda.current_device())


def device(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def tables(model):
    from deeprob.hip import clt
    trees, logw = model
    return clt.DeviceMixture(trees, logw, here())


def run(what, dm, x, seed=0, row0=0):
    """``(out, component or None)`` as numpy from the binding under both poison patterns: x and the model's buffer frozen,
    every element of ``out`` written (``component`` may hold -1, the bytes of the poison 0xFF), the same bytes both times."""
    from deeprob.hip import clt
    xd = device(x)
    results = []
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, dm._buf)
            if what == 'marginals':
                out, comp = clt.mixture_marginals(dm, xd), None
            elif what == 'mpe':
                out, comp = clt.mixture_mpe(dm, xd, want_component=True)
            else:
                out, comp = clt.mixture_sample(dm, xd, seed, row0, want_component=True)
            c.expect_written(out)
        results.append((out.cpu().numpy(), None if comp is None else comp.cpu().numpy()))
    (a, ca), (b, cb) = results
    assert a.tobytes() == b.tobytes() and a.shape == x.shape and a.dtype == np.float32
    if ca is not None:
        assert ca.tobytes() == cb.tobytes() and ca.dtype == np.int32 and ca.shape == (len(x),)
    return a, ca


class Wanted:
    """The restatement's answers for the rows ``x``, each computed when first asked for and kept: ``m64`` / ``m32`` the
    float64 and float32 marginals, ``replay`` the replay of seed 2024, ``mpe`` the float32 MPE."""

    def __init__(self, model, x):
        self.model, self.x, self.have = model, x, {}

    def __getitem__(self, what):
        if what not in self.have:
            with np.errstate(invalid='ignore', divide='ignore'):
                self.have[what] = {'m64': lambda: qref.marginals(self.model, self.x),
                                   'm32': lambda: qref.marginals(self.model, self.x, np.float32),
                                   'replay': lambda: qref.sample_replay(self.model, self.x, 2024),
                                   'mpe': lambda: qref.mpe(self.model, self.x)}[what]()
        return self.have[what]


def wanted(model, x, key):
    if key not in _want:
        _want[key] = Wanted(model, x)
    return _want[key]


def public(d, k):
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    trees, _ = qref.random_model(d, k)
    scope = list(range(d))
    return BinaryCLTMixture(scope, [BinaryCLT(scope, tree=t.copy(), params=p.copy()) for _, t, p in trees],
                            qref.random_weights(d, k))


def check_marginals(tag, model, x, out, want):
    obs = ~np.isnan(x)
    assert same_bits(out[obs], x[obs])
    assert np.array_equal(np.isnan(out), np.isnan(want['m64']))
    dev, own = np.nanmax(np.abs(out - want['m64']), initial=0.0), np.nanmax(np.abs(want['m32'] - want['m64']), initial=0.0)
    print('%s: device %.3g, float32 restatement %.3g from the float64 restatement' % (tag, dev, own))
    assert dev <= BAR
    if not np.isnan(out).any():
        assert out.min() >= 0.0 and out.max() <= 1.0 + 1e-6
    if x.shape[1] <= 10:
        with np.errstate(invalid='ignore', divide='ignore'):
            exact = qref.marginals_by_enumeration(model, x)
        assert np.array_equal(np.isnan(out), np.isnan(exact)) and np.nanmax(np.abs(out - exact), initial=0.0) <= BAR


def check_replay(x, out, comp, want):
    filled, want_comp, near = want['replay']
    obs = ~np.isnan(x)
    assert same_bits(out[obs], x[obs])
    keep = ~near[:len(x)]
    assert near.mean() <= 0.02
    assert same_bits(out[keep], filled[:len(x)][keep]) and np.array_equal(comp[keep], want_comp[:len(x)][keep])


def check_mpe(tag, model, x, out, comp, want):
    obs = ~np.isnan(x)
    assert same_bits(out[obs], x[obs])
    filled, want_comp = want['mpe']
    alive = want_comp[:len(x)] >= 0
    assert np.array_equal(comp >= 0, alive) and set(np.unique(out[alive])) <= {0.0, 1.0}
    assert same_bits(out[~alive], x[~alive]) and (comp[~alive] == -1).all()
    if not alive.any():
        return
    got = qref.log_joint(model, comp[alive], out[alive])
    best = qref.log_joint(model, want_comp[:len(x)][alive], filled[:len(x)][alive])
    gap = np.abs(got - best) / np.maximum(1.0, np.abs(best))
    print('%s: largest distance from the restated maximum %.3g' % (tag, gap.max()))
    assert (gap <= BAR).all()
    if x.shape[1] <= 10:
        exact = qref.best_by_enumeration(model, x)[alive]
        gap = np.abs(got - exact) / np.maximum(1.0, np.abs(exact))
        print('%s: largest distance from the enumerated maximum %.3g' % (tag, gap.max()))
        assert (gap <= BAR).all()


# ---- seeded random models, every batch size ------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,k', CASES)
def test_marginals_match_the_restatement_and_enumeration(d, k):
    model, x = qref.random_model(d, k), qref.batch(d)
    dm, want = tables(model), wanted(model, x, (d, k))
    whole = None
    for b in reversed(qref.BATCHES):
        out, _ = run('marginals', dm, x[:b])
        part = {key: want[key][:b] for key in ('m64', 'm32')}
        check_marginals('marginals d=%d K=%d b=%d' % (d, k, b), model, x[:b], out, part)
        whole = out if whole is None else whole
        assert out.tobytes() == whole[:b].tobytes()                     # a row does not depend on its batch
    assert np.isnan(x[0]).all() and not np.isnan(x[1]).any() and same_bits(whole[1], x[1])
    # the all-NaN row: the prior marginals, the trees' priors under the mixture weights
    trees, logw = model
    prior = sum(np.exp(float(lw)) * qref.mref.tree_marginals(bfs, tree, params, x[:1])[0] for (bfs, tree, params), lw in zip(trees, logw))
    assert np.abs(whole[0] - prior / np.exp(logw.astype(np.float64)).sum()).max() <= BAR


@pytest.mark.parametrize('d,k', CASES)
def test_sampler_replays_the_restatement(d, k):
    model, x = qref.random_model(d, k), qref.batch(d)
    dm, want = tables(model), wanted(model, x, (d, k))
    whole = None
    for b in reversed(qref.BATCHES):
        out, comp = run('sample', dm, x[:b], 2024)
        check_replay(x[:b], out, comp, want)
        whole = (out, comp) if whole is None else whole
        assert out.tobytes() == whole[0][:b].tobytes() and comp.tobytes() == whole[1][:b].tobytes()
    out, comp = whole
    assert set(np.unique(out)) <= {0.0, 1.0} and comp.min() >= 0 and comp.max() < k
    again, other = run('sample', dm, x, 2024), run('sample', dm, x, 2025)
    assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == comp.tobytes()
    assert other[0].tobytes() != out.tobytes()
    tail = run('sample', dm, x[70:], 2024, row0=70)                     # in pieces, with row0 carried
    assert tail[0].tobytes() == out[70:].tobytes() and tail[1].tobytes() == comp[70:].tobytes()


@pytest.mark.parametrize('d,k', CASES)
def test_mpe_attains_the_maximum_by_value(d, k):
    model, x = qref.random_model(d, k), qref.batch(d)
    dm, want = tables(model), wanted(model, x, (d, k))
    whole = None
    for b in reversed(qref.BATCHES):
        out, comp = run('mpe', dm, x[:b])
        check_mpe('mpe d=%d K=%d b=%d' % (d, k, b), model, x[:b], out, comp, want)
        whole = (out, comp) if whole is None else whole
        assert out.tobytes() == whole[0][:b].tobytes() and comp.tobytes() == whole[1][:b].tobytes()


@pytest.mark.parametrize('d', qref.DS)
def test_one_component_is_the_tree_byte_for_byte(d):
    from deeprob.spn.structure.cltree import BinaryCLT
    model, x = qref.random_model(d, 1), qref.batch(d)
    (bfs, tree, params), = model[0]
    alone = BinaryCLT(list(range(d)), tree=tree.copy(), params=params.copy())
    dm = tables(model)
    assert run('marginals', dm, x)[0].tobytes() == alone.marginals(x).tobytes()
    out, comp = run('mpe', dm, x)
    assert out.tobytes() == alone.mpe(x).tobytes() and (comp == 0).all()


# ---- a fitted mixture, a zero weight, impossible rows --------------------------------------------------------------------------
def test_a_mixture_fitted_on_the_d16_fixture():
    from deeprob.hip import clt
    from deeprob.spn.structure import BinaryCLTMixture
    g = clt_ref.golden('d16')
    m = BinaryCLTMixture(list(range(16))).fit(g['x'], [[0, 1]] * 16, n_components=3, random_state=5)
    model = ([(np.asarray(c.bfs), np.asarray(c.tree), c.params) for c in m.components], np.log(m.weights))
    x = np.concatenate([g['q'][:198], np.full((1, 16), np.nan, np.float32), g['x'][:1]])
    dm, want = m._on_device(here()), wanted(model, x, 'd16')
    out, _ = run('marginals', dm, x)
    check_marginals('marginals fitted d16', model, x, out, want)
    sampled = run('sample', dm, x, 2024)
    check_replay(x, sampled[0], sampled[1], want)
    best = run('mpe', dm, x)
    check_mpe('mpe fitted d16', model, x, best[0], best[1], want)
    # the public methods: numpy and device tensors give the bytes of the binding
    xd = device(x)
    for given, back in ((x, lambda t: t), (xd, lambda t: t.cpu().numpy())):
        kind = np.ndarray if given is x else torch.Tensor
        got = m.marginals(given)
        assert isinstance(got, kind) and back(got).tobytes() == out.tobytes()
        got = m.sample(given, seed=2024)
        assert isinstance(got, kind) and back(got).tobytes() == sampled[0].tobytes()
        got, comp = m.sample(given, seed=2024, return_component=True)
        assert isinstance(comp, kind) and back(got).tobytes() == sampled[0].tobytes()
        assert back(comp).dtype == np.int32 and back(comp).shape == (200,) and back(comp).tobytes() == sampled[1].tobytes()
        got = m.mpe(given)
        assert isinstance(got, kind) and back(got).tobytes() == best[0].tobytes()
        got, comp = m.mpe(given, return_component=True)
        assert back(got).tobytes() == best[0].tobytes()
        assert back(comp).dtype == np.int32 and back(comp).shape == (200,) and back(comp).tobytes() == best[1].tobytes()
    assert m.sample(xd).is_cuda and clt.MIXQ_ABI_VERSION == 6


def test_unseeded_sampling_draws_its_seed_from_numpy():
    m = public(10, 3)
    q = np.full((64, 10), np.nan, np.float32)
    np.random.seed(3)
    first = m.sample(q)
    np.random.seed(3)
    assert m.sample(q).tobytes() == first.tobytes() and set(np.unique(first)) <= {0.0, 1.0}
    assert m.sample(q).tobytes() != first.tobytes()


def test_a_component_of_weight_zero_takes_no_part():
    model, x = qref.zero_weight_model(), qref.batch(10)
    dm, want = tables(model), wanted(model, x, 'zero weight')
    out, _ = run('marginals', dm, x)
    check_marginals('marginals zero weight', model, x, out, want)
    out, comp = run('sample', dm, x, 2024)
    check_replay(x, out, comp, want)
    assert (comp != 1).all()
    out, comp = run('mpe', dm, x)
    check_mpe('mpe zero weight', model, x, out, comp, want)
    assert (comp != 1).all()
    # every weight zero: no row can be answered
    trees, logw = model
    nothing = (trees, np.full(3, -np.inf, np.float32))
    dm = tables(nothing)
    out, _ = run('marginals', dm, x)
    assert np.array_equal(np.isnan(out), np.isnan(x)) and same_bits(out[~np.isnan(x)], x[~np.isnan(x)])
    for what in ('sample', 'mpe'):
        out, comp = run(what, dm, x, 7)
        assert same_bits(out, x) and (comp == -1).all()


def test_impossible_rows_keep_their_nan():
    model, x = qref.impossible_model(), qref.impossible_rows()
    dm, want = tables(model), wanted(model, x, 'impossible')
    out, _ = run('marginals', dm, x)
    check_marginals('marginals impossible', model, x, out, want)
    dead = np.array([True, True, False, False, False, True, False])
    assert np.array_equal(np.isnan(out), np.isnan(x) & dead[:, None])    # NaN in exactly their NaN entries
    out, comp = run('sample', dm, x, 2024)
    check_replay(x, out, comp, want)
    assert same_bits(out[dead], x[dead]) and (comp[dead] == -1).all() and (comp[~dead] >= 0).all()
    assert not np.isnan(out[~dead]).any() and comp[3] == 0 and comp[6] == 0
    out, comp = run('mpe', dm, x)
    check_mpe('mpe impossible', model, x, out, comp, want)
    assert comp[3] == 0 and comp[6] == 0


# ---- the sampler, its distribution ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', range(3))
def test_sampler_draws_from_the_posterior_by_enumeration(pattern):
    model = qref.random_model(5, 3)
    row = np.asarray(PATTERNS_D5[pattern], np.float32)
    x = np.tile(row, (N_DRAWS, 1))
    out, comp = run('sample', tables(model), x, 2024)
    obs = ~np.isnan(row)
    assert same_bits(out[:, obs], x[:, obs]) and set(np.unique(out)) <= {0.0, 1.0} and comp.min() >= 0 and comp.max() < 3
    p = qref.joint_posterior(model, row)                                # [K, 2^D]
    index = (out.astype(np.int64) << np.arange(5)).sum(axis=1)

    def worst(counts, prob):
        support = prob > 0
        assert counts[~support].sum() == 0                              # no mass outside the support
        se = np.sqrt(prob[support] * (1.0 - prob[support]) / N_DRAWS)
        return float(np.max(np.abs(counts[support] / N_DRAWS - prob[support]) / np.maximum(se, 1e-300)))

    by_row = worst(np.bincount(index, minlength=32).astype(np.float64), p.sum(axis=0))
    by_comp = worst(np.bincount(comp, minlength=3).astype(np.float64), p.sum(axis=1))
    by_pair = worst(np.bincount(comp * 32 + index, minlength=96).astype(np.float64), p.reshape(-1))
    print('pattern %d: worst deviation %.2f s.e. over completions, %.2f over components, %.2f over pairs' % (
        pattern, by_row, by_comp, by_pair))
    assert by_row <= 4.0 and by_comp <= 4.0


# ---- the other paths -----------------------------------------------------------------------------------------------------------
def test_the_circuit_of_to_pc_gives_the_same_marginals():
    from deeprob.spn.algorithms.moments import expectation
    m, x = public(10, 3), qref.batch(10)
    got, circuit = m.marginals(x), np.asarray(expectation(m.to_pc(), x))
    holes = np.isnan(x)
    assert np.abs(got[holes] - circuit[holes]).max() <= BAR


def test_a_long_batch_in_pieces_gives_the_same_bytes(monkeypatch):
    from deeprob.hip import clt
    model = qref.random_model(10, 3)
    x = np.concatenate([qref.batch(10, n=700, seed=s) for s in (1, 2, 3)])
    dm = tables(model)
    whole = [run(what, dm, x, 11) for what in ('marginals', 'sample', 'mpe')]
    monkeypatch.setattr(clt, 'WORK_FLOATS', 0)
    assert clt.query_rows(10) == 1024 < len(x)
    for what, (out, comp) in zip(('marginals', 'sample', 'mpe'), whole):
        again = run(what, dm, x, 11)
        assert again[0].tobytes() == out.tobytes() and (comp is None or again[1].tobytes() == comp.tobytes())


def test_scratch_is_exactly_what_the_header_states():
    """The entry points called with ``work`` of the header's size and not a byte more, between guard bands."""
    from deeprob.hip import clt
    lib = clt.load_library()
    model, x = qref.random_model(33, 3), qref.batch(33, n=65)
    dm, xd = tables(model), device(x)
    b, d, k = 65, 33, 3
    assert clt.mixture_query_row_bytes(dm, 'marginals') == 16 * d + 8 * k and clt.mixture_query_row_bytes(dm, 'mpe') == 8 * d + 8 * k
    want = [run(what, dm, x, 5)[0] for what in ('marginals', 'sample', 'mpe')]
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, dm._buf)
            codes = clt.pack_query(xd)
            outs = [torch.empty((b, d), dtype=torch.float32, device=xd.device) for _ in range(3)]
            big = torch.empty(b * (16 * d + 8 * k) // 8, dtype=torch.float64, device=xd.device)
            small = [torch.empty(b * (8 * d + 8 * k) // 8, dtype=torch.float64, device=xd.device) for _ in range(2)]
            head = (xd.data_ptr(), codes.data_ptr(), b, d, k) + dm.pointers()
            clt.call(lib.dpc_mixq_marginals, *head, big.data_ptr(), outs[0].data_ptr(), None)
            clt.call(lib.dpc_mixq_sample, *head, 5, 0, small[0].data_ptr(), outs[1].data_ptr(), None, None)
            clt.call(lib.dpc_mixq_mpe, *head, small[1].data_ptr(), outs[2].data_ptr(), None, None)
            c.expect_written(*outs)
        for out, w in zip(outs, want):
            assert out.cpu().numpy().tobytes() == w.tobytes()

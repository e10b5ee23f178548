"""RatSpn.sample_conditional without a device: the restatement the GPU tests replay against (tests/ratspn_posterior_ref.py)
is itself checked against brute-force enumeration, its counter-based uniforms against integer arithmetic, and the argument
errors that are raised before anything reaches the device."""
import numpy as np
import pytest
import torch

from tests import ratspn_posterior_ref as ref


def test_restatement_draws_the_enumerated_posterior():
    """A BernoulliRatSpn small enough to enumerate (6 variables, 3 of them missing: 8 completions).  200 000 rows with
    distinct counters through the restatement, activations from the oracle's forward: the frequency of every completion
    within 5 standard errors of p(x) / sum p(x), computed in float64 from the oracle's forward on the 8 completed rows (the
    bar of tests/test_flat_spn_queries_gpu.py for sample frequencies; the seed is fixed, so the outcome is deterministic)."""
    model, row, full, post = ref.enumerable_case()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    acts = ref.host_activations(sd, row, ref.ENUM_KW['rg_depth'])
    n = ref.ENUM_ROWS
    samples, _, _, _ = ref.posterior_sample(acts, model._topdown_logw(), model._topdown_src(), model._leaf_params(),
                                            row.expand(n, -1), None, ref.ENUM_SEED)
    assert torch.equal(samples[:, [0, 2, 5]], row[:, [0, 2, 5]].expand(n, -1)) and not torch.isnan(samples).any()
    freq = ref.completion_counts(samples, full) / n
    se = np.sqrt(post * (1.0 - post) / n)
    assert post.min() > 1e-3 and abs(post.sum() - 1.0) < 1e-12        # (a posterior worth testing: no empty cell)
    assert (np.abs(freq - post) <= 5.0 * se).all(), (freq, post, se)
    # the weights alone are another distribution: the same draws without the evidence miss the bar by far
    blind = [torch.zeros_like(a) for a in acts]
    prior, _, _, _ = ref.posterior_sample(blind, model._topdown_logw(), model._topdown_src(), model._leaf_params(),
                                          row.expand(n, -1), None, ref.ENUM_SEED)
    assert (np.abs(ref.completion_counts(prior, full) / n - post) > 5.0 * se).any()


def _splitmix_uniform(seed: int, ctr: int) -> float:
    mask = (1 << 64) - 1
    z = (seed + ctr * 0x9E3779B97F4A7C15) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def test_counter_uniforms_are_splitmix64():
    """u(ctr) = (splitmix64(seed + ctr * golden) >> 40) / 2^24 (the header of csrc/ratspn_topdown.hip), recomputed in Python
    integers; and the counter of a slot: row * (2^depth + 2 D) + slot."""
    pairs = [(0, 0), (0, 1), (987654321, 1), (987654321, 300 * (4 + 2 * 15) + 4 + 2 * 7 + 1), (2 ** 62 - 1, 2 ** 40 + 12345),
             (2 ** 64 - 1, 2 ** 63)]
    for seed, ctr in pairs:
        got = ref.counter_uniform(seed, np.array([ctr], dtype=np.uint64))
        assert got.dtype == np.float32 and 0.0 <= got[0] < 1.0
        assert float(got[0]) == _splitmix_uniform(seed, ctr), (seed, ctr)
    # splitmix64's published first output for state 0 is 0xE220A8397B1DCDAF: seed 0, counter 1 is that state
    assert _splitmix_uniform(0, 1) == (0xE220A8397B1DCDAF >> 40) / 16777216.0


def test_argument_errors_need_no_device():
    """A CPU tensor raises (no silent fallback, as for mpe); a user-defined leaf layer and training-mode dropout are not
    built and say so."""
    from deeprob.hip import HipError
    from deeprob.spn.models import GaussianRatSpn, RatSpn
    from deeprob.spn.layers.ratspn import RegionGraphLayer
    model = GaussianRatSpn(8, rg_depth=1, rg_repetitions=2, rg_batch=2, random_state=1).eval()
    with pytest.raises((HipError, TypeError, ValueError, RuntimeError)):
        model.sample_conditional(torch.randn(3, 8))

    class MyLeaf(RegionGraphLayer):
        """A leaf family of the user's: neither of the two whose parameters the kernel reads."""
        def _leaf_forward(self, x):
            raise AssertionError('sample_conditional must refuse before it evaluates anything')

        _leaf_forward_dropout = distribution_mode = _leaf_forward

    custom = RatSpn(8, MyLeaf, rg_depth=1, rg_repetitions=2, rg_batch=2, random_state=1).eval()
    with pytest.raises(NotImplementedError, match='leaf layer'):
        custom.sample_conditional(torch.randn(3, 8))

    for kw in (dict(in_dropout=0.2), dict(sum_dropout=0.2)):
        drop = GaussianRatSpn(8, rg_depth=2, rg_repetitions=2, rg_batch=2, rg_sum=2, random_state=1, **kw).train()
        with pytest.raises(NotImplementedError, match='dropout'):
            drop.sample_conditional(torch.randn(3, 8))
        with pytest.raises((HipError, TypeError, ValueError, RuntimeError)) as info:
            drop.eval().sample_conditional(torch.randn(3, 8))
        assert not isinstance(info.value, NotImplementedError)

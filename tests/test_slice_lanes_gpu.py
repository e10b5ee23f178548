"""The RAT-SPN slice mapping on a share of the compute units (csrc/ratspn_gemm_slice.hip, include/deeprob_slice.h): a launch
told that it runs beside others takes fewer work-groups and walks more blocks with each.  Which block a work-group takes
changes nothing in a sample's arithmetic, so the per-sample log-likelihoods are held to BIT identity with the whole-chip
launch; the fp64 {sum, count} differs in the order of its atomics only (1e-9 relative; 8192 addends of magnitude ~1e3 in
fp64 are good for ~1e-12)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 784
BATCHES = [33, 32 * 13, 32 * 86 + 7, 32 * 170 + 1, 8192]
LANES = [1, 2, 3, 8]


@pytest.fixture
def slice_everywhere():
    """Every batch size on the slice mapping (its threshold lowered and restored); lane override off."""
    from deeprob.hip import load_library, slice as sl
    lib = load_library()
    prev = lib.dpk_ratspn_slice_batch_min(0)
    prev_lanes = sl.lanes(0)
    yield sl
    sl.lanes(prev_lanes)
    lib.dpk_ratspn_slice_batch_min(prev)


def make_model(reps=8, seed=42):
    from deeprob.spn.models import GaussianRatSpn
    torch.manual_seed(0)
    return GaussianRatSpn(D, rg_depth=2, rg_repetitions=reps, rg_batch=2, rg_sum=2, random_state=seed).eval().cuda()


def batch(B, seed=1):
    return torch.randn(B, D, generator=torch.Generator().manual_seed(seed)).cuda()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run(plan):
    """(per-sample LLs, fp64 sum, count) of one run of a bound forward."""
    acc = torch.zeros(17, dtype=torch.float64, device='cuda')
    ll = plan.run(acc).clone()
    return ll, acc[:16].sum().item(), acc[16].item()


def bits(t):
    return t.contiguous().view(torch.int32)


def check_grid(sl, B, lanes):
    nt = -(-B // 32)
    assert sl.last_lanes() == lanes
    g = sl.last_grid()
    if lanes == 1:
        assert g == min(nt, cus())
    else:   # (its share, or the work-groups an in-launch table check needs: 13 for eight repetitions, fewer for five)
        assert g in (sl.grid(nt, cus(), lanes, 0), sl.grid(nt, cus(), lanes, 13)) or g <= 13


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('frozen', [True, False], ids=['frozen', 'default'])
@pytest.mark.parametrize('reps', [8, 5])
def test_bit_identity_over_lane_counts(slice_everywhere, reps, frozen, B):
    sl = slice_everywhere
    model, x = make_model(reps), batch(B)
    with torch.no_grad():
        ref = None
        for lanes in LANES:
            plan = model.fused_plan(x, static_params=frozen, lanes=lanes)
            assert plan is not None
            ll, s, n = run(plan)
            check_grid(sl, B, lanes)
            if ref is None:
                ref = (ll, s, n)
                assert torch.isfinite(ll).all() and n == B
                continue
            assert torch.equal(ll, ref[0]), (lanes, B)
            assert n == ref[2] == B
            assert abs(s - ref[1]) <= 1e-9 * abs(ref[1]), (lanes, B, s, ref[1])


def test_stale_tables_under_a_share(slice_everywhere):
    """A parameter written through .data (no version bump) in front of a default-mode launch on three lanes: the launch's own
    table check finds it, every block goes through the table-free route and the tables are rebuilt in place.  The table-free
    route is the exact fp32 evaluation, the clean launch the split-f16 one: 1e-5 relative between them (the bar every
    mapping is held to against the oracle); the NEXT launch runs on rebuilt tables: bit-equal to a freshly built model's."""
    sl = slice_everywhere
    B = 32 * 86 + 7
    x = batch(B)
    with torch.no_grad():
        model = make_model()
        plan = model.fused_plan(x, lanes=3)
        run(plan)
        model.base_layer.loc.data.add_(0.05)
        model.root_layer.weight.data.mul_(0.5)
        stale, s_stale, n_stale = run(plan)
        check_grid(sl, B, 3)
        again, s_again, _ = run(plan)
        fresh_model = make_model()
        fresh_model.base_layer.loc.add_(0.05)
        fresh_model.root_layer.weight.mul_(0.5)
        fresh, s_fresh, _ = run(fresh_model.fused_plan(x, lanes=1))
    rel = ((stale - fresh).abs() / fresh.abs().clamp_min(1.0)).max().item()
    print('stale launch against a fresh model: max rel err {:.3e}'.format(rel))
    assert rel <= 1e-5 and n_stale == B
    assert abs(s_stale - stale.double().sum().item()) <= 1e-9 * abs(s_fresh)
    assert torch.equal(again, fresh)
    assert abs(s_again - s_fresh) <= 1e-9 * abs(s_fresh)


def test_exact_route_under_a_share(slice_everywhere):
    """One +inf and one NaN sample in one block: the block leaves the fast path and is evaluated exactly after the stream.
    (The first launch of a workspace: later ones would take the mapping built for marginalised evidence.)"""
    sl = slice_everywhere
    B = 32 * 86 + 7
    x = batch(B)
    x[32 * 40 + 3, 17] = float('inf')
    x[32 * 40 + 9, 100:140] = float('nan')
    outs = []
    with torch.no_grad():
        for lanes in (1, 3):
            plan = make_model().fused_plan(x, static_params=True, lanes=lanes)     # (its constructor launches once)
            check_grid(sl, B, lanes)
            outs.append(plan.out.clone())
    assert torch.isfinite(outs[0][32 * 40 + 9]).all()      # (marginalised: a likelihood like any other)
    assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_auto_mode(slice_everywhere):
    """Nothing stated, eager launches: a launch that finds every other stream idle takes the whole chip (deterministic after
    a synchronize); launches alternating between two streams and two workspaces take the whole chip or the half share, and
    their log-likelihoods are those of the single-stream launches, bit for bit."""
    from deeprob.parallel import workspace_replica
    sl = slice_everywhere
    B = 8192
    nt = B // 32
    full, half = min(nt, cus()), sl.grid(nt, cus(), 2, 0)
    model = make_model()
    models = [model, workspace_replica(model)]
    xs = [batch(B, seed=5), batch(B, seed=6)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with torch.no_grad():
        sl.lanes(1)
        ref = [run(model.fused_plan(xs[k]))[0] for k in range(2)]
        sl.lanes(0)
        plans = [models[k].fused_plan(xs[k]) for k in range(2)]
        torch.cuda.synchronize()
        outs, grids = [], []
        for i in range(8):
            with torch.cuda.stream(streams[i % 2]):
                outs.append(plans[i % 2].run().clone())
            grids.append(sl.last_grid())
        torch.cuda.synchronize()
        print('auto mode grids over eight alternating steps:', grids)
        assert grids[0] == full and set(grids) <= {full, half}
        for i, o in enumerate(outs):
            assert torch.equal(o, ref[i % 2]), i
        # every stream idle: a lane that was sharing looks again within DPS_AUTO_RECHECK launches, finds its peer idle and
        # takes the whole chip from then on
        seen = []
        for _ in range(sl.DPS_AUTO_RECHECK + 1):
            with torch.cuda.stream(streams[0]):
                plans[0].run()
            seen.append(sl.last_grid())
            torch.cuda.synchronize()
        print('after a synchronize:', seen)
        back = seen.index(full)
        assert back < sl.DPS_AUTO_RECHECK and set(seen[:back]) <= {half} and set(seen[back:]) == {full}
        assert sl.last_lanes() == 1


def test_graphed_window_chains_state_their_lanes(slice_everywhere):
    from deeprob.parallel import ShardedLogLikelihood, GraphedEvaluationWindow
    model = make_model()
    xs = [batch(B, seed=10 + i) for i, B in enumerate([32 * 13, 32 * 86 + 7, 33, 32 * 170 + 1])]
    with torch.no_grad():
        one = GraphedEvaluationWindow(ShardedLogLikelihood(model, static_inputs=True), xs, chains=1)
        want = one.replay()
        one.close()
        win = GraphedEvaluationWindow(ShardedLogLikelihood(model, static_inputs=True), xs, chains=3)
        assert [lane.lanes for lane in win.lanes] == [2, 2, 2]      # (two co-resident launches, the third queued: parallel.py)
        for _ in range(2):
            got = win.replay()
            for g, w in zip(got, want):
                assert abs(g - w) <= 1e-9 * abs(w), (got, want)
        win.close()

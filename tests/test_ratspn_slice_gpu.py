"""The RAT-SPN slice mapping (csrc/ratspn_gemm_slice.hip) across its model envelope against the float64 oracle: 5 to 8
repetitions (the spare slots of phase 2), 1 to 64 classes (root weights of the classes 1 and up, the fp64 {sum, count}), the
walk of a work-group over several blocks with exact-route blocks at its first, a middle and its last position and at every
position (the verdict read one iteration late, exact blocks dealt out eight at a time), two launches in one call, and the
model's own verdicts (eligibility bits, vanished nodes) at 5 and 7 repetitions.

The cases, their by-construction assertions (which block is on the fast path) and the references are
tests/ratspn_slice_cases.py's.  The bar is the project's: 1e-5 relative per sample and class against float64, the fp64 sum
within 1e-9 of the sum of the returned values.  Every measured error is recorded through tests/util.py::report_measured with the float32
oracle's own distance from float64 beside it.  Every case runs frozen (static_params=True: no table check) and in default
mode (the launch's own table check on its eighth waves, or the stand-alone check launch where it cannot carry one)."""
import pytest
import torch

from tests import ratspn_slice_cases as sc
from tests.util import rel_err, report_measured

pytestmark = pytest.mark.gpu

MODES = [True, False]
MODE_IDS = ['frozen', 'default']


@pytest.fixture
def sl():
    """Every batch size on the slice mapping (its threshold lowered and restored); process-wide lane override off."""
    from deeprob.hip import load_library, slice as sl
    lib = load_library()
    prev = lib.dpk_ratspn_slice_batch_min(0)
    prev_lanes = sl.lanes(0)
    yield sl
    sl.lanes(prev_lanes)
    lib.dpk_ratspn_slice_batch_min(prev)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch(model, x, frozen, lanes):
    """(first launch of a fresh plan -- its constructor's, which builds the tables --, a later launch, its fp64 sum, count)."""
    with torch.no_grad():
        plan = model.fused_plan(x, static_params=frozen, lanes=lanes)
        assert plan is not None
        first = plan.out.clone()
        acc = torch.zeros(17, dtype=torch.float64, device='cuda')
        ll = plan.run(acc).clone()
    return first, ll, acc[:16].sum().item(), acc[16].item()


def small_mapping(model, x):
    """(log-likelihoods, fp64 sum, count) of the same model and batch on the small-batch mapping (slice mapping off)."""
    from deeprob.hip import load_library
    lib = load_library()
    prev = lib.dpk_ratspn_slice_batch_min(-1)
    try:
        with torch.no_grad():
            plan = model.fused_plan(x, static_params=True)
            acc = torch.zeros(17, dtype=torch.float64, device='cuda')
            ll = plan.run(acc).clone()
        return ll, acc[:16].sum().item(), acc[16].item()
    finally:
        lib.dpk_ratspn_slice_batch_min(prev)


def check_values(tag, case, ll):
    err = rel_err(case.got_rows(ll), case.want)
    report_measured('test_ratspn_slice_gpu %s vs fp64' % tag, err, sc.LL_TOL, '(fp32 oracle vs fp64: %.2e)' % case.noise)
    print('%s: rel err %.3e (fp32 oracle %.2e)' % (tag, err, case.noise))
    assert err <= sc.LL_TOL, (tag, err)


def check_sum(tag, ll, s, n, count):
    tot = ll.double().sum().item()
    rel = abs(s - tot) / abs(tot)
    report_measured('test_ratspn_slice_gpu %s fp64 sum vs sum of the values' % tag, rel, sc.SUM_TOL)
    assert n == count, (tag, n, count)
    assert rel <= sc.SUM_TOL, (tag, s, tot)


def check_launch(sl, case, lanes, frozen):
    assert sl.last_lanes() == lanes
    assert sl.last_grid() == sc.expected_grid(sl, case.B, cus(), lanes, case.R, case.C, frozen), sl.last_grid()


# ---- 1: the envelope on the fast path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('frozen', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('B', [33, 257, 32 * 19 + 5])
@pytest.mark.parametrize('name', sc.ENVELOPE)
def test_envelope_fast_path(sl, name, B, frozen):
    """Every (repetitions, classes) of the envelope with every row on the fast path.  The largest batch runs on
    DPS_LANES_MAX lanes, so that work-groups walk a second block (except under the in-launch check of the 64-class model,
    whose 20 table work-groups are the grid); the others on 1 lane (frozen) and 2 (default), so that the lane count the
    library reports changes from launch to launch.  The count is the small-batch mapping's for the same model and batch."""
    case = sc.envelope_case(name, B)
    lanes = sl.DPS_LANES_MAX if B > 512 else (1 if frozen else 2)
    model, x = sc.make_model(name).cuda(), case.x.cuda()
    first, ll, s, n = launch(model, x, frozen, lanes)
    check_launch(sl, case, lanes, frozen)
    tag = 'envelope[%s, B=%d, %s]' % (name, B, 'frozen' if frozen else 'default')
    check_values(tag + ' first launch', case, first)
    check_values(tag, case, ll)
    _, _, n_small = small_mapping(model, x)
    assert n_small == B * case.C
    check_sum(tag, ll, s, n, n_small)


# ---- 2: positions on a work-group's walk -------------------------------------------------------------------------------------
@pytest.mark.parametrize('frozen', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('trigger', sc.TRIGGERS)
@pytest.mark.parametrize('name', sc.WALK)
def test_walk_positions(sl, name, trigger, frozen):
    """Every work-group walks ten blocks on DPS_LANES_MAX lanes; one sample leaves the fast path in the first block of one
    work-group, in a middle block of another, in the last block of a third and in every block of a fourth.  The fp64 sum must
    be the sum of the returned values: the verdict that is read one iteration late neither drops a block nor counts it
    twice.  (Under the +inf trigger the exact rows are -3.4e38 and the sum speaks for the exact blocks only; under the 200.0
    trigger every block weighs 1e-2 of it.)"""
    R, C, _ = sc.MODELS[name]
    lanes = sl.DPS_LANES_MAX
    G = sc.lane_share(sl, cus(), lanes, 0 if frozen else sc.prep_blocks(R, C))
    case = sc.walk_case(name, trigger, G)
    model, x = sc.make_model(name).cuda(), case.x.cuda()
    first, ll, s, n = launch(model, x, frozen, lanes)
    assert sl.last_lanes() == lanes and sl.last_grid() == G == sc.expected_grid(sl, case.B, cus(), lanes, R, C, frozen)
    tag = 'walk[%s, %s, %s]' % (name, trigger, 'frozen' if frozen else 'default')
    check_values(tag + ' first launch', case, first)
    check_values(tag, case, ll)
    check_sum(tag, ll, s, n, case.B * C)
    assert torch.isfinite(ll).all()


# ---- 3: the model's verdicts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frozen', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('kind', sc.VERDICT_KINDS)
@pytest.mark.parametrize('name', ['r5_c1', 'r7_c10'])
def test_model_verdicts(sl, name, kind, frozen):
    """Clean evidence under a model the fast path must decline, at 5 and 7 repetitions: the eligibility bit of the last
    repetition (the one the spare slots copy) or of repetition 0 is off, or the sum nodes' and the root's inputs vanish."""
    case = sc.verdict_case(name, kind)
    lanes = 1 if frozen else 3
    model, x = sc.make_model(name, kind).cuda(), case.x.cuda()
    first, ll, s, n = launch(model, x, frozen, lanes)
    check_launch(sl, case, lanes, frozen)
    tag = 'verdict[%s, %s, %s]' % (name, kind, 'frozen' if frozen else 'default')
    check_values(tag + ' first launch', case, first)
    check_values(tag, case, ll)
    check_sum(tag, ll, s, n, case.B * case.C)


# ---- 4: NaN evidence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frozen', MODES, ids=MODE_IDS)
def test_nan_evidence(sl, frozen):
    """One all-NaN row and one partly marginalised row in a clean batch, six repetitions, three classes.  The first launch of
    a fresh plan runs on the slice mapping: the two blocks go exact and raise the hint; the second launch runs on whichever
    mapping the hint sends it to.  Both against float64; the all-NaN row is 0 within 1e-5 in both."""
    case = sc.nan_case()
    lanes = 2
    model, x = sc.make_model(case.name).cuda(), case.x.cuda()
    first, ll, s, n = launch(model, x, frozen, lanes)
    tag = 'nan[%s, %s]' % (case.name, 'frozen' if frozen else 'default')
    for which, out in (('first launch', first), ('second launch', ll)):
        check_values('%s %s' % (tag, which), case, out)
        assert out[sc.NAN_ROW].abs().max().item() <= 1e-5
    check_sum(tag, ll, s, n, case.B * case.C)


def test_nan_evidence_first_launch_is_a_slice_launch(sl):
    case = sc.nan_case()
    model, x = sc.make_model(case.name).cuda(), case.x.cuda()
    with torch.no_grad():
        plan = model.fused_plan(x, static_params=True, lanes=4)
    assert plan is not None and sl.last_lanes() == 4 and sl.last_grid() == sl.grid(sc.cdiv(case.B, 32), cus(), 4, 0)


# ---- 5: two launches per call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r8_c1', 'r5_c3'])
def test_two_launches_per_call(sl, name):
    """B = 64 * 32 * (a lane's share on DPS_LANES_MAX lanes) + 32 * 3 + 5: gemm_slice_launch loops, moving x and out; the
    in-launch table check is off there, default mode takes the stand-alone check launch.  One exact-route sample in the last
    block of the first launch, one in the first block of the second."""
    lanes = sl.DPS_LANES_MAX
    share = sc.lane_share(sl, cus(), lanes)
    B, per_launch, _ = sc.two_launch_layout(share)
    need = 5 * B * sc.D * 4                     # x, and the float64 temporaries of the case builder's audit of it
    if torch.cuda.mem_get_info()[0] < need + (1 << 28):
        pytest.skip('the device cannot hold %d MB of buffers' % (need >> 20))
    case = sc.two_launch_case(name, share, torch.device('cuda'))
    for frozen in MODES:
        model = sc.make_model(name).cuda()
        first, ll, s, n = launch(model, case.x, frozen, lanes)
        # (the second launch's grid: four blocks, one work-group each)
        assert sl.last_lanes() == lanes and sl.last_grid() == 4 == sc.expected_grid(sl, B, cus(), lanes, case.R, case.C, frozen)
        tag = 'two_launches[%s, %s]' % (name, 'frozen' if frozen else 'default')
        check_values(tag + ' first call', case, first)
        check_values(tag, case, ll)
        check_sum(tag, ll, s, n, B * case.C)
        assert torch.isfinite(ll).all()


# ---- 6: agreement with the other mapping ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sc.ENVELOPE)
def test_agreement_with_the_small_batch_mapping(sl, name):
    case = sc.envelope_case(name, 257)
    model, x = sc.make_model(name).cuda(), case.x.cuda()
    _, ll, s, n = launch(model, x, True, 1)
    check_launch(sl, case, 1, True)
    ll_small, s_small, n_small = small_mapping(model, x)
    err = rel_err(ll.cpu().numpy(), ll_small.cpu().numpy())
    report_measured('test_ratspn_slice_gpu mappings[%s] slice vs small-batch' % name, err, sc.MAP_TOL)
    assert err <= sc.MAP_TOL and n == n_small
    assert abs(s - s_small) <= sc.MAP_TOL * abs(s_small)


# ---- 7: the envelope's borders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(rg_repetitions=4), dict(rg_repetitions=9), dict(in_features=780), dict(rg_batch=4),
                                dict(rg_sum=4)], ids=['R4', 'R9', 'D780', 'I4', 'S4'])
def test_neighbours_stay_off_the_slice_mapping(sl, kw):
    """gemm_slice_shape_ok says no to the nearest neighbours of the envelope, with the threshold at 0: a launch of theirs
    leaves the lane count of the last SLICE launch where a marker launch put it -- and a case model's moves it.  Their
    results are held to the same bar on whichever mapping takes them."""
    from deeprob.spn.models import GaussianRatSpn
    marker = sc.envelope_case('r5_c1', 33)
    with torch.no_grad():
        assert sc.make_model('r5_c1').cuda().fused_plan(marker.x.cuda(), static_params=True, lanes=3) is not None
    assert sl.last_lanes() == 3
    base = dict(in_features=sc.D, rg_depth=2, rg_batch=2, rg_sum=2, rg_repetitions=8, random_state=7)
    base.update(kw)
    torch.manual_seed(7)
    model = GaussianRatSpn(**base).eval()
    _, sd64 = sc.state_dicts(model)
    x = 1.2 * torch.randn(33, base['in_features'], generator=torch.Generator().manual_seed(8))
    want = sc.oracle_rows(sd64, x)
    with torch.no_grad():
        plan = model.cuda().fused_plan(x.cuda(), static_params=True, lanes=5)
        assert plan is not None
        got = plan.out.double().cpu().numpy()
    assert sl.last_lanes() == 3
    assert rel_err(got, want) <= sc.LL_TOL
    with torch.no_grad():
        assert sc.make_model('r8_c1').cuda().fused_plan(marker.x.cuda(), static_params=True, lanes=5) is not None
    assert sl.last_lanes() == 5

"""The cases of the RAT-SPN slice-mapping tests (tests/ratspn_slice_cases.py), checked where no device is needed: the case
builders' own by-construction assertions (which blocks are on the fast path, which leave it and why), the placement of the
exact-route samples computed from the library's grid choice, the float32 oracle's distance from the float64 one, the
sensitivity of the chosen parameters to the bugs the device tests are after, and the envelope the host side admits."""
import numpy as np
import pytest

from tests import ratspn_slice_cases as sc
from tests.util import report_measured

#: compute-unit counts of the placement checks: hypothetical devices (the device tests ask the device)
DEVICES = (256, 304, 120)


def slice_lib():
    from deeprob.hip import slice as sl
    return sl


def note(case, tag):
    report_measured('slice cases (host) %s float32 oracle vs float64' % tag, case.noise, sc.NOISE_TOL)
    assert case.noise <= sc.NOISE_TOL, (tag, case.noise)


@pytest.mark.parametrize('B', [33, 257, 32 * 19 + 5])
@pytest.mark.parametrize('name', sc.ENVELOPE)
def test_envelope_cases_are_on_the_fast_path(name, B):
    case = sc.envelope_case(name, B)          # (asserts the four conditions in float64)
    assert case.want.shape == (B, case.C) and case.exact == []
    note(case, 'envelope[%s, B=%d]' % (name, B))


@pytest.mark.parametrize('name', sorted(sc.MODELS))
def test_sensitivity(name):
    """The parameters make the expected bugs visible in the float64 reference itself, on the 257-row batch.
    q_twice and class_shift: at least 100 bars on at least half of the rows.  dup_last cannot reach that for ANY parameters:
    a repetition counted twice moves a log-likelihood by log(1 + its posterior) <= log 2 = 0.69, and |ll| >= 784 * 0.919 =
    720 under unit scales (2000 here), so 0.69 / 2000 = 35 bars at the most.  It is held to 10 bars (a posterior of the last
    repetition of 0.22) on at least a quarter of the rows -- the seeds are chosen for it (ratspn_slice_cases.MODELS); the
    device tests assert the maximum over the rows, so one such row fails them."""
    case = sc.envelope_case(name, 257)
    bad = sc.broken_variants(case.audit, case.x)
    bar = sc.LL_TOL
    for key, bars, share in (('q_twice', 100, 0.5), ('class_shift', 100, 0.5), ('dup_last', 10, 0.25)):
        if bad[key] is None:
            assert key == 'class_shift' and case.C == 1
            continue
        r = sc.row_rel(bad[key], case.want)
        frac = float((r >= bars * bar).mean())
        print('%s %s: %.2f of the rows at >= %d bars, max %.1f bars' % (name, key, frac, bars, r.max() / bar))
        assert frac >= share, (name, key, frac)


@pytest.mark.parametrize('cus', DEVICES)
def test_walk_placement(cus):
    """On DPS_LANES_MAX lanes a launch of ten blocks per work-group takes exactly the lane's share, frozen or with the widest
    in-launch table check of the walk models, and the four positions are where walk_layout says: block b is the (b // G)-th
    of work-group b % G."""
    sl = slice_lib()
    for name in sc.WALK:
        R, C, _ = sc.MODELS[name]
        for frozen in (True, False):
            np_ = 0 if frozen else sc.prep_blocks(R, C)
            G = sc.lane_share(sl, cus, sl.DPS_LANES_MAX, np_)
            B, lay = sc.walk_layout(G)
            nt = sc.cdiv(B, 32)
            assert nt == sc.WALK_BLOCKS * G and B % 32 == 5
            assert sl.grid(nt, cus, sl.DPS_LANES_MAX, np_) == G == sc.expected_grid(sl, B, cus, sl.DPS_LANES_MAX, R, C, frozen)
            assert [b // G for b in lay['first'][1]] == [0] and [b // G for b in lay['last'][1]] == [sc.WALK_BLOCKS - 1]
            assert 0 < lay['middle'][1][0] // G < sc.WALK_BLOCKS - 1
            assert [b // G for b in lay['every'][1]] == list(range(sc.WALK_BLOCKS)) and len(lay['every'][1]) > 8


@pytest.mark.parametrize('trigger', sc.TRIGGERS)
@pytest.mark.parametrize('name', sc.WALK)
def test_walk_cases(name, trigger):
    sl = slice_lib()
    G = sc.lane_share(sl, DEVICES[0], sl.DPS_LANES_MAX)
    case = sc.walk_case(name, trigger, G)     # (asserts which blocks break which condition, and that no other does)
    assert len(case.exact) == 13 and len(case.planted) == 13 and len(case.rows) >= 1024
    rows = set(case.rows.tolist())
    for b in case.exact:                      # every row of the affected blocks and of their neighbours
        for c in (b - 1, b, b + 1):
            assert all(r in rows for r in range(32 * c, min(32 * c + 32, case.B)))
    assert case.B - 1 in rows and 0 in rows
    note(case, 'walk[%s, %s]' % (name, trigger))


@pytest.mark.parametrize('kind', sc.VERDICT_KINDS)
@pytest.mark.parametrize('name', ['r5_c1', 'r7_c10'])
def test_verdict_cases(name, kind):
    case = sc.verdict_case(name, kind)        # (asserts the condition the model breaks, and that the evidence breaks none)
    assert case.exact is None
    note(case, 'verdict[%s, %s]' % (name, kind))


def test_nan_case():
    case = sc.nan_case()
    assert case.exact == [1, 3]
    note(case, 'nan[r6_c3]')


@pytest.mark.parametrize('cus', DEVICES)
def test_two_launch_placement(cus):
    """B = 64 * 32 * share + 32 * 3 + 5 is beyond what one launch covers: the first launch walks 64 blocks with every one of
    `share` work-groups, the second takes four blocks; neither can carry a table check of its own."""
    sl = slice_lib()
    L = sl.DPS_LANES_MAX
    share = sc.lane_share(sl, cus, L)
    B, per_launch, planted = sc.two_launch_layout(share)
    assert sl.grid(per_launch // 32, cus, L, 0) == share and sc.cdiv(per_launch // 32, share) == 64
    assert planted[0] // 32 == per_launch // 32 - 1 and planted[1] // 32 == per_launch // 32
    for name in ('r8_c1', 'r5_c3'):
        R, C, _ = sc.MODELS[name]
        if share >= sc.prep_blocks(R, C):     # (else the check's work-groups widen the launch: another device's layout)
            for frozen in (True, False):
                assert sc.expected_grid(sl, B, cus, L, R, C, frozen) == 4


def test_two_launch_case_on_the_host():
    import torch
    sl = slice_lib()
    share = sc.lane_share(sl, DEVICES[0], sl.DPS_LANES_MAX)
    case = sc.two_launch_case('r5_c3', share, torch.device('cpu'))
    assert len(case.exact) == 2 and case.exact[1] == case.exact[0] + 1
    note(case, 'two_launches[r5_c3]')


def test_the_envelope_is_admitted():
    """Every case model is inside the matrix-core route's envelope as the models ask for it (dpk_ratspn_forward_on_mfma with
    the unit-scale hint and a 16-byte aligned x), and outside it without the hint, with a misaligned x or with 65 classes;
    the slice threshold can be lowered to 0 and put back.  (Whether a shape inside that envelope takes the SLICE mapping --
    gemm_slice_shape_ok -- has no host-side query: tests/test_ratspn_slice_gpu.py::test_neighbours_stay_off_the_slice_mapping
    asks the launches.)"""
    from deeprob.hip import load_library, ops
    lib = load_library()
    for name, (R, C, _) in sc.MODELS.items():
        assert lib.dpk_ratspn_forward_on_mfma(0, sc.D, 2, R, 2, 2, C, 0, ops.DPK_FLAG_UNIT_SCALE) == 1, name
        assert lib.dpk_ratspn_forward_on_mfma(0, sc.D, 2, R, 2, 2, C, 0, 0) == 0
        assert lib.dpk_ratspn_forward_on_mfma(4, sc.D, 2, R, 2, 2, C, 0, ops.DPK_FLAG_UNIT_SCALE) == 0
        assert lib.dpk_ratspn_forward_on_mfma(0, sc.D, 2, R, 2, 2, 65, 0, ops.DPK_FLAG_UNIT_SCALE) == 0
        assert lib.dpk_ratspn_forward_on_mfma(0, sc.D, 3, R, 2, 2, C, 0, ops.DPK_FLAG_UNIT_SCALE) == 0
    prev = lib.dpk_ratspn_slice_batch_min(0)
    try:
        assert lib.dpk_ratspn_slice_batch_min(0) == 0
    finally:
        assert lib.dpk_ratspn_slice_batch_min(prev) == 0
    assert lib.dpk_ratspn_slice_batch_min(prev) == prev


def test_prep_blocks_of_the_headline_model():
    """tests/test_slice_lanes_gpu.py::check_grid: "13 for eight repetitions"."""
    assert sc.prep_blocks(8, 1) == 13 and sc.prep_blocks(5, 1) < 13

"""The RAT-SPN slice mapping (csrc/ratspn_gemm_slice.hip) across the envelope its host side admits -- 784 variables, depth 2,
two channels, two sums, 5 to 8 repetitions, 1 to 64 classes, any stated lane count -- as cases for the host and the device
tests: trained-like seeded models, evidence, the placement of exact-route samples on a work-group's walk, and the float64 /
float32 oracle references.  Everything here runs on the host except the evidence of the two-launch case, which is drawn on
the device it is handed.

Nothing in the library reports which route a block took, so every case states it BY CONSTRUCTION: a case builder asserts in
float64 that the blocks meant for the fast path hold every condition the kernel tests (bounded means, bounded sum of
squares, finite evidence, no vanished sum-node or root input) and that the blocks meant for the exact route break the one
they are meant to break.

A helper module (no tests in it)."""
import functools

import numpy as np
import torch

from oracle import ratspn_oracle as orc
from tests.util import rel_err

LL_TOL = 1e-5       # the project's bar: 1e-5 relative on fp32 log-likelihoods, per sample and class
SUM_TOL = 1e-9      # the fp64 {sum, count} against ll.double().sum() (tests/test_slice_lanes_gpu.py)
MAP_TOL = 1e-6      # between two mappings of the same arithmetic (tests/test_ratspn_gpu.py::test_full_size_properties)
NOISE_TOL = 1e-6    # the float32 oracle against the float64 one: measured 1.9e-7 .. 2.4e-7, a factor 10 inside LL_TOL

D = 784
MU_MAX = 5.5                      # the cases' means; the kernel's bound (common.h::kExpandBound) is 6
SUMSQ_BOUND = 36.0 * D            # the kernel's: "!(qtot <= kExpandBound * kExpandBound * (float)D)"
SUMSQ_MAX = 0.5 * SUMSQ_BOUND     # what fast-path evidence stays under
NODE_MIN = 1e-20                  # the kernel's "v < 1e-30f" with ten decades to spare
WALK_BLOCKS = 10
HUGE = 200.0                      # one entry: 40000 > 36 D = 28224, finite, raises no NaN hint

#: name -> (repetitions, classes, seed of the region graph and of the parameters).  The seeds are CHOSEN: with independent
#: means a repetition's likelihood carries a fixed -1/2 sum mu^2 (44 nats of spread between repetitions), so most rows hear
#: of one repetition only; under these seeds the LAST repetition -- the one the spare slots of phase 2 copy -- holds a
#: posterior worth 10 bars on at least a quarter of the rows (tests/test_ratspn_slice_host.py::test_sensitivity).
MODELS = {'r5_c1': (5, 1, 1001), 'r8_c1': (8, 1, 2101), 'r6_c3': (6, 3, 1203), 'r7_c10': (7, 10, 810), 'r8_c64': (8, 64, 1364),
          'r5_c3': (5, 3, 4303), 'r8_c3': (8, 3, 4503)}
ENVELOPE = ('r5_c1', 'r6_c3', 'r7_c10', 'r8_c64')
WALK = ('r5_c3', 'r8_c3')
VERDICT_KINDS = ('last_rep_x4', 'rep0_x4', 'vanishing')
TRIGGERS = ('huge', 'inf')


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---- the host side of the mapping, through the library -------------------------------------------------------------------
def prep_blocks(R: int, C: int) -> int:
    """Table work-groups of a model (ratspn_gemm_prep.h::gemm_prep_blocks: "NT * (8 / I) + cdiv(rows_total, threads / 64)"
    with NT = 2, I = 2, rows = R * 2 * S + C softmax rows, 512 threads): what an in-launch table check asks the grid for."""
    return 2 * 4 + cdiv(R * 2 * 2 + C, 8)


def lane_share(sl, cus: int, lanes: int, np_: int = 0) -> int:
    """The most work-groups a launch on `lanes` lanes takes (ratspn_gemm_slice.hip::slice_gmax), read off dps_slice_grid:
    a launch of up to that many blocks takes one work-group per block."""
    share = max(g for g in range(1, cus + 1) if sl.grid(g, cus, lanes, np_) == g)
    assert sl.grid(WALK_BLOCKS * share, cus, lanes, np_) == share
    return share


def expected_grid(sl, B: int, cus: int, lanes: int, R: int, C: int, frozen: bool) -> int:
    """Work-groups of the (last) slice launch of a call.  A frozen plan checks nothing (np = 0); a default-mode launch carries
    its own table check when gemm_slice_checks_inline says so ("B <= 64 * 32 * slice_gmax && ntiles >= np && slice_grid >=
    np") and then takes at least np work-groups; otherwise the stand-alone check launch runs and np = 0."""
    np_ = 0 if frozen else prep_blocks(R, C)
    nt = cdiv(B, 32)
    if np_ and not (B <= 64 * 32 * lane_share(sl, cus, lanes, np_) and nt >= np_ and sl.grid(nt, cus, lanes, np_) >= np_):
        np_ = 0
    per_launch = 64 * 32 * lane_share(sl, cus, lanes, np_)
    last = B - (cdiv(B, per_launch) - 1) * per_launch
    return sl.grid(cdiv(last, 32), cus, lanes, np_)


# ---- models ----------------------------------------------------------------------------------------------------------------
def make_model(name: str, kind: str = 'plain'):
    """The case's GaussianRatSpn on the host, in eval mode, unit scale.  The parameters are a pure function of the seed and
    trained-like, not the initialiser's: sum and root weights 3 randn, means 1.5 randn clamped to +-5.5 (unclamped, the
    largest of the 12 544 means reaches the expansion bound of 6 and its repetition silently goes to the exact route).
    kind (VERDICT_KINDS): 'last_rep_x4' / 'rep0_x4' multiply the means of that repetition alone by 4 (its eligibility bit is
    off: every block is evaluated exactly); 'vanishing' gives every sum node one dominant weight (the rest -200) and the root
    one dominant input (the rest -150): the linear-domain sums of the fast path vanish."""
    from deeprob.spn.models import GaussianRatSpn
    R, C, seed = MODELS[name]
    torch.manual_seed(seed)
    model = GaussianRatSpn(D, rg_depth=2, rg_batch=2, rg_sum=2, rg_repetitions=R, out_classes=C, random_state=seed).eval()
    base = model.base_layer
    assert tuple(base.loc.shape) == (4 * R, 2, D // 4) and not base.scale.requires_grad and bool((base.scale == 1).all())
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        base.loc.copy_((1.5 * torch.randn(base.loc.shape, generator=gen)).clamp_(-MU_MAX, MU_MAX))
        sums = [layer for layer in model.layers if hasattr(layer, 'weight')]
        assert len(sums) == 1 and tuple(sums[0].weight.shape) == (2 * R, 2, 4)
        sums[0].weight.copy_(3.0 * torch.randn(sums[0].weight.shape, generator=gen))
        assert tuple(model.root_layer.weight.shape) == (C, 4 * R)
        model.root_layer.weight.copy_(3.0 * torch.randn(model.root_layer.weight.shape, generator=gen))
        if kind == 'last_rep_x4':
            base.loc[4 * (R - 1):].mul_(4.0)
        elif kind == 'rep0_x4':
            base.loc[:4].mul_(4.0)
        elif kind == 'vanishing':
            sums[0].weight.fill_(-200.0)
            sums[0].weight[:, :, 1] = 0.0
            model.root_layer.weight.fill_(-150.0)
            model.root_layer.weight[:, 3] = 0.0
        else:
            assert kind == 'plain', kind
    return model


def state_dicts(model):
    """(float32, float64) state dicts of the model on the host."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def rep_mu_max(sd) -> np.ndarray:
    """max |mu| of every repetition."""
    loc = sd['base_layer.loc']
    return loc.abs().reshape(loc.shape[0] // 4, -1).max(dim=1).values.double().numpy()


# ---- references ------------------------------------------------------------------------------------------------------------
def oracle_rows(sd, x: torch.Tensor, chunk: int = 512) -> np.ndarray:
    """oracle.ratspn_oracle.ratspn_forward in the state dict's precision, at most `chunk` rows at a time: [B, C] float64."""
    dt = sd['base_layer.loc'].dtype
    with torch.no_grad():
        return np.concatenate([orc.ratspn_forward(sd, x[i:i + chunk].to(dt)).double().numpy()
                               for i in range(0, x.shape[0], chunk)])


def audit64(sd64, x: torch.Tensor, chunk: int = 512):
    """The float64 oracle on the rows of x together with what the kernel's verdicts look at, per row: {'out' [B, C],
    'finite' [B], 'sumsq' [B], 'sum_min' [B], 'root_min' [B], 'layer2' [B, R, 4], 'logw' [C, R, 4]}.  sum_min / root_min: the
    smallest sum over the inputs of a sum node / of a repetition's share of a root node, the inputs shifted by their
    maximum and weighted in the linear domain -- the `v` the fast path tests against 1e-30."""
    outs, smin, rmin, l2 = [], [], [], []
    wr = sd64['root_layer.weight']
    C, R = wr.shape[0], wr.shape[1] // 4
    logw = torch.log_softmax(wr, dim=1).view(C, R, 4)
    with torch.no_grad():
        for i in range(0, x.shape[0], chunk):
            out, acts = orc.ratspn_forward(sd64, x[i:i + chunk].double(), return_activations=True)
            prod0, sum1, prod2 = acts['layer0'], acts['layer1'], acts['layer2']
            assert prod0.shape[1:] == (2 * R, 4) and sum1.shape[1:] == (2 * R, 2) and prod2.shape[1:] == (R, 4)
            smin.append(torch.exp(sum1 - prod0.max(dim=2, keepdim=True).values).flatten(1).min(dim=1).values)
            v = torch.logsumexp(prod2[:, None] + logw[None], dim=3) - prod2.max(dim=2).values[:, None]     # [b, C, R]
            rmin.append(torch.exp(v).flatten(1).min(dim=1).values)
            outs.append(out)
            l2.append(prod2)
    xd = x.double()
    return dict(out=torch.cat(outs).numpy(), finite=torch.isfinite(x).all(dim=1).numpy(), sumsq=(xd * xd).sum(dim=1).numpy(),
                sum_min=torch.cat(smin).numpy(), root_min=torch.cat(rmin).numpy(), layer2=torch.cat(l2), logw=logw)


def broken_variants(audit, x: torch.Tensor):
    """Three wrong float64 references, the bugs the masks and the indexing of phase 2 could have:
      dup_last     the last repetition counted twice at the root (a spare slot of phase 2 that leaks in);
      class_shift  root weights of class c taken from class c - 1, for c >= 1 (None for one class);
      q_twice      one spare slot's share of sum x^2 added twice: the share of slice 6, half 0 -- features 0 .. 7 of the
                   K-steps 42 .. 48."""
    l2, logw = audit['layer2'], audit['logw']
    t = l2[:, None] + logw[None]                                       # [B, C, R, 4]
    dup = torch.logsumexp(torch.cat([t, t[:, :, -1:]], dim=2).flatten(2), dim=2).numpy()
    shift = None
    if logw.shape[0] > 1:
        lw = logw.clone()
        lw[1:] = logw[:-1]
        shift = torch.logsumexp((l2[:, None] + lw[None]).flatten(2), dim=2).numpy()
    feats = torch.tensor([(42 + kk) * 16 + i for kk in range(7) for i in range(8)])
    q = (x[:, feats].double() ** 2).sum(dim=1).numpy()
    return dict(dup_last=dup, class_shift=shift, q_twice=audit['out'] - 0.5 * q[:, None])


def row_rel(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """rel_err's measure per row: max over the classes of |a - b| / max(1, |b|)."""
    return (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max(axis=1)


class Case:
    """x [B, D] float32 (host, or the device of the two-launch case); rows: the rows the reference covers (None: all);
    want [len(rows), C] float64; noise: the float32 oracle's distance from want; exact: the blocks of 32 rows meant for the
    exact route (None: all of them); planted: rows that hold a trigger."""

    def __init__(self, name, kind, x, rows, want, noise, exact, planted=()):
        self.name, self.kind, self.x, self.rows, self.want, self.noise = name, kind, x, rows, want, noise
        self.exact, self.planted = exact, tuple(planted)
        self.R, self.C, _ = MODELS[name]
        self.B = x.shape[0]

    def got_rows(self, ll: torch.Tensor) -> np.ndarray:
        return (ll if self.rows is None else ll[self.rows.to(ll.device)]).double().cpu().numpy()


def _finish(name, kind, x, rows, exact, planted=(), inf_rows=None, all_exact_reason=None):
    """References on `rows` of x and the by-construction assertions.  Rows with +-inf evidence are referred to the float32
    oracle: its nan_to_num turns the -inf leaf term into the largest finite number OF THE FORMAT, -3.4e38, which is part of
    the result and which a float64 evaluation (-1.8e308) cannot state (tests/ratspn_gaussian_cases.py::forward_reference)."""
    model = make_model(name, kind if kind in VERDICT_KINDS else 'plain')
    sd32, sd64 = state_dicts(model)
    xr = (x if rows is None else x[rows.to(x.device)]).cpu()
    audit = audit64(sd64, xr)
    want = audit['out'].copy()
    want32 = oracle_rows(sd32, xr)
    inf = ~torch.isfinite(xr).all(dim=1).numpy() & ~torch.isnan(xr).any(dim=1).numpy()
    want[inf] = want32[inf]
    assert np.isfinite(want).all()
    noise = rel_err(want32, want)
    # ---- by construction ----
    ridx = np.arange(x.shape[0]) if rows is None else rows.numpy()
    mu = rep_mu_max(sd64)
    if all_exact_reason is None:
        assert mu.max() <= MU_MAX, mu
        on_exact = np.isin(ridx // 32, np.asarray(sorted(exact), dtype=np.int64)) if exact else np.zeros(len(ridx), bool)
        fast = ~on_exact
        assert audit['finite'][fast].all()
        assert audit['sumsq'][fast].max() <= SUMSQ_MAX, audit['sumsq'][fast].max()
        assert audit['sum_min'][fast].min() >= NODE_MIN and audit['root_min'][fast].min() >= NODE_MIN, \
            (audit['sum_min'][fast].min(), audit['root_min'][fast].min())
    else:
        all_exact_reason(mu, audit)
    case = Case(name, kind, x, rows, want, noise, exact, planted)
    case.audit = audit
    return case


# ---- 1: the envelope on the fast path ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def envelope_case(name: str, B: int) -> Case:
    """Evidence 1.2 randn, every row on the fast path."""
    R, C, seed = MODELS[name]
    x = 1.2 * torch.randn(B, D, generator=torch.Generator().manual_seed(10 * seed + B))
    return _finish(name, 'envelope', x, None, exact=[])


# ---- 2: positions on a work-group's walk -------------------------------------------------------------------------------------
def walk_layout(G: int):
    """A launch of G work-groups that walk WALK_BLOCKS blocks each (work-group g: blocks g, g + G, ...), the last block
    ragged (5 rows).  {position: (work-group, [blocks that hold an exact-route sample])}: the first block of one work-group, a
    middle block of another, the last block of a third (a full block: the ragged one stays on the fast path), every block of a
    fourth -- ten exact blocks in one work-group, more than the eight waves that share them out."""
    assert G >= 8, G
    nt = WALK_BLOCKS * G
    lay = {'first': (1, [1]), 'middle': (G // 2, [G // 2 + (WALK_BLOCKS // 2) * G]),
           'last': (G - 2, [G - 2 + (WALK_BLOCKS - 1) * G]), 'every': (3, [3 + it * G for it in range(WALK_BLOCKS)])}
    assert len({wg for wg, _ in lay.values()}) == 4
    for wg, blocks in lay.values():
        assert all(b % G == wg and 0 <= b < nt - 1 for b in blocks)
    return 32 * nt - 27, lay


@functools.lru_cache(maxsize=None)
def walk_case(name: str, trigger: str, G: int) -> Case:
    """One exact-route sample (`trigger`: a single entry of 200.0, or a single +inf) at each position of walk_layout(G).  The
    reference covers every row of the affected blocks, of their neighbours in memory and on the walk (b +- 1, b +- G), of
    the ragged last block, and 1024 rows drawn from the whole batch."""
    R, C, seed = MODELS[name]
    B, lay = walk_layout(G)
    nt = cdiv(B, 32)
    gen = torch.Generator().manual_seed(10 * seed + TRIGGERS.index(trigger))
    x = 1.2 * torch.randn(B, D, generator=gen)
    exact, planted = [], []
    for wg, blocks in lay.values():
        for b in blocks:
            it = b // G
            row, feat = 32 * b + (5 * it + 7 * wg) % 32, (97 * b + 13) % D
            x[row, feat] = HUGE if trigger == 'huge' else float('inf')
            exact.append(b)
            planted.append(row)
    near = {c for b in exact for c in (b - G, b - 1, b, b + 1, b + G) if 0 <= c < nt} | {0, nt - 1}
    rows = torch.cat([torch.arange(32 * b, min(32 * b + 32, B)) for b in sorted(near)] +
                     [torch.randint(0, B, (1024,), generator=gen)]).unique()
    # every block of the whole batch: which ones break the evidence conditions
    xd = x.double()
    sumsq = (xd * xd).sum(dim=1)
    broken = ~torch.isfinite(x).all(dim=1) if trigger == 'inf' else sumsq > SUMSQ_BOUND
    assert sorted(set((torch.nonzero(broken).flatten() // 32).tolist())) == sorted(exact)
    assert torch.nonzero(broken).flatten().tolist() == sorted(planted)
    assert torch.isfinite(x[~broken]).all() and sumsq[~broken].max().item() <= SUMSQ_MAX and not torch.isnan(x).any()
    return _finish(name, 'walk_' + trigger, x, rows, exact, planted)


# ---- 3: the model's verdicts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def verdict_case(name: str, kind: str, B: int = 257) -> Case:
    """Clean evidence under a model that the fast path must decline: every block goes to the exact route."""
    R, C, seed = MODELS[name]
    x = 1.2 * torch.randn(B, D, generator=torch.Generator().manual_seed(10 * seed + 5 + VERDICT_KINDS.index(kind)))

    def reason(mu, audit):
        assert audit['finite'].all() and audit['sumsq'].max() <= SUMSQ_MAX
        if kind == 'vanishing':
            # (the root's other repetitions carry e^-150: every row; a sum node's dominant pair under the lesser channels:
            # where those are 92 nats apart)
            assert mu.max() <= MU_MAX and audit['root_min'].max() < 1e-40 and (audit['sum_min'] < 1e-40).any()
        else:
            off = R - 1 if kind == 'last_rep_x4' else 0
            assert mu[off] > 6.0 and np.delete(mu, off).max() <= MU_MAX, mu
            assert audit['sum_min'].min() >= NODE_MIN and audit['root_min'].min() >= NODE_MIN

    return _finish(name, kind, x, None, exact=None, all_exact_reason=reason)


# ---- 4: NaN evidence -------------------------------------------------------------------------------------------------------------
NAN_ROW, PARTIAL_ROW = 40, 100


@functools.lru_cache(maxsize=None)
def nan_case(name: str = 'r6_c3', B: int = 257) -> Case:
    """One all-NaN row and one partly marginalised row in a clean batch: their two blocks leave the fast path (and raise the
    hint), the other seven stay on it."""
    R, C, seed = MODELS[name]
    x = 1.2 * torch.randn(B, D, generator=torch.Generator().manual_seed(10 * seed + 9))
    x[NAN_ROW] = float('nan')
    x[PARTIAL_ROW, 100:140] = float('nan')
    x[PARTIAL_ROW, 700::3] = float('nan')
    case = _finish(name, 'nan', x, None, exact=[NAN_ROW // 32, PARTIAL_ROW // 32], planted=(NAN_ROW, PARTIAL_ROW))
    assert np.abs(case.want[NAN_ROW]).max() <= 1e-9      # (every class: log sum softmax = 0)
    return case


# ---- 5: two launches per call ------------------------------------------------------------------------------------------------------
def two_launch_layout(share: int):
    """(B, per_launch, planted rows): a call of 64 * 32 * share + 32 * 3 + 5 rows is one launch of `share` work-groups that
    walk 64 blocks each and a second one of four blocks, the last ragged; one exact-route sample in the last block of the
    first launch, one in the first block of the second."""
    per_launch = 64 * 32 * share
    return per_launch + 32 * 3 + 5, per_launch, (per_launch - 32 + 11, per_launch + 20)


def two_launch_case(name: str, share: int, device) -> Case:
    """Evidence drawn on `device`; the reference covers rows 0 and B - 1, the 64 rows on either side of the launch boundary,
    the last ragged block and 1024 rows drawn from the whole batch.  (Not cached: 110 MB of evidence.)"""
    R, C, seed = MODELS[name]
    B, per_launch, planted = two_launch_layout(share)
    x = 1.2 * torch.randn(B, D, device=device, generator=torch.Generator(device).manual_seed(10 * seed + 7))
    for i, row in enumerate(planted):
        x[row, (131 * i + 17) % D] = HUGE
    rows = torch.cat([torch.tensor([0, B - 1]), torch.arange(per_launch - 64, per_launch + 64), torch.arange(B - 5, B),
                      torch.randint(0, B, (1024,), generator=torch.Generator().manual_seed(seed))]).unique()
    sumsq = (x.double() ** 2).sum(dim=1)
    broken = torch.nonzero(sumsq > SUMSQ_BOUND).flatten().tolist()
    assert broken == list(planted) and bool(torch.isfinite(x).all())
    keep = torch.ones(B, dtype=torch.bool, device=x.device)
    keep[list(planted)] = False
    assert sumsq[keep].max().item() <= SUMSQ_MAX
    return _finish(name, 'two_launches', x, rows, exact=[r // 32 for r in planted], planted=planted)

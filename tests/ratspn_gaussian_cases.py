"""GaussianRatSpn's leaf layer at the shapes that reach every DIST = 0 route of the RAT-SPN leaf kernels: the case table, the
host dispatch restated as two pure functions, seeded parameters, evidence and upstream gradients, and the float64 / float32
references the device tests compare with.  Everything here runs on the host.

R = regions, I = channels, d = variables per region, D = in_features.  Every case exists in two variants: 'scaled'
(optimize_scale=True: scale.requires_grad, no unit-scale hint) and 'unit' (the frozen scale of 1: the hint is given, the
matrix-core route and the means-only kernels become reachable, and scale.grad is None: W1 / WANT1 = false).

A helper module (no tests in it)."""
import torch

from oracle import ratspn_oracle as orc

LL_TOL = 1e-5     # the project's bar: 1e-5 relative on fp32 log-likelihoods
GRAD_TOL = 1e-4   # relative to the largest magnitude of the tensor

#: name -> (constructor kwargs, R, I, d, pad) as GaussianRatSpn(random_state=3, **kwargs) builds them
CASES = {
    # CB 8 / SPL 1; GEMM route in the unit variant (25 chunks, the last 16 wide); moment kernel with 25 column tiles, the
    # last one 16 wide
    'mnist8': (dict(in_features=784, rg_depth=2, rg_repetitions=4, rg_batch=8, rg_sum=8), 16, 8, 196, 0),
    # QB 2; GEMM with a 4-wide last chunk and one ragged column group (R I = 96 < 128); moment kernel with 2 regions per
    # row tile
    'wide16_d1': (dict(in_features=100, rg_depth=1, rg_repetitions=3, rg_batch=16, rg_sum=4, out_classes=3), 6, 16, 50, 0),
    # D % 4 != 0: unit = the compact-record kernel, scaled = GEN with LDS records; CBK 2 on the staged and 64-sample
    # kernels; scalar staging copy
    'pad2': (dict(in_features=61, rg_depth=3, rg_repetitions=5, rg_batch=2, rg_sum=3), 40, 2, 8, 3),
    # CB 1, CBK 1, odd d
    'odd3': (dict(in_features=130, rg_depth=2, rg_repetitions=7, rg_batch=3, rg_sum=5), 28, 3, 33, 2),
    # one channel; unit = GEN false with full records; float4 staging copy
    'one': (dict(in_features=64, rg_depth=2, rg_repetitions=4, rg_batch=1, rg_sum=2), 16, 1, 16, 0),
    # CB 2 without LDS records (I > 2), CBK 2
    'six': (dict(in_features=50, rg_depth=1, rg_repetitions=2, rg_batch=6, rg_sum=2), 4, 6, 25, 0),
    # CB 4; GEMM with 49 chunks and padding; moment kernel with padding (gradients zeroed first)
    'ad4': (dict(in_features=1556, rg_depth=4, rg_repetitions=3, rg_batch=4, rg_sum=4), 48, 4, 98, 12),
    # pad >= d: the per_rep reasoning of leaf_backward_common for d/dx
    'heavy_pad': (dict(in_features=9, rg_depth=3, rg_repetitions=5, rg_batch=2, rg_sum=2), 40, 2, 2, 7),
    # staged kernel, passes = 4 at B = 1024 on 256 compute units
    'many_groups': (dict(in_features=61, rg_depth=3, rg_repetitions=8, rg_batch=3, rg_sum=2), 64, 3, 8, 3),
    # 16 * (1400 + 4) * 4 = 89,856 B > 80 KB and SP > 1024: the non-staged kernel with 16-sample tiles
    'long_rows': (dict(in_features=1400, rg_depth=1, rg_repetitions=2, rg_batch=3, rg_sum=2), 4, 3, 700, 0),
    # 65 chunks > 64: the unit variant stays on the VALU kernel; moment kernel with 65 column tiles, the last one 4 wide
    'beyond_gemm': (dict(in_features=2052, rg_depth=2, rg_repetitions=2, rg_batch=8, rg_sum=2), 8, 8, 513, 0),
    # 40000 samples > 32768: SPL 2 at CB 8
    'two_per_lane': (dict(in_features=16, rg_depth=1, rg_repetitions=2, rg_batch=8, rg_sum=8), 4, 8, 8, 0),
    # the only two-channel case with D % 4 == 0: the GEMM route with NTG 2 -- three chunks, the last 8 wide, and R I = 24
    # columns of a 64-column group
    'pairs_gemm': (dict(in_features=72, rg_depth=2, rg_repetitions=3, rg_batch=2, rg_sum=2), 12, 2, 18, 0),
}
VARIANTS = ('scaled', 'unit')
ILL_REGIMES = ('mu_over_s_50', 'uint8_range', 'clusters')
SEED = 3
_NAME_SEED = {name: 300 + i for i, name in enumerate(sorted(CASES))}
_KIND_SEED = {'clean': 0, 'nan': 1, 'huge': 2, 'inf': 3}


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def geometry(name: str):
    """(D, R, I, d, pad) of the table."""
    kw, R, I, d, pad = CASES[name]
    return kw['in_features'], R, I, d, pad


# ---- the host dispatch, restated ------------------------------------------------------------------------------------------
def forward_route(name: str, variant: str, B: int, x_aligned: bool = True, mfma: bool = True):
    """What dpk_gaussian_leaf_forward launches (csrc/ratspn_fwd.hip::leaf_forward_common): ('gemm', NTG, NG, NCH) or
    ('valu', QB, CB, SPL, GEN, compact).  `x_aligned`: x and out are 16-byte aligned; `mfma`: dpk_ratspn_mfma_route."""
    D, R, I, d, _ = geometry(name)
    unit = variant == 'unit'
    # ratspn_fwd.hip::leaf_gemm_route: the route is on, the unit-scale hint, common.h::leaf_gemm_shape_ok (I in {2, 4, 8,
    # 16}, D % 4 == 0, at most 64 chunks of 16 * kLeafGemmKS = 32 features: "chunk bit masks of the kernel"), x / out aligned
    if mfma and unit and I in (2, 4, 8, 16) and D % 4 == 0 and cdiv(D, 32) <= 64 and x_aligned:
        NTG = 4 if I >= 4 else I                            # common.h::leaf_ntg
        return ('gemm', NTG, cdiv(R * I, 32 * NTG), cdiv(D, 32))   # ratspn_leaf_gemm.hip::ratspn_leaf_gemm_forward
    QB = 4 if R % 4 == 0 else 2                             # common.h::leaf_group
    CB = 8 if I % 8 == 0 else 4 if I % 4 == 0 else 2 if I % 2 == 0 else 1   # ratspn_fwd.hip::channel_block
    # ratspn_fwd.hip::leaf_forward_dispatch: "a.B > 2 * 256 * 64" sends CB 8 to two samples per lane, the others always
    SPL = 1 if (CB == 8 and B <= 2 * 256 * 64) else 2
    # ratspn_fwd.hip::launch_leaf: the means-only build "where the LDS-table pipeline does (Gaussian, CB <= 2, SPL == 2)"
    GEN = not (unit and CB <= 2 and SPL == 2)
    # ... and its compact records: launch_leaf asks for them at CB == 2, prepare_leaf_tables writes them at I == 2 only
    # (common.h::carve_ratspn_ws gives tabcap_c = 0 for I > 2: such a launch reads no LDS records at all)
    compact = (not GEN) and CB == 2 and I == 2
    return ('valu', QB, CB, SPL, GEN, compact)


def backward_route(name: str, variant: str, B: int, want_scale: bool, x_aligned: bool = True, g_aligned: bool = True,
                   dropout: bool = False, cus: int = 256):
    """What the parameter-gradient part of dpk_gaussian_leaf_backward / dpk_leaf_backward_dropout launches
    (csrc/ratspn_layers.hip::leaf_backward_common): ('moment', W1), ('staged', CBK, WANT1, passes) or ('plain', CBK, tile).
    `variant` does not enter (the backward is given no unit-scale hint); `want_scale`: grad_scale is requested."""
    D, R, I, d, _ = geometry(name)
    # "const bool moment = ... B <= kLeafMomentMaxB && drop_p == 0.f && I <= 32 && (32 % I) == 0 && ((R * I) % 32) == 0 &&
    #  d <= 32767 && ... (g & 15) == 0", kLeafMomentMaxB = 2048 ("constexpr int kLeafMomentMaxB = 2048;")
    if 0 < B <= 2048 and not dropout and I <= 32 and 32 % I == 0 and (R * I) % 32 == 0 and d <= 32767 and g_aligned:
        return ('moment', bool(want_scale))
    cbk = 4 if I % 4 == 0 else 2 if I % 2 == 0 else 1       # "const int cbk = ..."
    tile = 64 if B > 1024 else 16                           # "const int tile = (B > 1024) ? kLeafBwdTile : 16;"
    stage_bytes = tile * (D + R * cbk) * 4                  # "const size_t stage_bytes = ..."
    # common.h::carve_ratspn_ws: SP = align_up(QB d + (kBlock - 1) QB NC, kBlock) + kTableSlack, NC = cdiv(D, kChunk = 64)
    QB = 4 if R % 4 == 0 else 2
    SP = cdiv(QB * d + 3 * QB * cdiv(D, 64), 4) * 4 + 16
    # "staged = tile == 16 && drop_p == 0.f && stage_bytes <= 80 * 1024 && w.SP <= 4 * 256 && ((D & 3) != 0 || x aligned)"
    staged = tile == 16 and not dropout and stage_bytes <= 80 * 1024 and SP <= 4 * 256 and (D % 4 != 0 or x_aligned)
    if not staged:
        return ('plain', cbk, tile)
    passes = 1
    # "while (passes < 8 && cdiv(B, tile * passes * 2) * w.G * (I / cbk) >= 2 * device_cus()) passes *= 2;"
    while passes < 8 and cdiv(B, tile * passes * 2) * (R // QB) * (I // cbk) >= 2 * cus:
        passes *= 2
    return ('staged', cbk, bool(want_scale), passes)


def moment_shape(name: str):
    """(padded, ragged last column tile) of the moment kernel for this case: its grid is (R I / 32, cdiv(D, 32))."""
    D, _, _, _, pad = geometry(name)
    return pad > 0, D % 32 != 0


# ---- models ---------------------------------------------------------------------------------------------------------------
def make_model(name: str, variant: str, regime: str = 'plain'):
    """The case's GaussianRatSpn on the host, in eval mode, its region graph asserted against the table.  loc = randn;
    'scaled': scale = 0.5 + rand with about 2 % of the entries at 0.05 and 2 % at 20; 'unit': scale untouched (1, frozen).
    regime 'far_means': 5 % of the means at +-8 (beyond kExpandBound = 6: those regions lose their eligibility for the
    expanded square and are evaluated exactly).  The ill-conditioned regimes come with their own evidence: make_ill_case."""
    from deeprob.spn.models import GaussianRatSpn
    assert variant in VARIANTS and regime in ('plain', 'far_means'), (variant, regime)
    kw, R, I, d, pad = CASES[name]
    gen = torch.Generator().manual_seed(_NAME_SEED[name])
    torch.manual_seed(_NAME_SEED[name])                 # (the sum weights' Dirichlet initialiser)
    model = GaussianRatSpn(random_state=SEED, optimize_scale=(variant == 'scaled'), **kw).eval()
    base = model.base_layer
    assert (base.in_regions, base.out_channels, base.dimension, base.pad) == (R, I, d, pad), \
        (name, base.in_regions, base.out_channels, base.dimension, base.pad)
    assert tuple(base.loc.shape) == (R, I, d) and base.scale.requires_grad == (variant == 'scaled')
    if name == 'heavy_pad':
        assert base.pad >= base.dimension
    with torch.no_grad():
        loc = torch.randn(base.loc.shape, generator=gen)
        n = loc.numel()
        if regime == 'far_means':
            perm = torch.randperm(n, generator=gen)
            far = max(2, n // 20)
            loc.view(-1)[perm[:far:2]] = 8.0
            loc.view(-1)[perm[1:far:2]] = -8.0
        base.loc.copy_(loc)
        if variant == 'scaled':
            scale = 0.5 + torch.rand(base.scale.shape, generator=gen)
            perm = torch.randperm(n, generator=gen)
            k = max(1, n // 50)
            scale.view(-1)[perm[:k]] = 0.05
            scale.view(-1)[perm[k:2 * k]] = 20.0
            base.scale.copy_(scale)
        else:
            assert bool((base.scale == 1).all())
    return model


def ill_regime(base, regime: str, B: int, gen: torch.Generator) -> torch.Tensor:
    """Parameters and evidence on which the raw moments of the leaf backward cancel (|mu| / s large), for any Gaussian leaf
    layer `base` with trainable scales: writes base.loc / base.scale and returns the evidence [B, D].
      mu_over_s_50   small learned scales (0.1) around means far from 0 (5 +- 1), evidence within 0.1 of them;
      uint8_range    integer evidence in 0 .. 255 around per-variable centres, scales of 3;
      clusters       a sample sits on one of four clusters (0, 60, 128, 200), channel k on cluster k % 4: what no
                     per-variable pivot can centre."""
    assert regime in ILL_REGIMES, regime
    D, I = base.in_features, base.loc.shape[1]
    with torch.no_grad():
        if regime == 'mu_over_s_50':
            centre = 5.0 + torch.randn(D, generator=gen)
            x = centre + 0.1 * torch.randn(B, D, generator=gen)
            spread, scale = 0.05, 0.1
        elif regime == 'uint8_range':
            centre = 40.0 + 170.0 * torch.rand(D, generator=gen)
            x = (centre + 3.0 * torch.randn(B, D, generator=gen)).round().clamp(0, 255)
            spread, scale = 2.0, 3.0
        else:
            centre = torch.zeros(D)
            offs = torch.tensor([0.0, 60.0, 128.0, 200.0])
            x = offs[torch.randint(0, 4, (B, 1), generator=gen)] + torch.randn(B, D, generator=gen)    # (a sample = one cluster)
            spread, scale = 0.5, 1.0
        loc = torch.empty_like(base.loc)
        mask = base.mask                                  # [regions, positions] -> variable
        for k in range(I):
            centred = centre[mask.clamp_min(0)]
            if regime == 'clusters':
                centred = centred + offs[k % 4]
            loc[:, k] = centred + spread * torch.randn(centred.shape, generator=gen)
        base.loc.copy_(loc)
        base.scale.fill_(scale).mul_(1.0 + 0.2 * torch.rand(base.scale.shape, generator=gen))
    return x


def make_ill_case(name: str, regime: str, B: int, kind: str = 'clean'):
    """(model, x): the 'scaled' variant of the case in one of the ill-conditioned regimes, with that regime's evidence;
    kind 'nan' marginalises 20 % of it (row 0 all NaN, row 1 fully observed)."""
    model = make_model(name, 'scaled')
    gen = torch.Generator().manual_seed(7000 + 10 * _NAME_SEED[name] + ILL_REGIMES.index(regime) + 100000 * B)
    x = ill_regime(model.base_layer, regime, B, gen)
    if kind == 'nan':
        _plant_nan(x, gen)
    else:
        assert kind == 'clean', kind
    return model, x


# ---- evidence and upstream gradients ----------------------------------------------------------------------------------------
def _plant_nan(x: torch.Tensor, gen: torch.Generator, frac: float = 0.2):
    keep = x[1].clone() if x.shape[0] > 1 else None
    x[torch.rand(x.shape, generator=gen) < frac] = float('nan')
    x[0] = float('nan')
    if keep is not None:
        x[1] = keep


def make_evidence(name: str, B: int, kind: str) -> torch.Tensor:
    """[B, D] float32.  'clean': randn.  'nan': 20 % NaN, row 0 all NaN, row 1 fully observed.  'huge': 1 % of the entries
    at +-1e3 and +-1e6, and one row (row 2, or the last one of a smaller batch) with every entry at 7.0: sum x^2 = 49 D >
    36 D, so a wave of the matrix-core route must redo it exactly.  'inf': 'nan' plus (B >= 4) rows 2 and 3 with a single
    +inf and a single -inf entry."""
    D = geometry(name)[0]
    gen = torch.Generator().manual_seed(1000 * _NAME_SEED[name] + 10 * B + _KIND_SEED[kind])
    x = torch.randn(B, D, generator=gen)
    if kind == 'clean':
        return x
    if kind == 'huge':
        pick = torch.rand(B, D, generator=gen)
        for i, v in enumerate((1e3, -1e3, 1e6, -1e6)):
            x[(pick >= 0.0025 * i) & (pick < 0.0025 * (i + 1))] = v
        x[min(2, B - 1)] = 7.0
        return x
    assert kind in ('nan', 'inf'), kind
    _plant_nan(x, gen)
    if kind == 'inf' and B >= 4:
        f = torch.randint(0, D, (2,), generator=gen)
        x[2, f[0]] = float('inf')
        x[3, f[1]] = float('-inf')
    return x


def inf_row_mask(x: torch.Tensor) -> torch.Tensor:
    return torch.isinf(x).any(dim=1)


def make_upstream(name: str, B: int, sign: str) -> torch.Tensor:
    """[B, R, I] float32 gradient handed to the leaf layer.  'mixed': randn.  'negative': -rand, one sign -- what a
    likelihood loss hands down; the two take different branches of the moment kernel's conditioning detector."""
    _, R, I, _, _ = geometry(name)
    gen = torch.Generator().manual_seed(50000 + 1000 * _NAME_SEED[name] + B)
    if sign == 'mixed':
        return torch.randn(B, R, I, generator=gen)
    assert sign == 'negative', sign
    return -torch.rand(B, R, I, generator=gen)


def misaligned(t: torch.Tensor) -> torch.Tensor:
    """The same values as a contiguous view at storage offset 1 of a larger buffer on t's device: 4-byte aligned only."""
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == 1
    return view


# ---- references -------------------------------------------------------------------------------------------------------------
def leaf_state(model, dtype=torch.float64):
    """mask, pad_mask (or None), loc and scale of the model's leaf layer on the host, the parameters in `dtype`."""
    base = model.base_layer
    return dict(mask=base.mask.detach().cpu().clone(),
                pad_mask=base.pad_mask.detach().cpu().clone() if base.pad > 0 else None,
                loc=base.loc.detach().cpu().to(dtype), scale=base.scale.detach().cpu().to(dtype))


def forward_reference(state, x: torch.Tensor):
    """The oracle's leaf layer [B, R, I] as a float64 array: evaluated in float64 -- except the rows with +-inf evidence, which
    are evaluated in float32, the reference's own format.  There the reference's nan_to_num (ratspn.py:103) turns the -inf
    leaf term of a +-inf entry into the LARGEST FINITE NUMBER OF THE FORMAT, and that number is part of the result: -3.4e38
    in the reference, -1.8e308 in a float64 restatement, which no float32 kernel can return.  (Every such row holds a single
    infinite entry, so no two of these terms meet in one region's sum.)"""
    def run(dtype, xx):
        with torch.no_grad():
            return orc.gaussian_leaf(xx.to(dtype), state['mask'], state['pad_mask'], state['loc'].to(dtype),
                                     state['scale'].to(dtype)).double().numpy()

    leaf = run(torch.float64, x)
    planted = inf_row_mask(x)
    if planted.any():
        leaf[planted.numpy()] = run(torch.float32, x[planted])
    return leaf


def reference_grads(state, x: torch.Tensor, g: torch.Tensor, dtype=torch.float64, drop=None, block: int = 256):
    """Autograd of (leaf * g).sum() through the oracle's leaf layer in `dtype`: {'out', 'loc', 'scale', 'x'} as float64
    arrays.  The marginalised terms (NaN in x) -- and `drop` [B, R, I, d], the replayed dropout mask -- are cut out of the
    graph through the oracle's drop= (its own backward computes 0 * NaN there); x.grad is 0 in those entries.  Evaluated in
    row blocks of at most `block` samples, the parameter gradients added up in `dtype`, so that the [B, R, I, d] temporary of
    the widest case stays near 100 MB."""
    mask, pad_mask = state['mask'], state['pad_mask']
    loc = state['loc'].to(dtype).clone().requires_grad_(True)
    scale = state['scale'].to(dtype).clone().requires_grad_(True)
    I = loc.shape[1]
    outs, gxs = [], []
    for lo in range(0, x.shape[0], block):
        xb, gb = x[lo:lo + block], g[lo:lo + block].to(dtype)
        nan = torch.isnan(xb)
        xf = torch.where(nan, torch.zeros_like(xb), xb).to(dtype).requires_grad_(True)
        cut = None
        if nan.any() or drop is not None:
            cut = nan[:, mask].unsqueeze(2).expand(-1, -1, I, -1)                    # [b, R, I, d]
            if drop is not None:
                cut = cut | drop[lo:lo + block]
        with torch.enable_grad():
            out = orc.gaussian_leaf(xf, mask, pad_mask, loc, scale, drop=cut)
            (out * gb).sum().backward()
        outs.append(out.detach().double())
        gxs.append(xf.grad.double())
    return dict(out=torch.cat(outs).numpy(), loc=loc.grad.double().numpy(), scale=scale.grad.double().numpy(),
                x=torch.cat(gxs).numpy())

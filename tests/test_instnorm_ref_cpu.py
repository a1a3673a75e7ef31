"""The float64 reference of the instance-norm family (tests/instnorm_ref.py) and its fp32-compute yardstick, on the CPU.

* the reference equals F.instance_norm + F.leaky_relu under float64 autograd (affine / non-affine, residual, pair);
* the yardstick - the same composition in fp32 on the dtype-rounded inputs, outputs rounded once - stays below HALF of the tolerance
  tests/test_hip_instnorm_forms.py holds the kernels to, at every (S, C, option) of its matrix except the long rows: honest arithmetic has
  room at S = 2 .. 2049, so a kernel above the bar there is wrong and not unlucky;
* assert_parity fails against a reference with the last row zeroed, the last channel of a ragged tile zeroed, two samples' styles swapped,
  gadd dropped, or one channel's statistics taken from its neighbour: the defects a wrong guard or index in csrc/norm.hip would produce."""
import pytest
import torch
import torch.nn.functional as F

import instnorm_ref as R
from conftest import rel_err
from parity import assert_parity, local_err

DTYPES = [torch.float32, torch.bfloat16]


def _name(dt):
    return {torch.float32: "fp32", torch.bfloat16: "bf16"}[dt]


# ----------------------------------------------------------------------------------------------------------------- the reference
def _torch_norm(x, styles, gammas, betas):
    """per sample, as the reference network does (conditional_instance_norm.py): F.instance_norm on [1, C, S] with the style's rows"""
    outs = []
    for i in range(x.shape[0]):
        s = styles[i] if styles is not None else 0
        w = gammas[s] if gammas is not None else None
        b = betas[s] if betas is not None else None
        outs.append(F.instance_norm(x[i:i + 1].permute(0, 2, 1), weight=w, bias=b, eps=R.EPS).permute(0, 2, 1)[0])
    return torch.stack(outs)


@pytest.mark.parametrize("affine", ["both", "none"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
def test_reference_is_instance_norm_and_leaky_relu(affine, res):
    c = R.Case(3, 37, 10, torch.float32)
    cfg = c.config(styles=[1, 0, 1], affine=affine, res=res)
    got = R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"])
    xl = c.x.double().requires_grad_(True)
    rl = c.res.double().requires_grad_(True)
    gl = [g.double().requires_grad_(True) for g in c.gam] if affine == "both" else None
    bl = [b.double().requires_grad_(True) for b in c.bet] if affine == "both" else None
    y = _torch_norm(xl, cfg["styles"], gl, bl)
    y = F.leaky_relu(y + rl if res else y, R.SLOPE)
    y.backward(c.dy.double())
    assert_parity(got["y"], y, 1e-12, "y")
    assert_parity(*R.determined(xl.grad, got["dx"])[::-1], 1e-11, "dx")
    if res:
        assert_parity(*R.determined(rl.grad, got["dres"])[::-1], 1e-12, "dres")
    if affine == "both":
        for s in range(2):
            assert_parity(got["dgamma"][s], gl[s].grad, 1e-11, f"dgamma[{s}]")
            assert_parity(got["dbeta"][s], bl[s].grad, 1e-11, f"dbeta[{s}]")
    # gadd is added to dx and to nothing else
    g2 = R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"], gadd=c.gadd)
    assert torch.equal(torch.nan_to_num(g2["dx"]), torch.nan_to_num(got["dx"] + c.gadd.double())) and torch.equal(g2["y"], got["y"])


def test_reference_pair_is_two_instance_norms():
    c = R.Case(2, 29, 6, torch.float32)
    styles = [1, 0]
    got = R.pair_backward(c.dy, c.x, c.xb, styles, c.gam, c.bet, c.gam_b, c.bet_b)
    leaves = [t.double().requires_grad_(True) for t in (c.x, c.xb)]
    rows = [[t.double().requires_grad_(True) for t in ts] for ts in (c.gam, c.bet, c.gam_b, c.bet_b)]
    y = F.leaky_relu(_torch_norm(leaves[0], styles, rows[0], rows[1]) + _torch_norm(leaves[1], styles, rows[2], rows[3]), R.SLOPE)
    y.backward(c.dy.double())
    assert_parity(got["y"], y, 1e-12, "y")
    assert_parity(*R.determined(leaves[0].grad, got["dxa"])[::-1], 1e-11, "dxa")
    assert_parity(*R.determined(leaves[1].grad, got["dxb"])[::-1], 1e-11, "dxb")
    for k, name in enumerate(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")):
        for s in range(2):
            assert_parity(got[name][s], rows[k][s].grad, 1e-11, f"{name}[{s}]")


def test_an_unused_style_has_zero_gradients_and_absent_rows_none():
    c = R.Case(2, 9, 4, torch.float32)
    r = R.backward(c.dy, c.x, [0, 0], c.gam, c.bet)
    assert float(r["dgamma"][1].abs().max()) == 0.0 and float(r["dbeta"][1].abs().max()) == 0.0 and float(r["dgamma"][0].abs().max()) > 0
    r = R.backward(c.dy, c.x, None, c.gam[:1], None)
    assert len(r["dgamma"]) == 1 and r["dbeta"] == [None] and r["dres"] is None


def test_undeterminable_activation_signs_are_marked_and_rare():
    """a pre-activation of exactly zero (x symmetric about its mean, beta = 0, residual 0 in the middle row) is NaN in dx / dres and nowhere
    else; at the streaming shape about 1 element in 50 000 is marked"""
    x = torch.tensor([[[-1.0], [0.0], [1.0]]])
    dy = torch.ones(1, 3, 1)
    r = R.backward(dy, x, None, None, None, res=torch.tensor([[[0.5], [0.0], [-3.0]]]))
    assert torch.isnan(r["dx"]).reshape(-1).tolist() == [False, True, False] and torch.isnan(r["dres"]).reshape(-1).tolist() == [False, True, False]
    assert not torch.isnan(R.backward(dy, x, None, None, None, act=False)["dx"]).any()
    assert not torch.isnan(R.backward_yardstick(torch.float32, dy, x, None, None, None)["dx"]).any()      # the yardstick is a result, not a reference
    c = R.Case(2, R.STREAM_S, 50, torch.bfloat16)
    cfg = c.config()
    frac = float(torch.isnan(R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"])["dx"]).double().mean())
    assert frac < 2e-4, frac


# ----------------------------------------------------------------------------------------------------------------- the yardstick
def _matrix():
    cases = []
    for dt in DTYPES:
        for cid, Cc in R.stream_channels(dt):
            cases.append(pytest.param(dt, R.STREAM_S, Cc, "network", id=f"{_name(dt)}-stream-{cid}"))
        for S, Cc in R.fused_shapes(dt):
            cases.append(pytest.param(dt, S, Cc, "network", id=f"{_name(dt)}-fused-S{S}-C{Cc}"))
        for S, Cc in R.option_shapes(dt):
            for opt in R.OPTIONS:
                if opt != "network":
                    cases.append(pytest.param(dt, S, Cc, opt, id=f"{_name(dt)}-S{S}-C{Cc}-{opt}"))
    return cases


def _below_half(got, ref, tol, what, worst):
    got, ref = R.determined(got, ref)
    pooled, loc = rel_err(got, ref), local_err(got, ref)[0]
    worst[what] = (pooled, loc)
    assert pooled < tol / 2 and loc < tol / 2, f"{what}: the fp32-compute yardstick stands at pooled {pooled:.3e}, local {loc:.3e}: above half of the kernels' bar {tol:.3e}"


@pytest.mark.parametrize("dtype,S,Cc,opt", _matrix())
def test_fp32_compute_yardstick_stays_below_half_the_kernel_bars(dtype, S, Cc, opt):
    """measured here: bf16 y <= 3.2e-3 local, dx <= 3.5e-3 local, dgamma / dbeta <= 7e-6; fp32: everything <= 1e-5 (dx at S = 2: 3e-6 .. 1e-5,
    on inputs of 1/16 amplitude - see instnorm_ref.Case)"""
    c = R.Case(2, S, Cc, dtype)
    cfg = c.config(**R.OPTIONS[opt])
    args = (c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"])
    kw = {"res": cfg["res"], "act": cfg["act"], "gadd": cfg["gadd"]}
    ref, yard = R.backward(*args, **kw), R.backward_yardstick(dtype, *args, **kw)
    ft, bt = R.fwd_tol(dtype), R.bwd_tol(dtype, S)
    worst = {}
    _below_half(yard["y"], ref["y"], ft, "y", worst)
    _below_half(yard["dx"], ref["dx"], bt, "dx", worst)
    if cfg["res"] is not None:
        _below_half(yard["dres"], ref["dres"], bt, "dres", worst)
    used = set(cfg["styles"]) if cfg["styles"] is not None else {0}
    for name in ("dgamma", "dbeta"):
        for s, (a, b) in enumerate(zip(yard[name], ref[name])):
            if a is not None and s in used:
                _below_half(a, b, bt, f"{name}[{s}]", worst)
    if opt == "network":      # the pair form has no options besides y given / recomputed, which the arithmetic does not see
        pa = (c.dy, c.x, c.xb, cfg["styles"], c.gam, c.bet, c.gam_b, c.bet_b)
        ref, yard = R.pair_backward(*pa), R.pair_backward_yardstick(dtype, *pa)
        _below_half(yard["y"], ref["y"], ft, "pair y", worst)
        for k in ("dxa", "dxb"):
            _below_half(yard[k], ref[k], bt, "pair " + k, worst)
        for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"):
            for s in range(2):
                _below_half(yard[k][s], ref[k][s], bt, f"pair {k}[{s}]", worst)
    print("yardstick", _name(dtype), S, Cc, opt, {k: f"{p:.1e}/{l:.1e}" for k, (p, l) in worst.items()})


def _rank1_matrix():
    return [pytest.param(dt, Cc, id=f"{_name(dt)}-C{Cc}") for dt in DTYPES for Cc in R.rank1_channels(dt)]


@pytest.mark.parametrize("dtype,Cc", _rank1_matrix())
def test_fp32_compute_yardstick_of_the_rank1_pair_stays_below_half_the_kernel_bars(dtype, Cc):
    """the inputs of the rank-1 pair cases of tests/test_hip_instnorm_forms.py (instnorm_ref.Rank1Case): dxa and the affine gradients below
    half of bwd_tol, the weight gradient below half of the 1e-4 test_instnorm_residual_pair_rank1_shortcut holds it to.  Measured here:
    dxa 6.5e-8 / 1.7e-3 pooled (fp32 / bf16), dW 3e-8 .. 6e-7 pooled, 5e-8 .. 3e-6 local"""
    c = R.Rank1Case(dtype, Cc)
    ref, yard = c.backward(), c.backward(work=torch.float32)
    assert 0 < c.n_unsure < 64 and not torch.isnan(ref["dxa"]).any() and not torch.isnan(ref["dxb"]).any()
    bt = R.bwd_tol(dtype, c.S)
    worst = {}
    _below_half(yard["dxa"].to(dtype), ref["dxa"], bt, "dxa", worst)
    for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"):
        for s in range(2):
            _below_half(yard[k][s], ref[k][s], bt, f"{k}[{s}]", worst)
    _below_half(yard["dw"].float(), ref["dw"], 1e-4, "dw", worst)
    # the terms add up instead of cancelling: what makes one bf16 ulp of one term small against the sum
    assert float((ref["dw"].abs() / ref["dw_terms"].abs().sum((0, 1))).min()) > 0.5
    print("yardstick rank-1", _name(dtype), Cc, {k: f"{p:.1e}/{l:.1e}" for k, (p, l) in worst.items()})


# ----------------------------------------------------------------------------------------------------------------- mutations
def _caught(got, ref, tol, what):
    got, ref = R.determined(got, ref)
    with pytest.raises(AssertionError) as ei:
        assert_parity(got, ref, tol, what)
    assert what in str(ei.value) and "worst element" in str(ei.value), str(ei.value)
    return local_err(got, ref)[1]


@pytest.fixture(scope="module", params=DTYPES, ids=_name)
def honest(request):
    """the honest result (the yardstick) and the float64 reference at the streaming ragged-tile shape: 2049 rows x 50 channels, LeakyReLU +
    residual + gadd, styles [1, 0]"""
    dt = request.param
    c = R.Case(2, R.STREAM_S, 50, dt)
    cfg = c.config(gadd=True)
    args = (c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"])
    kw = {"res": cfg["res"], "gadd": cfg["gadd"]}
    ref, yard = R.backward(*args, **kw), R.backward_yardstick(dt, *args, **kw)
    assert_parity(yard["y"], ref["y"], R.fwd_tol(dt), "honest y")
    assert_parity(*R.determined(yard["dx"], ref["dx"]), R.bwd_tol(dt, c.S), "honest dx")
    return dt, c, cfg, ref, yard


def test_last_row_zeroed_is_caught(honest):
    dt, c, cfg, ref, yard = honest
    for k, tol in (("y", R.fwd_tol(dt)), ("dx", R.bwd_tol(dt, c.S)), ("dres", R.bwd_tol(dt, c.S))):
        lost = ref[k].clone()
        lost[c.B - 1, c.S - 1] = 0
        idx = _caught(yard[k], lost, tol, f"{k}: last row zeroed")
        assert idx[:2] == (c.B - 1, c.S - 1)


def test_last_channel_of_the_ragged_tile_zeroed_is_caught(honest):
    dt, c, cfg, ref, yard = honest
    for k, tol in (("y", R.fwd_tol(dt)), ("dx", R.bwd_tol(dt, c.S))):
        lost = ref[k].clone()
        lost[..., c.C - 1] = 0
        assert _caught(yard[k], lost, tol, f"{k}: channel 49 zeroed")[2] == c.C - 1
    for k in ("dgamma", "dbeta"):
        lost = ref[k][1].clone()
        lost[c.C - 1] = 0
        assert _caught(yard[k][1], lost, R.bwd_tol(dt, c.S), f"{k}: channel 49 zeroed") == (c.C - 1,)


def test_swapped_styles_are_caught(honest):
    dt, c, cfg, ref, yard = honest
    swapped = R.backward(c.dy, c.x, cfg["styles"][::-1], cfg["gam"], cfg["bet"], res=cfg["res"], gadd=cfg["gadd"])
    _caught(yard["y"], swapped["y"], R.fwd_tol(dt), "y: styles swapped")
    _caught(yard["dx"], swapped["dx"], R.bwd_tol(dt, c.S), "dx: styles swapped")
    for k in ("dgamma", "dbeta"):
        _caught(yard[k][0], swapped[k][0], R.bwd_tol(dt, c.S), f"{k}: styles swapped")


def test_dropped_gadd_is_caught(honest):
    dt, c, cfg, ref, yard = honest
    plain = R.backward(c.dy, c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"])
    _caught(yard["dx"], plain["dx"], R.bwd_tol(dt, c.S), "dx: gadd dropped")


def test_statistics_of_the_neighbouring_channel_are_caught(honest):
    dt, c, cfg, ref, yard = honest
    x = c.x.double()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    for ch in (17, c.C - 1):      # an inner channel and the last one of the ragged tile, each with the statistics of the channel before it
        mu2, var2 = mu.clone(), var.clone()
        mu2[..., ch], var2[..., ch] = mu[..., ch - 1], var[..., ch - 1]
        wrong = R.forward(c.x, cfg["styles"], cfg["gam"], cfg["bet"], res=cfg["res"], moments=(mu2, var2))
        assert _caught(yard["y"], wrong, R.fwd_tol(dt), f"y: channel {ch} normalised with the statistics of channel {ch - 1}")[2] == ch

"""The float64 judge of the loss and Dice metric kernels (tests/seg_loss_ref.py) against everything else in the repository that states the
same arithmetic, its own gradient against finite differences, and the case list of tests/seg_loss_cases.py against the launchers of
csrc/training.hip: every instantiation the source lists is reached by a case.  CPU only."""
import numpy as np
import pytest
import torch

import seg_loss_cases as SC
import seg_loss_ref as R
from test_generalized_dice_cpu import gdice_focal_by_hand, score_by_hand, tiny_case


_crit = SC.criterion


def _existing_inputs(B, C, shape, seed):
    """the seeded recipe of test_hip_training._logits_labels, on the CPU in float64"""
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(B, C, *shape, generator=g)).double()
    labels = torch.randint(0, C, (B, 1) + tuple(shape), generator=g)
    if B > 1:
        labels[1][labels[1] == C - 1] = 0
    return logits, labels


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("include_background", [False, True])
@pytest.mark.parametrize("shape,squared", [((20, 24, 28), True), ((9, 7, 5), False), ((16, 16, 17), True)])
def test_reference_equals_forward_torch_on_the_existing_inputs(kind, include_background, shape, squared):
    """forward_torch evaluates its focal and CE terms in float32: the judge agrees with it to that precision, loss and gradient"""
    for w_type in (R.W_TYPES if kind == "gdice_focal" else ("square",)):
        cfg = R.Cfg(kind, include_background, squared and kind != "gdice_focal", 0.0, 1e-6, w_type=w_type)
        x, lab = _existing_inputs(2, 6, shape, 5)
        want, gwant = R.loss_and_grad(x, lab, cfg, 1.7)
        xin = x.clone().requires_grad_(True)
        got = _crit(cfg).forward_torch(xin, lab)
        (got * 1.7).backward()
        assert abs(float(got.detach()) - float(want)) <= 1e-6 * abs(float(want)), (float(got.detach()), float(want))
        assert float((xin.grad - gwant).norm() / gwant.norm()) < 1e-6


@pytest.mark.parametrize("w_type", R.W_TYPES)
@pytest.mark.parametrize("include_background", [True, False])
@pytest.mark.parametrize("absent", [None, "one", "all"])
def test_reference_equals_the_generalized_dice_focal_by_hand(absent, include_background, w_type):
    x, lab = tiny_case(absent)
    for nr, dr, gamma, ld, lo in ((0.0, 1e-6, 2.0, 1.0, 1.0), (1e-5, 1e-5, 0.5, 0.3, 2.5)):
        want = gdice_focal_by_hand(x, lab, include_background, w_type, nr, dr, gamma, ld, lo)
        got = float(R.loss(torch.from_numpy(x), torch.from_numpy(lab), R.Cfg("gdice_focal", include_background, False, nr, dr, gamma, ld, lo, w_type)))
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_reference_equals_the_dice_focal_background_case_by_hand():
    """the numpy restatement of test_dice_focal_include_background_semantics_by_hand (channel 0 leaves BEFORE the softmax), to 1e-12;
    and the dice_ce order (softmax over all channels, channel 0 dropped after) on the same numbers"""
    rng = np.random.default_rng(3)
    x = rng.normal(size=(1, 4, 3, 2, 2)) * 2
    lab = rng.integers(0, 4, size=(1, 1, 3, 2, 2))
    xs = x[:, 1:]
    t = np.stack([(lab[:, 0] == c) for c in range(1, 4)], 1).astype(np.float64)
    e = np.exp(xs - xs.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    ax = (2, 3, 4)
    dice = (1 - (2 * (p * t).sum(ax) + 0.0) / ((t * t).sum(ax) + (p * p).sum(ax) + 1e-6)).mean()
    ce = xs - xs * t + np.log1p(np.exp(-np.abs(xs))) + np.maximum(-xs, 0)
    z = -xs * (2 * t - 1)
    logsig = -(np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0))
    focal = (np.exp(2.0 * logsig) * ce).reshape(1, 3, -1).mean(-1).mean()
    got = float(R.loss(torch.from_numpy(x), torch.from_numpy(lab), R.Cfg("dice_focal", False, True, 0.0, 1e-6)))
    assert abs(got - (dice + focal)) <= 1e-12 * abs(dice + focal)
    ea = np.exp(x - x.max(1, keepdims=True))
    pa = ea / ea.sum(1, keepdims=True)
    dice_all = (1 - 2 * (pa[:, 1:] * t).sum(ax) / (t.sum(ax) + (pa[:, 1:] ** 2).sum(ax) + 1e-6)).mean()
    nll = -np.log(np.take_along_axis(pa, lab, 1)).mean()
    got = float(R.loss(torch.from_numpy(x), torch.from_numpy(lab), R.Cfg("dice_ce", False, True, 0.0, 1e-6)))
    assert abs(got - (dice_all + nll)) <= 1e-12 * abs(dice_all + nll)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("include_background", [False, True])
def test_reference_gradient_against_finite_differences(kind, include_background):
    x, lab = tiny_case("one")
    x, lab = torch.from_numpy(x), torch.from_numpy(lab)
    for sq, w_type, gamma in ((False, "square", 2.0), (True, "simple", 0.5), (False, "uniform", 3.5)):
        cfg = R.Cfg(kind, include_background, sq, 1e-5, 1e-5, gamma, 0.7, 1.3, w_type)
        _, grad = R.loss_and_grad(x, lab, cfg, -2.5)
        fd, h = torch.zeros_like(x), 1e-6
        for i in range(x.numel()):
            d = torch.zeros(x.numel(), dtype=torch.float64)
            d[i] = h
            d = d.reshape(x.shape)
            fd.reshape(-1)[i] = -2.5 * (R.loss(x + d, lab, cfg) - R.loss(x - d, lab, cfg)) / (2 * h)
        assert float((grad - fd).abs().max()) < 1e-8 * max(1.0, float(grad.abs().max())), (cfg, float((grad - fd).abs().max()))
        if kind == "dice_focal" and not include_background:
            assert torch.equal(grad[:, 0], torch.zeros_like(grad[:, 0]))      # channel 0 is outside the softmax support and the focal term


def test_reference_stable_forms_at_extreme_logits():
    """x = -80 with t = 0: the literal x - x t + softplus(-x) cancels to 0 in float64, the stable form keeps log1p(e^-80); 1e4 overflows nothing"""
    x = torch.tensor([-80.0, 80.0, -1e4, 1e4, 0.0], dtype=torch.float64)
    for t in (0.0, 1.0):
        f = R.focal_elements(x, torch.full_like(x, t), 2.0)
        assert bool(torch.isfinite(f).all()) and bool((f >= 0).all())
    f0 = R.focal_elements(x[:1], torch.zeros(1, dtype=torch.float64), 0.0)
    assert float(f0) == pytest.approx(np.log1p(np.exp(-80.0)), rel=1e-15) and float(f0) > 0
    assert float(R.focal_elements(x[3:4], torch.zeros(1, dtype=torch.float64), 0.0)) == 1e4


def test_reference_metric_against_the_restatements():
    """counts -> Dice and generalized score against training/metrics.py and score_by_hand on tie-rich logits; an all-zero one-hot row counts
    for the prediction only"""
    from mi_seg_amd.training.metrics import as_discrete_argmax_onehot, as_discrete_onehot, compute_generalized_dice, dice_metric
    g = torch.Generator().manual_seed(4)
    C = 5
    logits = torch.round(2 * torch.randn(2, C, 300, generator=g))
    lab = torch.randint(0, C, (2, 1, 300), generator=g)
    lab[1][lab[1] == 3] = 0
    assert torch.equal(R.argmax_first(logits), logits.argmax(1))
    counts = R.metric_counts(logits, R.one_hot(lab, C))
    pred1h, lab1h = as_discrete_argmax_onehot(logits, C), as_discrete_onehot(lab, C)
    want = dice_metric(pred1h, lab1h).double()
    got = R.dice_of_counts(counts)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got).any())
    assert torch.allclose(got[~torch.isnan(got)], want[~torch.isnan(want)], rtol=1e-6, atol=0)
    for inc in (True, False):
        for w_type in R.W_TYPES:
            s = R.generalized_score_of_counts(counts, inc, w_type)
            assert torch.allclose(s, compute_generalized_dice(pred1h, lab1h, inc, w_type).double(), rtol=1e-6, atol=0)
            assert np.allclose(s.numpy(), score_by_hand(logits.argmax(1).numpy(), lab[:, 0].numpy(), C, inc, w_type), rtol=1e-12, atol=0)
    out = lab.clone()
    out[0, 0, :50] = C
    out[0, 0, 50:60] = -1
    c2 = R.metric_counts(logits, R.one_hot(out, C))
    assert torch.equal(c2[..., 1], counts[..., 1]) and int(c2[0, :, 2].sum()) == 240 and torch.equal(c2[1], counts[1])
    # rule 7: nothing labelled and nothing predicted among the kept classes -> 1; something predicted -> 0
    z = torch.zeros(2, 3, 3, dtype=torch.int64)
    z[0, 0, 1] = z[1, 0, 1] = 7
    z[1, 2, 1] = 1
    assert R.generalized_score_of_counts(z, False, "square").tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ launchers and case list
def test_launcher_restatement_matches_the_source():
    fwd, bwd, labels = SC.launcher_forms()
    assert len(fwd) == len(set(fwd)) and set(fwd) == SC.FWD_FORMS, fwd
    assert len(bwd) == len(set(bwd)) and set(bwd) == SC.BWD_FORMS, bwd
    assert sorted(labels) == sorted(SC.LABEL_DTYPES), labels
    assert SC.fwd_form(8, 500, 0) == (8, 4) and SC.fwd_form(8, 500, 4) == (8, 1) and SC.fwd_form(8, 501, 0) == (8, 1) and SC.fwd_form(9, 500, 0) == (16, 1)
    assert SC.form("gdice_focal", 3, 500, 0, 0) == (8, 4, True) and SC.form("dice_ce", 3, 500, 0, 8) == (8, 1, False)
    assert SC.form("dice_focal", 16, 512, 0, 0) == (16, 1, False)
    assert [SC.nblk(s) for s in (1, 1024, 1025, 65 * 1024 + 3)] == [1, 1, 2, 66]
    assert [SC.metric_grid_x(s) for s in (1, 2048, 2049, 2048 * 2048, 2048 * 2048 + 5)] == [1, 1, 2, 2048, 2048]
    assert SC.metric_trips(2048 * 2048) == 8 and SC.metric_trips(2048 * 2048 + 5) == 9


def test_every_loss_instantiation_is_reached_by_a_case():
    fwd, bwd, labels = SC.launcher_forms()
    reached_fwd = {(c.fwd_form(), c.label_dtype) for c in SC.CASES}
    for f in fwd:
        for dt in labels:
            assert (f, dt) in reached_fwd, f"no case runs seg_loss_fwd_kernel<{dt}, {f[0]}, {f[1]}>"
    reached_bwd = {(c.bwd_form(), c.label_dtype, c.cfg.kind) for c in SC.CASES}
    for f in bwd:
        kinds = ("gdice_focal",) if f[2] else ("dice_focal", "dice_ce")
        for kind in kinds:
            for dt in labels:
                assert (f, dt, kind) in reached_bwd, f"no {kind} case runs seg_loss_bwd_kernel<{dt}, {f[0]}, {f[1]}, {f[2]}>"
    # the scalar form is reached by the pointer alone, and gscale == NULL by a backward
    assert any(c.misaligned and c.S % 4 == 0 and c.C <= 8 and c.bwd_form()[1] == 1 for c in SC.CASES)
    assert any(c.upstream is None for c in SC.CASES)


def test_the_bars_hold_for_float32_arithmetic_on_every_case():
    """the float32 torch composition is within half of each bar of the float64 judge on every case not named in WIDENED, so the GPU file holds
    the kernels to the plain bars there; a case that needs the max(bar, 2 x error) rule has to be named, which makes the wider bound a decision"""
    ids = {c.id for c in SC.CASES}
    assert SC.WIDENED <= ids and (SC.LOSS_BAR, SC.GRAD_BAR) == (1e-5, 1e-4)
    for c in SC.CASES:
        if c.id in SC.WIDENED:
            continue
        lab = SC.make_labels(c)
        e = SC.composition_errors(SC.make_logits(c, lab), lab, c.cfg, c.upstream)
        assert 2 * max(e["loss"], e["other"], e["sums"]) <= SC.LOSS_BAR and 2 * e["grad_local"] <= SC.GRAD_BAR, (c.id, e)
        j = SC.judged(c.id, SC.make_logits(c, lab), lab, c.cfg, c.upstream) if c.S <= 4 else None
        assert j is None or (j["loss_bound"], j["other_bound"], j["sums_bound"], j["grad_pooled_bound"], j["grad_local_bound"]) == (1e-5, 1e-5, 1e-5, 1e-4, 1e-4)


def test_the_case_list_covers_the_edges():
    by = {}
    for c in SC.CASES:
        by.setdefault(c.id.split("-")[0], []).append(c)
    for C in (2, 3, 8, 9, 16):
        for kind in R.KINDS:
            got = {(c.cfg.include_background, c.cfg.squared_pred, c.cfg.w_type) for c in by["classes"] if c.C == C and c.cfg.kind == kind}
            bgs, sqs = {g[0] for g in got}, {g[1] for g in got}
            assert bgs == {False, True} and (kind == "gdice_focal" or sqs == {False, True})
            if kind == "gdice_focal" and C in (3, 9):
                assert {g[2] for g in got} == set(R.W_TYPES)
    for C in (3, 9):
        assert {c.S for c in by["edge"] if c.C == C} == {1, 3, 4, 1020, 1023, 1024, 1025, 1028, 2052}
    assert {(c.S, c.B, c.C) for c in by["wrap"]} == {(65 * 1024 + 4, 1, 3), (65 * 1024 + 3, 1, 3)} and all(SC.nblk(c.S) > 64 for c in by["wrap"])
    assert {c.B for c in by["batch"]} == {1, 3, 17, 64} and all((c.S, c.C) == (36, 4) for c in by["batch"])
    assert {c.cfg.gamma for c in by["gamma"]} == {0.0, 0.5, 2.0, 3.5}
    assert {(c.cfg.smooth_nr, c.cfg.smooth_dr) for c in by["smooth"]} == {(1e-5, 1e-5), (1.0, 1.0)}
    assert {(c.cfg.lambda_dice, c.cfg.lambda_other) for c in by["lambda"]} == {(0.0, 1.0), (1.0, 0.0), (0.3, 2.5)}
    assert {c.upstream for c in by["upstream"]} == {1.0, -2.5, 0.0, None}
    assert {c.labels for c in by["labels"]} == {"absent_one", "absent_all", "background_only", "single_class"}
    assert {c.logits for c in by["logits"]} == {"equal", "times30", "times100", "focal_corner", "voxel_1e4"}
    m = SC.METRIC_CASES
    assert {(c.C, c.B, c.S) for c in m if c.id.startswith("grid")} == {(C, B, S) for C in (1, 2, 9, 33, 64) for B in (1, 3) for S in (1, 255, 256, 257, 2049)}
    assert [SC.metric_trips(c.S) for c in m if c.id == "capped-grid"] == [9] and max(SC.metric_trips(c.S) for c in m if c.id != "capped-grid") <= 8
    assert {c.label_dtype for c in m} == set(SC.LABEL_DTYPES)

"""CPU tests of flip test-time augmentation and model ensembling: the torch restatement of the fold
(hip/ops.py::ensemble_accumulate_torch, the oracle of the GPU tests) against a hand-written float64 computation, the vote rules, the flip
sets, the EnsembleInferer against the explicit loop, the MONAI-style callables and the command-line surface."""
import argparse
from functools import partial

import numpy as np
import pytest
import torch

import ensemble_ref as R

SHAPE = (2, 3, 2, 3, 5)
EPS = 2.0 ** -24


def _ops():
    from mi_seg_amd.hip import ops
    return ops


def _run(members, kind, scale=None, fn=None):
    """the members folded one after the other through the product's CPU path: first on the first, the scale on the last"""
    ops = _ops()
    fn = fn or ops.ensemble_accumulate
    acc = torch.full(members[0][0].shape, float("nan"))
    for k, (src, flip, w) in enumerate(members):
        out = fn(src, acc, flip=flip, kind=kind, weight=w, first=k == 0, out_scale=scale if k == len(members) - 1 else None)
        assert out is acc
    return acc


@pytest.mark.parametrize("flip", R.FLIPS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_against_the_hand_written_float64_computation(kind, flip):
    g = torch.Generator().manual_seed(1 + 8 * R.KINDS.index(kind) + R.FLIPS.index(flip))
    # dyadic logits and power-of-two weights: every fp32 step is exact, so kinds 0 and 2 must equal the float64 result to the bit
    exact = [(torch.randint(-16, 17, SHAPE, generator=g).float() / 4, flip, w) for w in (0.5, (1.0, 2.0, 0.25), 2.0)]
    got = _run(exact, kind, scale=0.25)
    want, _ = R.fold64([(s.numpy(), f, w) for s, f, w in exact], kind, scale=0.25)
    if kind != "mean_prob":
        assert np.array_equal(got.numpy().astype(np.float64), want)
    # general weights: N members make N products, N - 1 sums, the scale and its own rounding: (N + 3) * 2^-24 * s * sum |w t| per element;
    # mean_prob adds the fp32 softmax's own error - the difference x - max (exp turns its rounding into |x - max| * 2^-24 relative, and
    # |x - max| is at most the spread of the logits), exp, C sums, the reciprocal and the product: spread + C + 3 more units
    N, C = 3, SHAPE[1]
    members = [(torch.randn(SHAPE, generator=g) * 3, flip, w) for w in (0.3, (1.7, 0.9, 0.4), 1.1)]
    scale = 1.0 / (0.3 + 1.1 + np.array([1.7, 0.9, 0.4]))
    got = _run(members, kind, scale=scale)
    want, mag = R.fold64([(s.numpy(), f, w) for s, f, w in members], kind, scale=scale)
    spread = int(np.ceil(max(float(s.max() - s.min()) for s, _, _ in members)))      # bounds |x - max| of every voxel
    units = N + 3 + (spread + C + 3 if kind == "mean_prob" else 0)
    err = np.abs(got.numpy().astype(np.float64) - want)
    assert (err <= units * EPS * mag).all(), float((err / (EPS * mag + 1e-300)).max())
    assert float(err.max()) > 0 or kind == "vote"
    # the restatement is what CPU tensors take, and a first fold never reads the accumulator
    again = _run(members, kind, scale=scale, fn=_ops().ensemble_accumulate_torch)
    assert torch.equal(got, again) and not bool(torch.isnan(got).any())
    if flip != (False, False, False):
        assert not torch.equal(got, _run([(s, (False, False, False), w) for s, _, w in members], kind, scale=scale))


def test_vote_ties_take_the_lowest_class_and_nan_follows_first_max_argmax():
    ops = _ops()
    shape = (1, 4, 2, 2, 3)
    votes = []
    for cls in (2, 1, 1, 2):                                  # two members for class 2, two for class 1: a tie between the members
        x = torch.zeros(shape)
        x[:, cls] = 1.0
        votes.append((x, (False, False, False), 1.0))
    acc = _run(votes, "vote")
    assert torch.equal(acc[0, :, 0, 0, 0], torch.tensor([0.0, 2.0, 2.0, 0.0]))
    assert bool((ops.first_max_argmax(acc[0]) == 1).all())
    tied = torch.zeros(shape)
    tied[:, 1:] = 5.0                                         # exact ties inside one member: the first maximum wins
    nan0, nan2 = torch.randn(shape), torch.randn(shape)
    nan0[:, 0] = float("nan")                                  # a NaN in channel 0 gives class 0
    nan2[:, 2] = float("nan")                                  # a NaN in a later channel never wins
    for x in (tied, nan0, nan2):
        acc = _run([(x, (False, False, False), 7.0)], "vote")        # (the weight is ignored)
        want = torch.stack([(ops.first_max_argmax(x[0]) == c) for c in range(4)]).float()[None]
        assert torch.equal(acc, want)
    assert bool((_run([(tied, (False,) * 3, 1.0)], "vote")[0, 1] == 1).all()) and bool((_run([(nan0, (False,) * 3, 1.0)], "vote")[0, 0] == 1).all())
    assert bool((_run([(nan2, (False,) * 3, 1.0)], "vote")[0, 2] == 0).all())


def test_argument_checks():
    ops = _ops()
    src, acc = torch.zeros(SHAPE), torch.zeros(SHAPE)
    for bad in (dict(kind="nope"), dict(flip=(True, False)), dict(weight=-1.0), dict(weight=float("inf")), dict(weight=(1.0, 2.0)),
                dict(out_scale=float("nan")), dict(out_scale=(1.0,) * 4)):
        with pytest.raises(ValueError, match="ensemble_accumulate"):
            ops.ensemble_accumulate(src, acc, **bad)
    for a, b in ((src.double(), acc), (src, acc[:, :2]), (src[0], acc[0]), (src.transpose(3, 4), acc.transpose(3, 4)), (torch.zeros(1, 65, 1, 1, 2),) * 2):
        with pytest.raises(ValueError, match="ensemble_accumulate"):
            ops.ensemble_accumulate(a, b)


def test_tta_flip_sets_order_and_size():
    from mi_seg_amd.training.ensemble import tta_flip_sets
    F, T = False, True
    assert tta_flip_sets(()) == [(F, F, F)]
    assert tta_flip_sets((1,)) == [(F, F, F), (F, T, F)]
    assert tta_flip_sets((0, 2)) == tta_flip_sets([2, 0]) == [(F, F, F), (T, F, F), (F, F, T), (T, F, T)]
    full = tta_flip_sets((0, 1, 2))
    assert len(full) == 8 and len(set(full)) == 8 and full[0] == (F, F, F) and full == R.FLIPS
    for bad in ((3,), (-1,), (0, 0)):
        with pytest.raises(ValueError):
            tta_flip_sets(bad)


class _Toy:
    """a predictor that is not flip-equivariant: a ramp along W times the window plus a roll along H, two channels"""

    def __init__(self, k):
        self.k = k

    def __call__(self, x):
        ramp = torch.linspace(0.5, 2.0, x.shape[-1]) + self.k
        return torch.cat([x * ramp + torch.roll(x, 1, -2), torch.roll(x, 2, -3) - 0.25 * ramp * self.k], 1)


@pytest.mark.parametrize("blend", ["constant", "gaussian"])
def test_ensemble_inferer_equals_the_explicit_loop_on_cpu(blend):
    from mi_seg_amd.training.ensemble import EnsembleInferer, tta_flip_sets
    from mi_seg_amd.training.inferer import sliding_window_inference
    vol = torch.randn(1, 1, 20, 17, 13, generator=torch.Generator().manual_seed(3))
    roi, sw = (16, 8, 8), 3
    run = lambda x, p: sliding_window_inference(x, roi, sw, p, overlap=0.5, mode=blend)
    toys = [_Toy(1.0), _Toy(2.0), _Toy(3.0)]
    plain = run(vol, toys[0])
    one = EnsembleInferer(toys[0], roi, sw, 0.5, infer_mode=blend)
    assert one.members == 1 and torch.equal(one(vol), plain)                       # a single member: the plain inferer's result
    assert torch.equal(EnsembleInferer([toys[0]], roi, sw, 0.5, flips=tta_flip_sets(()), infer_mode=blend)(vol, modalities=None), plain)
    assert not torch.equal(run(torch.flip(vol, [4]), toys[0]).flip(4), plain)      # the toy is not flip-equivariant
    for predictors, axes, weights in ((toys[:1], (0, 1, 2), None), (toys[:2], (0, 2), None), (toys, (), None), (toys, (1,), (0.3, 1.7, 0.9))):
        flips = tta_flip_sets(axes)
        for mode in ("mean_logits", "vote"):
            inf = EnsembleInferer(predictors, roi, sw, 0.5, flips=flips, mode=mode, weights=weights, infer_mode=blend)
            got = inf(vol)
            assert inf.members == len(predictors) * len(flips) and got.dtype == torch.float32 and got.shape == plain.shape
            assert torch.equal(got, R.loop_reference(vol, predictors, flips, run, mode, weights)), (len(predictors), axes, mode)
        prob = EnsembleInferer(predictors, roi, sw, 0.5, flips=flips, mode="mean_prob", weights=weights, infer_mode=blend)(vol)
        assert torch.allclose(prob.sum(1), torch.ones(()), atol=1e-5)
    # a volume smaller than the roi is padded by the inferer: the un-padded (non-contiguous) logits fold just the same
    small = vol[:, :, :12]
    got = EnsembleInferer(toys[:2], roi, sw, 0.5, flips=tta_flip_sets((0,)), infer_mode=blend)(small)
    assert torch.equal(got, R.loop_reference(small, toys[:2], tta_flip_sets((0,)), run))
    with pytest.raises(ValueError):
        EnsembleInferer(toys, roi, sw, mode="nope")
    with pytest.raises(ValueError):
        EnsembleInferer([], roi, sw)


def test_mean_and_vote_ensemble_callables():
    from mi_seg_amd.training.ensemble import MeanEnsemble, VoteEnsemble
    g = torch.Generator().manual_seed(5)
    preds = [torch.randn(3, 4, 5, 6, generator=g) for _ in range(4)]
    got = MeanEnsemble()(preds)
    want = ((preds[0] + preds[1]) + preds[2] + preds[3]) * 0.25
    assert got.shape == preds[0].shape and torch.equal(got, want) and torch.equal(MeanEnsemble()(torch.stack(preds)), want)
    w = [1.0, 2.0, 0.5, 0.5]
    monai = (torch.stack(preds) * torch.tensor(w).reshape(4, 1, 1, 1, 1)).mean(0) / torch.tensor(w).mean()      # MONAI's own expression
    assert torch.allclose(MeanEnsemble(weights=w)(preds), monai, atol=1e-6)
    wc = torch.rand(4, 3, generator=g) + 0.1
    monai = (torch.stack(preds) * wc.reshape(4, 3, 1, 1, 1)).mean(0) / wc.mean(0).reshape(3, 1, 1, 1)
    assert torch.allclose(MeanEnsemble(weights=wc)(preds), monai, atol=1e-6)
    batched = MeanEnsemble()([p[None] for p in preds])
    assert batched.shape == (1, 3, 4, 5, 6) and torch.equal(batched[0], want)
    maps = [torch.randint(0, 3, (1, 4, 5, 6), generator=g) for _ in range(4)]
    voted = VoteEnsemble(num_classes=3)(maps)
    counts = torch.stack([torch.stack([(m[0] == c) for m in maps]).sum(0) for c in range(3)])
    assert voted.shape == (1, 4, 5, 6) and voted.dtype == maps[0].dtype and torch.equal(voted[0], counts.argmax(0))      # (argmax of integer counts: ties to the lowest)
    onehot = [torch.stack([(m[0] == c) for c in range(3)]).float() for m in maps]
    binary = VoteEnsemble()(onehot)
    assert torch.equal(binary, torch.round(torch.stack(onehot).mean(0)))                                           # MONAI's own expression
    with pytest.raises(ValueError):
        MeanEnsemble(weights=[1.0, 2.0])(preds)


def _parser():
    from mi_seg_amd.utils.parser import add_data_argparse_args, add_model_argparse_args, add_tune_argparse_args
    p = argparse.ArgumentParser()
    add_tune_argparse_args(add_data_argparse_args(add_model_argparse_args(p)))
    return p


def test_command_line_surface():
    from mi_seg_amd.networks.lightning_monai import LitMonai
    from mi_seg_amd.training import predict
    from mi_seg_amd.training.ensemble import EnsembleInferer, tta_flip_sets
    a = _parser().parse_args([])
    assert a.infer_tta_flips is None and a.ensemble_mode == "mean_logits"
    # every default that was there stays
    assert (a.model_name, a.roi_x, a.feature_size, a.hidden_size, a.mlp_dim, a.num_heads, a.pos_embed) == ("unetr", 96, [16], 768, 3072, 12, "perceptron")
    assert (a.infer_overlap, a.sw_batch_size, a.infer_cpu, a.infer_mode, a.infer_sigma_scale, a.infer_padding_mode) == (0.5, 1, False, "constant", 0.125, "constant")
    assert (a.criterion, a.optim_name, a.lr, a.reg_weight, a.scheduler, a.iters_to_accumulate) == ("dice_focal", "adamw", 1e-4, 1e-5, "reduce_on_plateau", 1)
    b = _parser().parse_args(["--infer_tta_flips", "0", "2", "--ensemble_mode", "vote"])
    assert b.infer_tta_flips == [0, 2] and b.ensemble_mode == "vote"
    assert _parser().parse_args(["--infer_tta_flips"]).infer_tta_flips == []
    for bad in (["--infer_tta_flips", "3"], ["--ensemble_mode", "nope"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(bad)
    p = predict.build_parser().parse_args([])
    assert p.ensemble_checkpoints == [] and p.infer_tta_flips is None and p.ensemble_mode == "mean_logits" and p.checkpoint == ""
    p = predict.build_parser().parse_args(["--ensemble_checkpoints", "b.pt", "c.pt", "--infer_tta_flips", "0", "1", "2"])
    assert p.ensemble_checkpoints == ["b.pt", "c.pt"] and p.infer_tta_flips == [0, 1, 2]
    model = ["--model_name=unet", "--out_channels=3", "--roi_x=32", "--roi_y=24", "--roi_z=16", "--infer_overlap=0.25", "--sw_batch_size=4"]
    plain = LitMonai.from_argparse_args(_parser().parse_args(model))
    assert isinstance(plain.model_inferer, partial) and plain.model_inferer.keywords["mode"] == "constant"      # None leaves the object as it is
    lit = LitMonai.from_argparse_args(_parser().parse_args(model + ["--infer_tta_flips", "0", "2", "--ensemble_mode=mean_prob", "--infer_mode=gaussian"]))
    inf = lit.model_inferer
    assert isinstance(inf, EnsembleInferer) and inf.flips == tta_flip_sets((0, 2)) and inf.mode == "mean_prob" and inf.members == 4
    assert inf.predictors == [lit.model] and tuple(inf.roi_size) == (32, 24, 16) and inf.sw_batch_size == 4 and inf.overlap == 0.25
    assert (inf.keywords["mode"], inf.keywords["sigma_scale"], inf.keywords["padding_mode"]) == ("gaussian", 0.125, "constant")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mean_prob_class_map_against_float64(seed):
    """8 members of randn * 3 logits at [2, 5, 6, 7, 9]: the fp32 restatement's class map equals the float64 one wherever the float64 top-two
    gap is >= 1e-5 (at most 1 % of the voxels fall under that gap)"""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    members = [(torch.randn(2, 5, 6, 7, 9, generator=g) * 3, R.FLIPS[k], 1.0) for k in range(8)]
    got = _run(members, "mean_prob", scale=0.125)
    want, _ = R.fold64([(s.numpy(), f, w) for s, f, w in members], "mean_prob", scale=0.125)
    left_out = R.class_map_agrees(got, want)
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print(f"mean_prob seed {seed}: fp32 restatement against float64: largest error {err:.3e}, share under the 1e-5 gap {left_out:.4%}")
    spread = int(np.ceil(max(float(s.max() - s.min()) for s, _, _ in members)))
    assert err <= (8 + 3 + spread + 5 + 3) * EPS          # the bound of the hand-built case with sum |w t| s <= 1: probabilities, weight 1, scale 1/8
    acc64 = torch.empty(2, 5, 6, 7, 9, dtype=torch.float64)
    for k, (s, f, w) in enumerate(members):                       # the restatement on float64 tensors is the float64 restatement
        ops.ensemble_accumulate_torch(s.double(), acc64, flip=f, kind="mean_prob", first=k == 0, out_scale=0.125 if k == 7 else None)
    assert np.allclose(acc64.numpy(), want, rtol=0, atol=1e-14)

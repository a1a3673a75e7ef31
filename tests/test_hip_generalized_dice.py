"""GPU tests of the generalized Dice focal criterion (MISEG_LOSS_GDICE_FOCAL) and the generalized Dice score (miseg_dice_metric's `gdice`
output): DESIGN.md section 7.4, reference utils/training_utils.py:26-33 and tune.py:124-129,208-213.  MONAI is absent (parity unpinned): the
judges are the torch restatement in float64 (training/losses.py, training/metrics.py) and the numpy restatement of
test_generalized_dice_cpu.py.  The bars are the ones test_hip_training.py applies to the sibling kinds."""
import argparse

import numpy as np
import pytest
import torch

from conftest import rel_err
from parity import assert_parity
from mi_seg_amd.training.losses import DiceCELoss, DiceFocalLoss, GeneralizedDiceFocalLoss, GeneralizedDiceLoss
from mi_seg_amd.training.metrics import GeneralizedDiceScore, compute_generalized_dice, generalized_dice_from_logits
from test_generalized_dice_cpu import W_TYPES, gdice_focal_by_hand, tiny_case
from test_hip_training import _logits_labels, _small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("w_type", W_TYPES)
@pytest.mark.parametrize("include_background", [False, True])
@pytest.mark.parametrize("shape,label_dtype", [((20, 24, 28), torch.float32), ((9, 7, 5), torch.int64), ((16, 16, 17), torch.uint8)])
def test_fused_generalized_dice_focal_matches_torch(w_type, include_background, shape, label_dtype):
    """the grid of test_fused_seg_loss_matches_torch (B = 2, C = 6, 3 randn logits, the last class absent from sample 1, upstream gradient
    1.7) crossed with include_background and the weight type: loss within 1e-5 relative and d(loss)/d(logits) within 1e-4 relative L2 of
    the float64 restatement, a second forward bit-identical.  (16, 16, 17) and (9, 7, 5) take the scalar instantiation, (20, 24, 28) the
    vector one."""
    crit = GeneralizedDiceFocalLoss(include_background=include_background, to_onehot_y=True, softmax=True, w_type=w_type, smooth_nr=0.0, smooth_dr=1e-6)
    logits, labels = _logits_labels(2, 6, shape, 5, label_dtype)
    loss = crit(logits, labels)
    assert loss.dim() == 0 and loss.is_cuda
    (loss * 1.7).backward()
    ref_in = logits.detach().double().cpu().requires_grad_(True)
    ref = crit.forward_torch(ref_in, labels.cpu())
    (ref * 1.7).backward()
    print(f"gdice_focal {w_type} bg={include_background} {shape}: loss {float(loss):.9g} ref {float(ref):.9g} rel {abs(float(loss) - float(ref)) / abs(float(ref)):.3g}"
          f" dlogits rel_err {rel_err(logits.grad, ref_in.grad):.3g}")
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert_parity(logits.grad, ref_in.grad, 1e-4, "d loss / d logits against float64")
    l2 = crit(logits.detach(), labels)
    assert torch.equal(l2, loss.detach())
    # the generalized Dice term alone takes the same kernels with lambda_focal = 0
    gdl = GeneralizedDiceLoss(include_background=include_background, to_onehot_y=True, softmax=True, w_type=w_type, smooth_nr=0.0, smooth_dr=1e-6)
    lg = gdl(logits.detach(), labels)
    rg = gdl.forward_torch(logits.detach().double().cpu(), labels.cpu())
    assert lg.is_cuda and abs(float(lg) - float(rg)) <= 1e-5 * abs(float(rg))


@pytest.mark.parametrize("C", [11, 16])
def test_fused_generalized_dice_focal_wide(C):
    """more than 8 classes: the 16-channel instantiation, same bars"""
    crit = GeneralizedDiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True)
    logits, labels = _logits_labels(2, C, (12, 10, 9), 7, torch.int32)
    loss = crit(logits, labels)
    (loss * 1.7).backward()
    ref_in = logits.detach().double().cpu().requires_grad_(True)
    ref = crit.forward_torch(ref_in, labels.cpu())
    (ref * 1.7).backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert_parity(logits.grad, ref_in.grad, 1e-4, "d loss / d logits against float64")


@pytest.mark.parametrize("w_type", W_TYPES)
@pytest.mark.parametrize("include_background", [False, True])
@pytest.mark.parametrize("absent", [None, "one", "all"])
def test_generalized_dice_focal_by_hand_on_the_device(absent, include_background, w_type):
    """the tiny case of test_generalized_dice_cpu.py through the kernel: 2e-6 relative to the numpy float64 restatement"""
    x, lab = tiny_case(absent)
    want = gdice_focal_by_hand(x, lab, include_background, w_type, 0.0, 1e-6)
    crit = GeneralizedDiceFocalLoss(include_background=include_background, to_onehot_y=True, softmax=True, w_type=w_type, smooth_nr=0.0, smooth_dr=1e-6)
    lk = crit(torch.from_numpy(x).float().to(DEV), torch.from_numpy(lab).to(DEV))
    assert lk.is_cuda
    assert abs(float(lk) - want) < 2e-6 * abs(want), (float(lk), want)


@pytest.mark.parametrize("kind", ["dice_focal", "dice_ce"])
@pytest.mark.parametrize("shape", [(20, 24, 28), (96, 96, 96)])
def test_existing_kinds_did_not_move(kind, shape):
    """dice_focal / dice_ce as LitMonai builds them, on seeded inputs: run to run bit-identical and within the sibling test's bars of the
    float64 restatement (DESIGN.md section 7.4 records the bitwise comparison with the previous build)"""
    cls = DiceFocalLoss if kind == "dice_focal" else DiceCELoss
    crit = cls(include_background=False, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=0.0, smooth_dr=1e-6)
    B = 2 if shape[0] < 96 else 1
    logits, labels = _logits_labels(B, 6, shape, 21, torch.int32)
    loss = crit(logits, labels)
    (loss * 1.7).backward()
    ref_in = logits.detach().double().cpu().requires_grad_(True)
    ref = crit.forward_torch(ref_in, labels.cpu())
    (ref * 1.7).backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert_parity(logits.grad, ref_in.grad, 1e-4, "d loss / d logits against float64")
    again = logits.detach().clone().requires_grad_(True)
    l2 = crit(again, labels)
    (l2 * 1.7).backward()
    assert torch.equal(l2.detach(), loss.detach()) and torch.equal(again.grad, logits.grad)


def _nan_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


@pytest.mark.parametrize("B", [1, 2, 3])
def test_generalized_dice_score_kernel(B):
    """the input of test_dice_metric_kernel (exact ties included): the score of the extended miseg_dice_metric against compute_generalized_dice
    on the one-hot volumes, and the Dice of the same call against today's dice_from_logits, bit for bit"""
    from mi_seg_amd.training.metrics import as_discrete_argmax_onehot, as_discrete_onehot, dice_from_logits
    logits, labels = _logits_labels(B, 6, (17, 19, 23), 9, torch.float32)
    logits = logits.detach()
    logits[0, 2] = logits[0, 4]
    plain = dice_from_logits(logits, labels, 6)
    pred, lab = as_discrete_argmax_onehot(logits.cpu(), 6), as_discrete_onehot(labels.cpu(), 6)
    for inc in (True, False):
        for w_type in W_TYPES:
            dice, got = generalized_dice_from_logits(logits, labels, 6, inc, w_type, with_dice=True)
            assert got.is_cuda and got.shape == (B,) and got.dtype == torch.float32
            want = compute_generalized_dice(pred, lab, include_background=inc, weight_type=w_type)
            assert torch.allclose(got.cpu(), want, rtol=1e-6, atol=0), (inc, w_type, got.cpu(), want)
            assert _nan_equal(dice, plain)
            assert torch.equal(generalized_dice_from_logits(logits, labels, 6, inc, w_type), got)


def test_generalized_dice_score_kernel_empty_cases():
    """rule 7 on the device: empty label and empty prediction (1), empty label and a non-empty prediction (0), a perfect prediction (1)"""
    C = 4
    lab = torch.zeros(3, 1, 5, 6, 7, dtype=torch.int64)
    pred = torch.zeros(3, 5, 6, 7, dtype=torch.int64)
    pred[1, 0, 0, 0] = 2
    g = torch.Generator().manual_seed(1)
    lab[2, 0] = torch.randint(0, C, (5, 6, 7), generator=g)
    pred[2] = lab[2, 0]
    logits = (5.0 * torch.nn.functional.one_hot(pred, C).movedim(-1, 1).float()).to(DEV)
    for w_type in W_TYPES:
        got = generalized_dice_from_logits(logits, lab.to(DEV), C, False, w_type)
        assert got.tolist() == [1.0, 0.0, 1.0], (w_type, got)
        want = compute_generalized_dice(torch.nn.functional.one_hot(pred, C).movedim(-1, 1).float(),
                                        torch.nn.functional.one_hot(lab[:, 0], C).movedim(-1, 1).float(), include_background=False, weight_type=w_type)
        assert want.tolist() == [1.0, 0.0, 1.0]
    # the cumulative object on device tensors
    metric = GeneralizedDiceScore(include_background=False)
    ret = metric(y_pred=torch.nn.functional.one_hot(pred, C).movedim(-1, 1).float().to(DEV), y=torch.nn.functional.one_hot(lab[:, 0], C).movedim(-1, 1).float().to(DEV))
    assert ret.is_cuda and metric.aggregate().item() == pytest.approx(2.0 / 3.0, rel=1e-6)


def test_graphed_train_step_with_the_generalized_criterion():
    """test_graphed_train_step_matches_the_eager_loop with GeneralizedDiceFocalLoss: the loss rides in the captured step; same bars"""
    from mi_seg_amd.runtime.arena import ParamArena
    from mi_seg_amd.runtime.graph import GraphedTrainStep
    from mi_seg_amd.training.optim import ArenaOptimizer
    from mi_seg_amd.utils.detfill import det_input
    crit = GeneralizedDiceFocalLoss(include_background=False, to_onehot_y=True, softmax=True, smooth_nr=0.0, smooth_dr=1e-6)
    xs = [det_input(30 + i, (1, 1, 64, 64, 64)).to(DEV) for i in range(6)]
    ys = [(x.abs() * 3).floor().clamp(0, 5).to(torch.int32) for x in xs]
    mods = [0, 1, 1, 0, 0, 1]
    lrs = [2e-3, 2e-3, 2e-3, 5e-4, 5e-4, 5e-4]
    runs = {}
    for mode in ("eager", "graph"):
        m = _small_model(64, torch.bfloat16)
        params = [p for p in m.parameters() if p.requires_grad]
        arena = ParamArena(params, torch.bfloat16)
        try:
            opt = ArenaOptimizer(arena, "adamw", lr=lrs[0], weight_decay=1e-5)
            losses = []
            if mode == "graph":
                gts = GraphedTrainStep(m, crit, opt, xs[0].shape, ys[0].shape, arena)
            for x, y, md, lr in zip(xs, ys, mods, lrs):
                if mode == "graph":
                    gts.set_lr(lr)
                    losses.append(float(gts(x, y, [md])))
                else:
                    arena.begin_step()
                    loss = crit(m(x, [md]), y)
                    loss.backward()
                    arena.publish()
                    opt.step(lr=lr)
                    losses.append(float(loss))
            torch.cuda.synchronize()
            runs[mode] = (losses, {k: v.detach().clone() for k, v in m.state_dict().items()})
        finally:
            arena.detach()
    le, lg = runs["eager"][0], runs["graph"][0]
    print("generalized dice focal train step losses: eager", [round(v, 5) for v in le], "graph", [round(v, 5) for v in lg])
    assert all(v == v for v in lg) and lg[-1] < lg[0]
    for i, (a, b) in enumerate(zip(le, lg)):
        assert abs(a - b) < 2e-3 * (1 + i) * abs(a), (i, a, b)
    num = den = 0.0
    for k, v in runs["eager"][1].items():
        w = runs["graph"][1][k]
        if v.is_floating_point():
            num += float((v.double() - w.double()).pow(2).sum())
            den += float(v.double().pow(2).sum())
    print("generalized dice focal train step parameter distance", (num / den) ** 0.5)
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5


def test_litmonai_with_the_generalized_criterion_on_the_hip_path():
    """test_litmonai_training_and_validation_steps_on_the_hip_path with --criterion=generalized_dice_focal: training_step and the shared
    evaluation on the device, the loss against forward_torch on the oracle's float64 logits within 1e-4 relative"""
    from mi_seg_amd.data.synthetic import synthetic_volume
    from mi_seg_amd.networks.lightning_monai import LitMonai
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.training.metrics import dice_from_logits
    from mi_seg_amd.utils.detfill import fill_module_
    from mi_seg_amd.utils.parser import add_data_argparse_args, add_model_argparse_args, add_tune_argparse_args
    from oracle import nets as ON
    p = argparse.ArgumentParser()
    add_tune_argparse_args(add_data_argparse_args(add_model_argparse_args(p)))
    a = p.parse_args(["--model_name=swin_unetr", "--out_channels=6", "--feature_size=12", "--num_heads=3", "--roi_x=64", "--roi_y=64", "--roi_z=64",
                      "--encoder_norm_name=instance_cond", "--vit_norm_name=instance_cond", "--no_include_background", "--sw_batch_size=4",
                      "--criterion=generalized_dice_focal"])
    lit = LitMonai.from_argparse_args(a)
    assert type(lit.criterion) is GeneralizedDiceFocalLoss and not lit.criterion.cfg.include_background
    fill_module_(lit.model)
    lit = lit.to(DEV)
    sd = {k: v.detach().cpu().clone() for k, v in lit.model.state_dict().items()}
    cfg = ON.swin_unetr_cfg(feature_size=12)
    img, lab = synthetic_volume((96, 80, 64), 11, 1)
    crop = (slice(None), slice(None), slice(16, 80), slice(8, 72), slice(0, 64))
    batch = {"image": img[crop].to(DEV), "label": lab[crop].float().to(DEV), "modality": torch.tensor([1], device=DEV)}
    out = lit.training_step(batch, 0)
    assert set(out) == {"loss"} and out["loss"].is_cuda
    out["loss"].backward()
    assert all(bool(torch.isfinite(q.grad).all()) for q in lit.model.parameters() if q.grad is not None)
    with torch.no_grad():
        oracle_logits = ON.swin_unetr_forward(sd, img[crop], [1], cfg).double()
        want = lit.criterion.forward_torch(oracle_logits, lab[crop])
        moved = lit.criterion.forward_torch(oracle_logits.float().double(), lab[crop])
    print(f"litmonai generalized dice focal: train loss {float(out['loss']):.9g} oracle {float(want):.9g} rel {abs(float(out['loss']) - float(want)) / abs(float(want)):.3g}"
          f"; float64 loss moves by {abs(float(moved) - float(want)) / abs(float(want)):.3g} when the oracle logits are rounded to fp32")
    assert abs(float(out["loss"]) - float(want)) < 1e-4 * abs(float(want))
    assert abs(lit.logged["train/loss"] - float(want)) < 1e-4 * abs(float(want))
    val = lit.validation_step({"image": img.to(DEV), "label": lab.float().to(DEV), "modality": torch.tensor([1], device=DEV)}, 0)
    with torch.no_grad():
        logits = sliding_window_inference(img, 64, 1, lambda xx, mm: ON.swin_unetr_forward(sd, xx, mm, cfg), overlap=0.5, modalities=[1])
        want_dice = float(torch.nanmean(dice_from_logits(logits, lab, 6)))
        want_loss = float(lit.criterion.forward_torch(logits.double(), lab))
    print(f"litmonai generalized dice focal: val loss {float(val['loss']):.9g} oracle {want_loss:.9g} rel {abs(float(val['loss']) - want_loss) / abs(want_loss):.3g}")
    assert abs(float(val["accuracy"]) - want_dice) < 1e-4 and abs(float(val["loss"]) - want_loss) < 1e-4 * abs(want_loss)


def test_evaluate_with_a_generalized_dice_score_on_the_fused_branch():
    """evaluate.test with additional_metrics=[GeneralizedDiceScore]: the fused branch returns the same Dice and surface results as without it,
    and the score equals the one of the one-hot chain on the same logits within 1e-6"""
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    from surface_common import swin_evaluation
    C = 6
    m, loader, on_device, seen = swin_evaluation(C, volumes=3)

    def run(model_inferer, additional):
        res = {}
        ret = E.test(m, loader, DEV, M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True),
                     E.AsDiscrete(to_onehot=C), E.AsDiscrete(argmax=True, to_onehot=C), model_inferer=model_inferer, amp=False,
                     surface_distance=M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True),
                     results=res, additional_metrics=additional)
        return ret, res

    ret_plain, res_plain = run(on_device, None)
    logits = list(seen)
    ret_fused, res_fused = run(on_device, [GeneralizedDiceScore(include_background=False)])
    assert all(torch.equal(a, b) for a, b in zip(logits, seen[3:]))
    assert "additional_metrics" not in res_plain
    assert np.array_equal(np.array(ret_plain), np.array(ret_fused), equal_nan=True)
    for part in res_plain:
        assert np.array_equal(np.array(list(res_plain[part].values())), np.array(list(res_fused[part].values())), equal_nan=True), part
    replay = iter(logits)
    ret_cpu, res_cpu = run(lambda x, modalities=None: next(replay), [GeneralizedDiceScore(include_background=False)])       # CPU logits: the one-hot chain
    assert len(res_fused["additional_metrics"]) == 1
    assert res_fused["additional_metrics"][0] == pytest.approx(res_cpu["additional_metrics"][0], rel=1e-6, abs=1e-6)
    assert 0.0 <= res_fused["additional_metrics"][0] <= 1.0

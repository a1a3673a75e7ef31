"""What the GPU tests of the surface metrics and of the evaluation loop built on them share (test_hip_surface_distance.py, test_hip_hausdorff.py,
test_hip_surface_dice.py, test_hip_evaluate_paths.py): tied logits, bit equality, the SwinUNETR evaluation set-up with replayed CPU logits, and
the comparison of two `results` dicts of evaluate.test."""
from functools import partial

import pytest
import torch

from test_surface_distance_cpu import random_case, same

DEV = "cuda"
REL = 1e-9


def ops():
    from mi_seg_amd.hip import ops
    return ops


def tied_logits(pred, C, seed):
    """logits whose argmax is `pred` under torch's first-maximum rule, with exact ties: some channels after pred[v] equal the maximum, so the
    kernel must take the first maximum to find pred[v]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 3, (pred.shape[0], C) + pred.shape[1:], generator=g).float()
    p = torch.from_numpy(pred)[:, None]
    top = torch.full_like(x, 5.0)
    idx = torch.arange(C).view(1, C, 1, 1, 1)
    tie = torch.randint(0, 2, x.shape, generator=g).bool() & (idx > p)       # later channels equal to the max: the first one still wins
    x = torch.where(idx == p, top, torch.where(tie, top, x))
    assert torch.equal(x.argmax(dim=1), torch.from_numpy(pred))
    return x


def bits_equal(a, b):
    """torch.equal on the bit patterns: NaNs in the same places count as equal"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def swin_evaluation(C=6, volumes=4):
    """(model, loader, on_device, seen): a small SwinUNETR on the device, `volumes` volumes of 40 x 36 x 32 alternating between the two modalities,
    and the sliding-window inferer that appends every batch's logits, copied to the CPU, to the list `seen`"""
    from mi_seg_amd.networks.nets.swin_unetr import SwinUNETR
    from mi_seg_amd.networks.norms.utils import parse_normalization
    from mi_seg_amd.training.inferer import sliding_window_inference
    from mi_seg_amd.utils.detfill import det_input, fill_module_
    norm = partial(parse_normalization, affine=True, num_groups=4, num_styles=2)
    m = SwinUNETR((32,) * 3, 1, C, feature_size=12, num_heads=(3, 6, 12, 24), vit_norm_name=norm("instance_cond"),
                  encoder_norm_name=norm("instance_cond"), decoder_norm_name=norm("instance"))
    fill_module_(m)
    m = m.to(DEV)
    loader = []
    for i in range(volumes):
        _, lab = random_case(40 + i, (40, 36, 32), C, B=1)
        loader.append({"image": det_input(i, (1, 1, 40, 36, 32)), "label": torch.from_numpy(lab)[:, None].float(), "modality": torch.tensor([i % 2])})
    inferer = partial(sliding_window_inference, roi_size=(32, 32, 32), sw_batch_size=2, predictor=m, overlap=0.5)
    seen = []

    def on_device(x, modalities=None):
        out = inferer(x, modalities=modalities)
        seen.append(out.detach().cpu())
        return out

    return m, loader, on_device, seen


def swin_device_vs_replayed(C, metrics):
    """evaluate.test over swin_evaluation(C) with Dice and the metric objects `metrics()` returns as keywords, on the device's logits and then on
    their replayed CPU copies (the one-hot chain): ((return value, results) of the device run, the same of the replayed run)"""
    from mi_seg_amd.training import evaluate as E
    from mi_seg_amd.training import metrics as M
    m, loader, on_device, seen = swin_evaluation(C)

    def run(model_inferer):
        res = {}
        ret = E.test(m, loader, DEV, M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True),
                     E.AsDiscrete(to_onehot=C), E.AsDiscrete(argmax=True, to_onehot=C), model_inferer=model_inferer, amp=False, results=res, **metrics())
        return ret, res

    dev = run(on_device)
    assert len(seen) == len(loader) and seen[0].dtype == torch.float32
    replay = iter(seen)
    return dev, run(lambda x, modalities=None: next(replay))


def assert_results_match(res_dev, res_cpu):
    """two `results` dicts of evaluate.test, one from device logits and one from their CPU copies: the same keys in the same order; Dice (and
    the additional metrics' fp32 scores) at rel 1e-6, the surface-Dice parts exact, the other surface metrics at REL"""
    assert res_dev.keys() == res_cpu.keys()
    for part in res_dev:
        if part == "additional_metrics":
            assert res_dev[part] == pytest.approx(res_cpu[part], rel=1e-6), part
            continue
        assert list(res_dev[part]) == list(res_cpu[part]), part
        a, b = list(res_dev[part].values()), list(res_cpu[part].values())
        if part.startswith("dice"):
            assert a == pytest.approx(b, rel=1e-6, nan_ok=True), part
        elif part.startswith("surface_dice"):
            same(a, b, rel=0)
        else:
            same(a, b, rel=REL)


def assert_returns_match(ret_dev, ret_cpu):
    """the return values of evaluate.test: the mean Dice at rel 1e-6 and, with a surface-distance metric, the mean surface distance at REL"""
    if isinstance(ret_dev, tuple):
        assert isinstance(ret_cpu, tuple) and len(ret_dev) == len(ret_cpu) == 2
        assert ret_dev[0] == pytest.approx(ret_cpu[0], rel=1e-6)
        same([ret_dev[1]], [ret_cpu[1]], rel=REL)
    else:
        assert isinstance(ret_dev, float) and isinstance(ret_cpu, float) and ret_dev == pytest.approx(ret_cpu, rel=1e-6)

"""What evaluate.test() prints, stores and returns, on CPU tensors (the one-hot chain): for every subset of {surface distance, Hausdorff
distance, surface Dice}, with and without two generalized Dice scores, the exact printed text (titles, per-modality blocks, totals, additional
metrics, in that order), the keys of `results` and of each totals dict, the type of the return value, and that every metric object and every
per-modality buffer is reset on return."""
import contextlib
import io
import itertools

import numpy as np
import pytest
import torch

from mi_seg_amd.training import evaluate as E
from mi_seg_amd.training import metrics as M
from test_surface_distance_cpu import random_case

C = 4
SURFACE = ("surface_distance", "hausdorff_distance", "surface_dice")
TITLES = {"dice": "Dice per modality", "surface_distance": "Surface Distance per modality", "hausdorff_distance": "Hausdorff Distance per modality",
          "surface_dice": "Surface Dice per modality"}
FIRST_CLASS = {"dice": 0, "surface_distance": 0, "hausdorff_distance": 1, "surface_dice": 1}       # 1: the metric excludes the background
GRID = [(given, extra) for n in range(4) for given in itertools.combinations(SURFACE, n) for extra in (False, True)]


def _id(case):
    given, extra = case
    return ("+".join(given) or "dice_only") + ("+2gds" if extra else "")


_LOADER = []


def loader_and_logits():
    """three volumes of 7 x 8 x 9, modalities 0, 1, 0, and the logits a stub inferer replays for them"""
    if not _LOADER:
        loader, logits = [], []
        for i in range(3):
            pred, lab = random_case(50 + i, (7, 8, 9), C, B=1)
            x = torch.zeros(1, C, 7, 8, 9)
            x.scatter_(1, torch.from_numpy(pred)[:, None], 1.0)
            logits.append(x)
            loader.append({"image": torch.zeros(1, 1, 7, 8, 9), "label": torch.from_numpy(lab)[:, None].float(), "modality": torch.tensor([i % 2])})
        _LOADER.extend((loader, logits))
    return _LOADER


def make_metrics(given, extra):
    """the keyword arguments of evaluate.test for one case: Dice and surface distance with the background, the other two without"""
    kw = {"acc_func": M.DiceMetric(include_background=True, reduction="mean_batch", get_not_nans=True)}
    if "surface_distance" in given:
        kw["surface_distance"] = M.SurfaceDistanceMetric(include_background=True, symmetric=True, reduction="mean_batch", get_not_nans=True)
    if "hausdorff_distance" in given:
        kw["hausdorff_distance"] = M.HausdorffDistanceMetric(include_background=False, percentile=95, reduction="mean_batch", get_not_nans=True)
    if "surface_dice" in given:
        kw["surface_dice"] = M.SurfaceDiceMetric([1.0, 2.0 ** 0.5, 2.0], include_background=False, reduction="mean_batch", get_not_nans=True)
    if extra:
        kw["additional_metrics"] = [M.GeneralizedDiceScore(include_background=False, weight_type="square"),
                                    M.GeneralizedDiceScore(include_background=True, weight_type="simple")]
    return kw


def run_case(given, extra):
    """(printed text, results, return value, the metric objects) of evaluate.test on the replayed logits"""
    loader, logits = loader_and_logits()
    replay = iter(logits)
    kw = make_metrics(given, extra)
    res, text = {}, io.StringIO()
    with contextlib.redirect_stdout(text):
        ret = E.test(torch.nn.Identity(), loader, "cpu", post_label=E.AsDiscrete(to_onehot=C), post_pred=E.AsDiscrete(argmax=True, to_onehot=C),
                     model_inferer=lambda x, modalities=None: next(replay), amp=False, results=res, **kw)
    return text.getvalue(), res, ret, kw


def report_lines(res, given, extra):
    """the lines evaluate.test prints, restated from `results`: per tracked metric its title and, per modality, the classes' dict and the
    average's; then the totals in the same order; then the additional metrics.  The surface-distance title is printed with or without one."""
    tracked = ["dice"] + [k for k in SURFACE if k in given]
    lines = []
    for name in ["dice", "surface_distance"] + tracked[1 + ("surface_distance" in given):]:
        lines.append(TITLES[name])
        block = {}
        for k, v in (res[f"{name}_modality"] if name in tracked else {}).items():
            if k.endswith("/avg"):
                lines += [str(block), str({k: v})]
                block = {}
            else:
                block[k] = v
        assert not block
    lines += [str(res[f"{name}_total"]) for name in tracked]
    if extra:
        lines.append(str({"additional_metrics": res["additional_metrics"]}))
    return lines


@pytest.mark.parametrize("case", GRID, ids=_id)
def test_report(case, monkeypatch):
    given, extra = case
    made = []

    class Recorded(M.Cumulative):
        def __init__(self):
            super().__init__()
            made.append(self)

    monkeypatch.setattr(E, "Cumulative", Recorded)
    text, res, ret, kw = run_case(given, extra)
    tracked = ["dice"] + [k for k in SURFACE if k in given]
    lines = text.splitlines()
    titles = [ln for ln in lines if not ln.startswith("{")]
    assert titles == [TITLES["dice"], TITLES["surface_distance"]] + [TITLES[k] for k in given if k != "surface_distance"]
    assert lines == report_lines(res, given, extra) and text.endswith("\n")
    assert list(res) == ([f"{k}_modality" for k in tracked] + [f"{k}_total" for k in tracked] + (["additional_metrics"] if extra else []))
    for name in tracked:
        n = C - FIRST_CLASS[name]
        assert list(res[f"{name}_total"]) == [f"val_total_{name}/class{c}" for c in range(FIRST_CLASS[name], C)]
        per_mod = [f"val_modality{m}/{what}" for m in (0, 1) for what in [f"class{c}" for c in range(FIRST_CLASS[name], C)] + ["avg"]]
        assert list(res[f"{name}_modality"]) == per_mod and len(res[f"{name}_total"]) == n
        assert all(isinstance(v, float) for part in (f"{name}_modality", f"{name}_total") for v in res[part].values())
    if extra:
        assert len(res["additional_metrics"]) == 2 and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res["additional_metrics"])
        assert res["additional_metrics"][0] != res["additional_metrics"][1]
    if "surface_distance" in given:
        assert isinstance(ret, tuple) and len(ret) == 2 and all(isinstance(v, float) for v in ret)
        assert ret[1] == pytest.approx(np.nanmean(list(res["surface_distance_total"].values())), rel=1e-12)
    else:
        assert isinstance(ret, float)
    dice = ret[0] if isinstance(ret, tuple) else ret
    assert dice == pytest.approx(np.nanmean(np.float32(list(res["dice_total"].values()))), rel=1e-6)
    objects = [kw[k] for k in ("acc_func",) + SURFACE if k in kw] + list(kw.get("additional_metrics", ()))
    assert len(objects) == len(tracked) + 2 * extra and all(m.get_buffer() is None for m in objects)
    assert len(made) == len(tracked) and all(cum.get_buffer() is None for cum in made)


def test_the_dice_does_not_depend_on_the_other_metrics():
    """whatever else is tracked, the Dice parts of `results` and of the return value are the same numbers"""
    _, res0, ret0, _ = run_case((), False)
    for given, extra in GRID[1:]:
        _, res, ret, _ = run_case(given, extra)
        assert res["dice_modality"] == res0["dice_modality"] and res["dice_total"] == res0["dice_total"]
        assert (ret[0] if isinstance(ret, tuple) else ret) == ret0

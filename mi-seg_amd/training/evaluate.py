"""Test-set evaluation: Dice and, optionally, average surface distance, Hausdorff distance and normalized surface Dice per class, per modality
and over the whole set (reference test.py:17-123).

test() tracks its metrics through one table (_KINDS): per batch, _batch_values gives {name: [B, C'] values} and one loop appends them; at the
end one loop reports and resets.  With float32 logits on a HIP device and this module's AsDiscrete post-transforms and metric classes the batch
takes the fused path (no one-hot volume is built); anything else runs the reference's decollate / post-transform / metric
chain.  The checkpoint loading and MONAI's get_loaders of the reference's main() stay with the caller."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from .metrics import (Cumulative, DiceMetric, GeneralizedDiceScore, HausdorffDistanceMetric, SurfaceDiceMetric, SurfaceDistanceMetric,
                      dice_from_class_map, dice_from_logits, generalized_dice_from_class_map, generalized_dice_from_logits, surface_metrics_from_logits)

# the tracked metrics, in the order they are reported.  name: results[f"{name}_modality"], results[f"{name}_total"] and the keys
# val_total_{name}/class{c}; title: the printed one; cls: the class the fused path knows; want: its key in ops.surface_metrics(want=); ref: one of
# the reference's own two, whose title is printed with or without the metric and whose aggregate() is unpacked as (value, not_nans)
_Kind = namedtuple("_Kind", "name title cls want ref")
_KINDS = (_Kind("dice", "Dice per modality", DiceMetric, None, True),
          _Kind("surface_distance", "Surface Distance per modality", SurfaceDistanceMetric, "asd", True),
          _Kind("hausdorff_distance", "Hausdorff Distance per modality", HausdorffDistanceMetric, "hd", False),
          _Kind("surface_dice", "Surface Dice per modality", SurfaceDiceMetric, "nsd", False))


class AsDiscrete:
    """monai.transforms.AsDiscrete(argmax, to_onehot) on one channel-first sample [C, ...] (a label: [1, ...])"""

    def __init__(self, argmax=False, to_onehot=None):
        self.argmax, self.to_onehot = argmax, to_onehot

    def __call__(self, x):
        if self.argmax:
            x = x.argmax(dim=0, keepdim=True)
        if self.to_onehot is not None:
            x = F.one_hot(x[0].long(), self.to_onehot).movedim(-1, 0)
        return x.to(torch.float32)


def decollate_batch(t):
    return list(t.unbind(0))


def _fused(output, post_label, post_pred, given, additional_metrics):
    """the batch can skip the one-hot volumes: the post-transforms and metrics are the ones this module knows the semantics of"""
    C = output.shape[1]
    return (output.is_cuda and output.dtype == torch.float32 and output.dim() == 5 and C <= 64
            and isinstance(post_pred, AsDiscrete) and post_pred.argmax and post_pred.to_onehot == C
            and isinstance(post_label, AsDiscrete) and not post_label.argmax and post_label.to_onehot == C
            and all(type(m) is kind.cls for kind, m in given) and all(type(m) is GeneralizedDiceScore for m in additional_metrics or ()))


def _post_pred_filtered(post_pred, filters):
    """post_pred with the post-transforms `filters` (keep-largest, then fill-holes) between its argmax and its one-hot (after it, for a
    post-transform of the caller's own)"""
    def chain(t):
        for f in filters:
            t = f(t)
        return t
    if isinstance(post_pred, AsDiscrete) and post_pred.argmax:
        discrete, onehot = AsDiscrete(argmax=True), AsDiscrete(to_onehot=post_pred.to_onehot)
        return lambda t: onehot(chain(discrete(t)))
    return lambda t: chain(post_pred(t))


def _fused_surface_metrics(output, target, C, surface, pred=None):
    """{name: values} of the surface metric objects `surface` ([(kind, object)]) from ONE launch set over the logits `output` (or the int32
    class map `pred`): computed with the background if any of the objects wants it, and sliced for those that do not (the surface Dice then gets
    a tolerance for class 0 whose column is dropped)"""
    if not surface:
        return {}
    by_want = {kind.want: m for kind, m in surface}
    sd, hd, nsd = by_want.get("asd"), by_want.get("hd"), by_want.get("nsd")
    inc = any(m.include_background for m in by_want.values())
    kw = dict(include_background=inc, symmetric=sd.symmetric if sd is not None else True, percentile=hd.percentile if hd is not None else None,
              directed=hd.directed if hd is not None else False, want=tuple(by_want))
    if nsd is not None:
        kw["class_thresholds"] = ([0.0] if inc and not nsd.include_background else []) + list(nsd.class_thresholds)
    if pred is not None:
        from ..hip import ops
        got = ops.surface_metrics(target, pred=pred, num_classes=C, **kw)
    else:
        got = surface_metrics_from_logits(output, target, C, **kw)
    return {kind.name: v[:, int(inc and not m.include_background):] for (kind, m), v in zip(surface, got)}


def _batch_values(output, target, fused, filters, post_label, post_pred, given, additional_metrics):
    """{name: [B, C'] values} of one batch for the tracked metric objects `given` ([(kind, object)], the Dice first); the additional metrics
    are updated here.  Not fused: the one-hot chain, every object called as metric(y_pred=, y=), which appends to it (`post_pred` holds the
    filters).  Fused: the Dice from miseg_dice_metric with the first additional score riding on it, and every surface metric from one launch
    set; with `filters`, all of them from the filtered int32 class map instead, computed once on the device."""
    extra = list(additional_metrics or ())
    if not fused:
        y_pred = torch.stack([post_pred(t) for t in decollate_batch(output)])
        y = torch.stack([post_label(t) for t in decollate_batch(target)])
        for m in extra:
            m(y_pred=y_pred, y=y)
        return {kind.name: m(y_pred=y_pred, y=y) for kind, m in given}
    C, pred = output.shape[1], None
    if filters:
        pred = filters[0].class_map(logits=output.contiguous(), out_dtype=torch.int32)
        for f in filters[1:]:
            pred = f.class_map(pred=pred, num_classes=C, out_dtype=torch.int32)
        dice = dice_from_class_map(pred, target, C)
        scores = [generalized_dice_from_class_map(pred, target, C, m.include_background, m.weight_type) for m in extra]
    elif extra:         # the first score comes out of the Dice's own pass; a further one (other settings) re-reads the volume
        dice, score = generalized_dice_from_logits(output, target, C, extra[0].include_background, extra[0].weight_type, with_dice=True)
        scores = [score] + [generalized_dice_from_logits(output, target, C, m.include_background, m.weight_type) for m in extra[1:]]
    else:
        dice, scores = dice_from_logits(output, target, C), []
    for m, score in zip(extra, scores):
        m.extend(score)
    values = _fused_surface_metrics(output, target, C, given[1:], pred=pred)
    values["dice"] = dice if given[0][1].include_background else dice[:, 1:]
    return values


def compute_metric_modality(metric_func, include_background=0):
    """per-modality batch average of every class (NaNs left out, as do_metric_reduction's mean_batch) and their mean over the classes that
    have a value (reference test.py:17-43); prints and returns {key: value}"""
    metric, mod_metric = metric_func.get_buffer()
    metric = metric.cpu()
    mod_metric = mod_metric.cpu()
    out = {}
    for m in torch.unique(mod_metric):
        metric_m = metric[mod_metric == m]
        nans = torch.isnan(metric_m)
        not_nans = (~nans).float()
        t_zero = torch.zeros(1, device=metric_m.device, dtype=metric_m.dtype)
        not_nans = not_nans.sum(dim=0)
        metric_m[nans] = 0
        metric_m = torch.where(not_nans > 0, metric_m.sum(dim=0) / not_nans, t_zero)
        per_class = {f"val_modality{m}/class{c + include_background}": v for c, v in enumerate(metric_m.tolist())}
        print(per_class)
        avg = {f"val_modality{m}/avg": torch.nanmean(metric_m[not_nans > 0]).item()}
        print(avg)
        out.update(per_class)
        out.update(avg)
    return out


def test(model, loader, device, acc_func, post_label, post_pred, model_inferer=None, amp=True, surface_distance=None, results=None,
         additional_metrics=None, hausdorff_distance=None, keep_largest=None, fill_holes=None, surface_dice=None):
    """the reference's evaluation loop (test.py:46-123): returns the mean total Dice over the classes with a value (and the mean total surface
    distance when `surface_distance` is given).  `results`, a dict, receives the printed values: per tracked metric (_KINDS: the Dice and each
    of `surface_distance`, `hausdorff_distance`, `surface_dice` that is given) "{name}_modality" and "{name}_total", each {printed key: value}.
    `additional_metrics`: a list of cumulative metric objects updated with every batch and aggregated (`metric.aggregate().item()`) and reset
    at the end, as the reference's validation loop does (utils/trainer.py:145-149,246-250); their values are printed and stored in
    results["additional_metrics"].  Every metric object is reset on return.
    `model_inferer` is the caller's, e.g. the reference's partial(sliding_window_inference, predictor=model, roi_size=..., sw_batch_size=...,
    overlap=...); MONAI's Gaussian window blend is the same partial with mode="gaussian" (and sigma_scale= / padding_mode= as wanted).
    `keep_largest` (a postprocess.KeepLargestConnectedComponent) and then `fill_holes` (a postprocess.FillHoles) are applied to the argmax
    before every metric (MONAI places them between AsDiscrete(argmax=True) and the metrics)."""
    model.eval()
    filters = [f for f in (keep_largest, fill_holes) if f is not None]
    chain_pred = _post_pred_filtered(post_pred, filters) if filters else post_pred
    metrics = (acc_func, surface_distance, hausdorff_distance, surface_dice)
    tracked = {kind: (m, Cumulative()) for kind, m in zip(_KINDS, metrics) if m is not None}
    given = [(kind, m) for kind, (m, _) in tracked.items()]
    dev_type = torch.device(device).type
    with torch.no_grad():
        for batch in loader:
            data, target = batch["image"].to(device), batch["label"].to(device)
            modality = batch["modality"].to(device) if "modality" in batch.keys() else None
            with torch.autocast(device_type=dev_type, enabled=amp and dev_type == "cuda"):
                output = model_inferer(data, modalities=modality) if model_inferer is not None else model(data, modality)
            fused = _fused(output, post_label, post_pred, given, additional_metrics)
            values = _batch_values(output, target, fused, filters, post_label, chain_pred, given, additional_metrics)
            for kind, (m, cumulative) in tracked.items():
                if fused:       # in the one-hot chain the object's own call has appended them
                    m.extend(values[kind.name])
                cumulative.extend(values[kind.name], modality)
    results = {} if results is None else results
    totals, means = {}, []
    for kind in _KINDS:
        if kind in tracked or kind.ref:
            print(kind.title)
        if kind not in tracked:
            continue
        m, cumulative = tracked[kind]
        first = int(not m.include_background)
        results[f"{kind.name}_modality"] = compute_metric_modality(cumulative, first)
        value = m.aggregate()
        if kind.ref:
            value, not_nans = value
            means.append(torch.nanmean(value[not_nans > 0]).item())
        else:
            value = (value[0] if isinstance(value, tuple) else value).reshape(-1)          # get_not_nans or not
        totals[f"{kind.name}_total"] = {f"val_total_{kind.name}/class{c + first}": v for c, v in enumerate(value.tolist())}
        m.reset()
        cumulative.reset()
    for total in totals.values():
        print(total)
    results.update(totals)
    if additional_metrics:
        scores = []
        for m in additional_metrics:
            scores.append(m.aggregate().item())
            m.reset()
        print({"additional_metrics": scores})
        results["additional_metrics"] = scores
    return tuple(means) if len(means) == 2 else means[0]

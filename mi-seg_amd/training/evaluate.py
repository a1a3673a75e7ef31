"""Test-set evaluation: Dice, average surface distance and (optionally) Hausdorff distance per class, per modality and over the whole set
(reference test.py:17-123).

With float32 logits on a HIP device, this module's AsDiscrete post-transforms, DiceMetric and SurfaceDistanceMetric, the batch takes the fused
path (dice_from_logits + surface_distance_from_logits: no one-hot volume is built); anything else runs the reference's decollate / post-transform
/ metric chain.  `additional_metrics` (reference utils/trainer.py:145-149,246-250): a GeneralizedDiceScore rides on the fused path, fed from the
same miseg_dice_metric call as the Dice; any other metric object sends the batch down the unfused chain.  The checkpoint loading and MONAI's
get_loaders of the reference's main() stay with the caller.  A HausdorffDistanceMetric (`hausdorff_distance`, DESIGN.md
section 7.5) rides on the fused path too: its values and the surface distance's come out of ONE surface_metrics_from_logits call per batch.
`keep_largest` (a postprocess.KeepLargestConnectedComponent) filters the argmax before every metric: on the fused path the
filtered int32 class map is computed once on the device and feeds the Dice counts and ops.surface_metrics(pred=).  `fill_holes` (a
postprocess.FillHoles) follows it, or stands alone, in the same two places.  A SurfaceDiceMetric (`surface_dice`, DESIGN.md
section 7.9) rides on the fused path as well: the surface distance, the Hausdorff distance and the surface Dice of a batch come out of ONE call."""
import torch
import torch.nn.functional as F

from .metrics import (Cumulative, DiceMetric, GeneralizedDiceScore, HausdorffDistanceMetric, SurfaceDiceMetric, SurfaceDistanceMetric,
                      dice_from_class_map, dice_from_logits, generalized_dice_from_class_map, generalized_dice_from_logits, surface_distance_from_logits,
                      surface_metrics_from_logits)


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


def _fused(output, post_label, post_pred, acc_func, surface_distance, additional_metrics=None, hausdorff_distance=None, surface_dice=None):
    """the batch can skip the one-hot volumes: the post-transforms and metrics are the ones this module knows the semantics of"""
    C = output.shape[1]
    return (output.is_cuda and output.dtype == torch.float32 and output.dim() == 5 and C <= 64
            and isinstance(post_pred, AsDiscrete) and post_pred.argmax and post_pred.to_onehot == C
            and isinstance(post_label, AsDiscrete) and not post_label.argmax and post_label.to_onehot == C
            and type(acc_func) is DiceMetric and (surface_distance is None or type(surface_distance) is SurfaceDistanceMetric)
            and all(type(m) is GeneralizedDiceScore for m in additional_metrics or ())
            and (hausdorff_distance is None or type(hausdorff_distance) is HausdorffDistanceMetric)
            and (surface_dice is None or type(surface_dice) is SurfaceDiceMetric))


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


def _fused_surface_metrics(output, target, C, sd, hd, nsd, pred=None):
    """(surface distance, Hausdorff distance, surface Dice) of a batch, None for a metric object that is None, from ONE launch set over the logits
    `output` (or the int32 class map `pred`): computed with the background if any of the objects wants it, and sliced for those that do not
    (the surface Dice then gets a tolerance for class 0 whose column is dropped)"""
    inc = any(m.include_background for m in (sd, hd, nsd) if m is not None)
    want = tuple(k for k, m in (("asd", sd), ("hd", hd), ("nsd", nsd)) if m is not None)
    kw = dict(include_background=inc, symmetric=sd.symmetric if sd is not None else True, percentile=hd.percentile if hd is not None else None,
              directed=hd.directed if hd is not None else False, want=want)
    if nsd is not None:
        kw["class_thresholds"] = ([0.0] if inc and not nsd.include_background else []) + list(nsd.class_thresholds)
    if pred is not None:
        from ..hip import ops
        got = ops.surface_metrics(target, pred=pred, num_classes=C, **kw)
    else:
        got = surface_metrics_from_logits(output, target, C, **kw)
    got = dict(zip(want, got))
    return tuple(None if m is None else got[k][:, int(inc and not m.include_background):] for k, m in (("asd", sd), ("hd", hd), ("nsd", nsd)))


def _filtered_batch(output, target, filters, acc_func, surface_distance, additional_metrics, hausdorff_distance, surface_dice=None):
    """the fused path with post-transforms: (dice [B, C], surface distance or None, Hausdorff distance or None, surface Dice or None) from the
    filtered int32 class map, computed once on the device; the generalized Dice scores are extended here"""
    C = output.shape[1]
    pred = filters[0].class_map(logits=output.contiguous(), out_dtype=torch.int32)
    for f in filters[1:]:
        pred = f.class_map(pred=pred, num_classes=C, out_dtype=torch.int32)
    dice = dice_from_class_map(pred, target, C)
    for m in additional_metrics or ():
        m.extend(generalized_dice_from_class_map(pred, target, C, m.include_background, m.weight_type))
    batch_surface = batch_hd = batch_nsd = None
    if surface_distance is not None or hausdorff_distance is not None or surface_dice is not None:
        batch_surface, batch_hd, batch_nsd = _fused_surface_metrics(None, target, C, surface_distance, hausdorff_distance, surface_dice, pred=pred)
    return dice, batch_surface, batch_hd, batch_nsd


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
    distance when `surface_distance` is given).  `results`, a dict, receives the printed values: "dice_modality", "dice_total" and, with
    `surface_distance`, "surface_distance_modality", "surface_distance_total", each {printed key: value}.  `additional_metrics`: a list of
    cumulative metric objects updated with every batch and aggregated (`metric.aggregate().item()`) and reset at the end, as the reference's
    validation loop does (utils/trainer.py:145-149,246-250); their values are printed and stored in results["additional_metrics"].
    `hausdorff_distance`: a HausdorffDistanceMetric accumulated, printed and reset like the surface distance; `results` then also holds
    "hausdorff_distance_modality" and "hausdorff_distance_total".  The return value does not change.
    `model_inferer` is the caller's, e.g. the reference's partial(sliding_window_inference, predictor=model, roi_size=..., sw_batch_size=...,
    overlap=...); MONAI's Gaussian window blend is the same partial with mode="gaussian" (and sigma_scale= / padding_mode= as wanted).
    `keep_largest`: a postprocess.KeepLargestConnectedComponent applied to the argmax before every metric (MONAI places it between
    AsDiscrete(argmax=True) and the metrics); None leaves the loop exactly as it is without one.
    `fill_holes`: a postprocess.FillHoles applied in the same place, after `keep_largest` when both are given; None changes nothing.
    `surface_dice`: a SurfaceDiceMetric accumulated, printed and reset like the Hausdorff metric; `results` then also holds
    "surface_dice_modality" and "surface_dice_total" (keys val_total_surface_dice/class{c}).  None changes nothing."""
    model.eval()
    filters = [f for f in (keep_largest, fill_holes) if f is not None]
    if filters:
        post_pred_kl = _post_pred_filtered(post_pred, filters)
    acc_mod_cumulative = Cumulative()
    surface_mod_cumulative = Cumulative() if surface_distance is not None else None
    hausdorff_mod_cumulative = Cumulative() if hausdorff_distance is not None else None
    nsd_mod_cumulative = Cumulative() if surface_dice is not None else None
    dev_type = torch.device(device).type
    with torch.no_grad():
        for batch in loader:
            data, target = batch["image"].to(device), batch["label"].to(device)
            modality = batch["modality"].to(device) if "modality" in batch.keys() else None
            with torch.autocast(device_type=dev_type, enabled=amp and dev_type == "cuda"):
                output = model_inferer(data, modalities=modality) if model_inferer is not None else model(data, modality)
            fused = _fused(output, post_label, post_pred, acc_func, surface_distance, additional_metrics, hausdorff_distance, surface_dice)
            if fused and filters:
                dice, batch_surface, batch_hd, batch_nsd = _filtered_batch(output, target, filters, acc_func, surface_distance, additional_metrics,
                                                                           hausdorff_distance, surface_dice)
                batch_acc = dice if acc_func.include_background else dice[:, 1:]
                acc_func.extend(batch_acc)
                acc_mod_cumulative.extend(batch_acc, modality)
                if surface_distance is not None:
                    surface_distance.extend(batch_surface)
                    surface_mod_cumulative.extend(batch_surface, modality)
                if hausdorff_distance is not None:
                    hausdorff_distance.extend(batch_hd)
                    hausdorff_mod_cumulative.extend(batch_hd, modality)
                if surface_dice is not None:
                    surface_dice.extend(batch_nsd)
                    nsd_mod_cumulative.extend(batch_nsd, modality)
                continue
            if fused:
                C = output.shape[1]
                if additional_metrics:      # the first score comes out of the Dice's own pass; a further one (other settings) re-reads the volume
                    m0 = additional_metrics[0]
                    dice, score = generalized_dice_from_logits(output, target, C, m0.include_background, m0.weight_type, with_dice=True)
                    m0.extend(score)
                    for m in additional_metrics[1:]:
                        m.extend(generalized_dice_from_logits(output, target, C, m.include_background, m.weight_type))
                else:
                    dice = dice_from_logits(output, target, C)
                batch_acc = dice if acc_func.include_background else dice[:, 1:]
                acc_func.extend(batch_acc)
            else:
                val_output_convert = torch.stack([(post_pred_kl if filters else post_pred)(t) for t in decollate_batch(output)])
                val_labels_convert = torch.stack([post_label(t) for t in decollate_batch(target)])
                batch_acc = acc_func(y_pred=val_output_convert, y=val_labels_convert)
                for m in additional_metrics or ():
                    m(y_pred=val_output_convert, y=val_labels_convert)
            acc_mod_cumulative.extend(batch_acc, modality)
            if surface_dice is not None and fused:      # every surface metric of the batch from one launch set
                batch_surface, batch_hd, batch_nsd = _fused_surface_metrics(output, target, output.shape[1], surface_distance, hausdorff_distance,
                                                                            surface_dice)
                for m, cum, val in ((surface_distance, surface_mod_cumulative, batch_surface), (hausdorff_distance, hausdorff_mod_cumulative, batch_hd),
                                    (surface_dice, nsd_mod_cumulative, batch_nsd)):
                    if m is not None:
                        m.extend(val)
                        cum.extend(val, modality)
                continue
            if surface_dice is not None:
                nsd_mod_cumulative.extend(surface_dice(y_pred=val_output_convert, y=val_labels_convert), modality)
            if hausdorff_distance is not None:
                hd = hausdorff_distance
                if fused and surface_distance is not None:      # both from one launch set; with the background and sliced if the two disagree
                    inc = bool(surface_distance.include_background or hd.include_background)
                    batch_surface, batch_hd = surface_metrics_from_logits(output, target, output.shape[1], include_background=inc,
                                                                          symmetric=surface_distance.symmetric, percentile=hd.percentile, directed=hd.directed)
                    batch_surface = batch_surface[:, int(inc and not surface_distance.include_background):]
                    batch_hd = batch_hd[:, int(inc and not hd.include_background):]
                    surface_distance.extend(batch_surface)
                    hd.extend(batch_hd)
                    surface_mod_cumulative.extend(batch_surface, modality)
                elif fused:
                    batch_hd = surface_metrics_from_logits(output, target, output.shape[1], include_background=hd.include_background, percentile=hd.percentile,
                                                           directed=hd.directed, want=("hd",))[0]
                    hd.extend(batch_hd)
                else:
                    batch_hd = hd(y_pred=val_output_convert, y=val_labels_convert)
                hausdorff_mod_cumulative.extend(batch_hd, modality)
            if surface_distance is not None and not (fused and hausdorff_distance is not None):
                if fused:
                    batch_surface = surface_distance_from_logits(output, target, output.shape[1], include_background=surface_distance.include_background,
                                                                 symmetric=surface_distance.symmetric)
                    surface_distance.extend(batch_surface)
                else:
                    batch_surface = surface_distance(y_pred=val_output_convert, y=val_labels_convert)
                surface_mod_cumulative.extend(batch_surface, modality)
    results = {} if results is None else results
    print("Dice per modality")
    include_background_acc = int(not acc_func.include_background)
    results["dice_modality"] = compute_metric_modality(acc_mod_cumulative, include_background_acc)
    print("Surface Distance per modality")
    if surface_distance is not None:
        include_background_surf = int(not surface_distance.include_background)
        results["surface_distance_modality"] = compute_metric_modality(surface_mod_cumulative, include_background_surf)
    if hausdorff_distance is not None:
        print("Hausdorff Distance per modality")
        include_background_hd = int(not hausdorff_distance.include_background)
        results["hausdorff_distance_modality"] = compute_metric_modality(hausdorff_mod_cumulative, include_background_hd)
    if surface_dice is not None:
        print("Surface Dice per modality")
        include_background_nsd = int(not surface_dice.include_background)
        results["surface_dice_modality"] = compute_metric_modality(nsd_mod_cumulative, include_background_nsd)
    accuracy, not_nans = acc_func.aggregate()
    dict_acc_class = {f"val_total_dice/class{c + include_background_acc}": v for c, v in enumerate(accuracy.tolist())}
    print(dict_acc_class)
    results["dice_total"] = dict_acc_class
    if surface_distance is not None:
        surface, not_nans_surface = surface_distance.aggregate()
        dict_surf_class = {f"val_total_surface_distance/class{c + include_background_surf}": v for c, v in enumerate(surface.tolist())}
        print(dict_surf_class)
        results["surface_distance_total"] = dict_surf_class
        surface_distance.reset()
        surface_mod_cumulative.reset()
    if hausdorff_distance is not None:
        hausdorff = hausdorff_distance.aggregate()
        hausdorff = hausdorff[0] if isinstance(hausdorff, tuple) else hausdorff          # get_not_nans or not
        dict_hd_class = {f"val_total_hausdorff_distance/class{c + include_background_hd}": v for c, v in enumerate(hausdorff.reshape(-1).tolist())}
        print(dict_hd_class)
        results["hausdorff_distance_total"] = dict_hd_class
        hausdorff_distance.reset()
        hausdorff_mod_cumulative.reset()
    if surface_dice is not None:
        nsd = surface_dice.aggregate()
        nsd = nsd[0] if isinstance(nsd, tuple) else nsd          # get_not_nans or not
        dict_nsd_class = {f"val_total_surface_dice/class{c + include_background_nsd}": v for c, v in enumerate(nsd.reshape(-1).tolist())}
        print(dict_nsd_class)
        results["surface_dice_total"] = dict_nsd_class
        surface_dice.reset()
        nsd_mod_cumulative.reset()
    acc_func.reset()
    acc_mod_cumulative.reset()
    if additional_metrics:
        metrics = []
        for m in additional_metrics:
            metrics.append(m.aggregate().item())
            m.reset()
        print({"additional_metrics": metrics})
        results["additional_metrics"] = metrics
    if surface_distance is not None:
        return torch.nanmean(accuracy[not_nans > 0]).item(), torch.nanmean(surface[not_nans_surface > 0]).item()
    return torch.nanmean(accuracy[not_nans > 0]).item()

"""Dice metric / AsDiscrete with MONAI 1.1.0 semantics (reference lightning_monai.py:68-79,190-195).  Parity unpinned (Appendix B).
Average surface distance and the cumulative metric objects of the reference's evaluation script (test.py:17-171).
Generalized Dice score of the reference's validation (tune.py:124-129,208-213).
Hausdorff distance (MONAI 1.1.0 metrics/hausdorff_distance.py) on the surface-distance machinery.
Normalized surface Dice at per-class tolerances (MONAI's SurfaceDiceMetric / compute_surface_dice) on the same machinery."""
import math
import numpy as np
import torch
import torch.nn.functional as F


def as_discrete_argmax_onehot(logits, num_classes):
    """AsDiscrete(argmax=True, to_onehot=C) on a batched [B,C,...] tensor."""
    idx = logits.argmax(dim=1)
    return F.one_hot(idx, num_classes).movedim(-1, 1).to(torch.float32)


def as_discrete_onehot(label, num_classes):
    return F.one_hot(label[:, 0].long(), num_classes).movedim(-1, 1).to(torch.float32)


def dice_metric(y_pred_onehot, y_onehot):
    """per (b, c): 2|y & yhat| / (|y| + |yhat|), NaN where |y| == 0  (DiceMetric(include_background=True, get_not_nans=True))."""
    dims = tuple(range(2, y_pred_onehot.dim()))
    inter = (y_pred_onehot * y_onehot).sum(dims)
    y_o = y_onehot.sum(dims)
    den = y_o + y_pred_onehot.sum(dims)
    out = 2.0 * inter / den.clamp(min=1e-30)
    out = torch.where(den > 0, out, torch.ones_like(out))
    return torch.where(y_o > 0, out, torch.full_like(out, float("nan")))


def dice_from_logits(logits, label, num_classes):
    """AsDiscrete(argmax, to_onehot) on the logits + AsDiscrete(to_onehot) on the label + DiceMetric, as LitMonai._shared_eval chains them
    (reference lightning_monai.py:190-195).  On a HIP device: one pass over logits + labels with integer counters (csrc/training.hip,
    bit-reproducible); on CPU tensors (--infer_cpu) the torch arithmetic above."""
    if logits.is_cuda and logits.dtype == torch.float32 and logits.shape[1] == num_classes and num_classes <= 64:
        from ..hip import ops
        return ops.dice_metric(logits.contiguous(), label.to(logits.device))
    return dice_metric(as_discrete_argmax_onehot(logits, num_classes), as_discrete_onehot(label, num_classes))


# ------------------------------------------------------------------------------------------ generalized Dice score (reference tune.py:124-129)
_WEIGHT_TYPES = ("square", "simple", "uniform")


def _check_weight_type(weight_type):
    if weight_type not in _WEIGHT_TYPES:
        raise ValueError(f"Unsupported weight type: {weight_type}, available options are {list(_WEIGHT_TYPES)}.")


def compute_generalized_dice(y_pred, y, include_background=True, weight_type="square"):
    """MONAI 1.1.0 compute_generalized_dice on one-hot [B, C, ...] inputs -> fp32 [B] (DESIGN.md section 7.4 rules 6-7, parity unpinned):
    2 sum_c w I / sum_c w (G + P) over the kept classes with w = 1/G^2 | 1/G | 1 of the label count, an infinite w replaced by the sample's
    largest finite one; where the denominator is 0 the score is 1 if the prediction has no kept-class voxel and 0 otherwise.  The sums are
    voxel counts, formed in float64 (MONAI forms the weights in float32: the same numbers to fp32 rounding)."""
    _check_weight_type(weight_type)
    if y_pred.shape != y.shape:
        raise ValueError(f"y_pred - {tuple(y_pred.shape)} - and y - {tuple(y.shape)} - should have the same shapes.")
    if y_pred.dim() < 3:
        raise ValueError(f"y_pred should have at least 3 dimensions (batch, channel, spatial), got {y_pred.dim()}.")
    y = y.to(y_pred.device)
    if not include_background and y_pred.shape[1] > 1:
        y_pred, y = y_pred[:, 1:], y[:, 1:]
    dims = tuple(range(2, y_pred.dim()))
    yp, yt = y_pred.double(), y.double()
    return _generalized_dice_of_sums((yp * yt).sum(dims), yt.sum(dims), yp.sum(dims), weight_type)


def _generalized_dice_of_sums(inter, y_o, y_pred_o, weight_type):
    """compute_generalized_dice from the float64 [B, C'] sums of the kept classes: intersection, label, prediction"""
    from .losses import generalized_dice_weights
    w = generalized_dice_weights(y_o, weight_type)
    numer = 2.0 * (inter * w).sum(1)
    denom = ((y_o + y_pred_o) * w).sum(1)
    score = numer / denom.clamp(min=1e-300)
    empty = torch.where(y_pred_o.sum(1) == 0, torch.ones_like(score), torch.zeros_like(score))
    return torch.where(denom == 0, empty, score).float()


def class_map_counts(pred, label, num_classes):
    """int64 [B, C] voxel counts (intersection, label, prediction) per class of two integer class maps [B, ...] (label: [B, (1,) ...]) from one
    torch.bincount of the per-sample confusion matrix; values outside [0, C) belong to no class on either side"""
    B, Cc = pred.shape[0], int(num_classes)
    p, g = pred.reshape(B, -1).long(), label.to(pred.device).reshape(B, -1).long()
    p = torch.where((p >= 0) & (p < Cc), p, torch.full_like(p, Cc))
    g = torch.where((g >= 0) & (g < Cc), g, torch.full_like(g, Cc))
    n = (Cc + 1) * (Cc + 1)
    key = p * (Cc + 1) + g + n * torch.arange(B, device=pred.device).view(B, 1)
    conf = torch.bincount(key.reshape(-1), minlength=B * n).view(B, Cc + 1, Cc + 1)
    return conf.diagonal(dim1=1, dim2=2)[:, :Cc], conf.sum(1)[:, :Cc], conf.sum(2)[:, :Cc]


def dice_from_class_map(pred, label, num_classes):
    """dice_metric (fp32 [B, C], NaN where the label has no voxel of the class) of an already discrete prediction, from class_map_counts: the
    one-hot volumes' float sums are these counts"""
    inter, y_o, p_o = (t.float() for t in class_map_counts(pred, label, num_classes))
    den = y_o + p_o
    out = 2.0 * inter / den.clamp(min=1e-30)
    out = torch.where(den > 0, out, torch.ones_like(out))
    return torch.where(y_o > 0, out, torch.full_like(out, float("nan")))


def generalized_dice_from_class_map(pred, label, num_classes, include_background=True, weight_type="square"):
    """compute_generalized_dice (fp32 [B]) of an already discrete prediction, from class_map_counts"""
    _check_weight_type(weight_type)
    c0 = 0 if include_background or num_classes == 1 else 1
    inter, y_o, p_o = (t[:, c0:].double() for t in class_map_counts(pred, label, num_classes))
    return _generalized_dice_of_sums(inter, y_o, p_o, weight_type)


def generalized_dice_from_logits(logits, label, num_classes, include_background=True, weight_type="square", with_dice=False):
    """AsDiscrete(argmax, to_onehot) on the logits + AsDiscrete(to_onehot) on the label + compute_generalized_dice: fp32 [B].  On a HIP device:
    the one pass of dice_from_logits, the score taken from the same integer counts (miseg_dice_metric with its `gdice` output,
    bit-reproducible); on CPU tensors the torch arithmetic above.  with_dice=True returns (dice [B, C], score [B]) from that one pass."""
    _check_weight_type(weight_type)
    if logits.is_cuda and logits.dtype == torch.float32 and logits.shape[1] == num_classes and num_classes <= 64:
        from ..hip import ops
        dice, score = ops.dice_metric(logits.contiguous(), label.to(logits.device), gdice=(include_background, weight_type))
    else:
        pred, lab = as_discrete_argmax_onehot(logits, num_classes), as_discrete_onehot(label, num_classes)
        score = compute_generalized_dice(pred, lab, include_background, weight_type)
        dice = dice_metric(pred, lab) if with_dice else None
    return (dice, score) if with_dice else score


# ------------------------------------------------------------------------------------------ surface distance (reference test.py:145-151)
# MONAI 1.1.0 metrics/surface_distance.py + metrics/utils.py restated (parity unpinned).  The CPU restatement below is
# MONAI's own recipe (scipy.ndimage when it imports, an exact numpy EDT otherwise); on a HIP device csrc/surface.hip computes the same numbers.

def _erode(m):
    """scipy.ndimage.binary_erosion(m) with its defaults: cross structure, border_value 0 (a 0-d array erodes to itself)"""
    if m.ndim == 0:
        return m.copy()
    p = np.pad(m, 1, constant_values=False)
    out = m.copy()
    for ax in range(m.ndim):
        for lo in (0, 2):
            out &= p[tuple(slice(lo, lo + n) if a == ax else slice(1, 1 + n) for a, n in enumerate(m.shape))]
    return out


def _edt(nonseed):
    """distance_transform_edt(nonseed): exact Euclidean distance of every voxel to the nearest False voxel (at least one exists), float64.
    Separable: the squared distance along axis 0 first, then min_k f(x + k) + k^2 along every further axis."""
    inf = np.int64(1) << 40
    f = np.where(nonseed, inf, 0).astype(np.int64)
    for ax in range(f.ndim):
        f = np.moveaxis(f, ax, 0)
        g = f.copy()
        for k in range(1, f.shape[0]):
            np.minimum(g[k:], f[:-k] + k * k, out=g[k:])
            np.minimum(g[:-k], f[k:] + k * k, out=g[:-k])
        f = np.moveaxis(g, 0, ax)
    return np.sqrt(f.astype(np.float64))


def _ndimage():
    try:
        from scipy import ndimage
        return ndimage
    except ImportError:
        return None


def _mask_edges(p, g, nd):
    """get_mask_edges: crop to the box of p | g, squeeze, edges = erode(m) ^ m"""
    u = p | g
    if not u.any():
        return np.zeros_like(p), np.zeros_like(g)
    box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in np.nonzero(u))
    p, g = np.squeeze(p[box]), np.squeeze(g[box])
    erode = nd.binary_erosion if nd is not None else _erode
    return erode(p) ^ p, erode(g) ^ g


def _surface_distance(ea, eb, nd):
    """get_surface_distance(ea, eb, 'euclidean'): distance of every voxel of ea to the nearest voxel of eb"""
    if not eb.any():
        dis = np.full(eb.shape, np.inf)
    else:
        if not ea.any():
            return np.full(eb.shape, np.inf)[eb]
        dis = nd.distance_transform_edt(~eb) if nd is not None else _edt(~eb)
    return np.asarray(dis[ea])


def average_surface_distance_numpy(pred, gt, symmetric, use_scipy=True):
    """pred, gt: bool [B, C, *spatial] -> float64 [B, C] (compute_average_surface_distance after ignore_background).  use_scipy=False takes
    the numpy erosion / EDT even where scipy imports."""
    nd = _ndimage() if use_scipy else None
    B, Cc = pred.shape[:2]
    asd = np.empty((B, Cc))
    for b, c in np.ndindex(B, Cc):
        ep, eg = _mask_edges(pred[b, c], gt[b, c], nd)
        sd = _surface_distance(ep, eg, nd)
        if symmetric:
            sd = np.concatenate([sd, _surface_distance(eg, ep, nd)])
        asd[b, c] = np.nan if sd.shape == (0,) else sd.mean()
    return asd


def _check_metric(distance_metric):
    if distance_metric != "euclidean":
        raise NotImplementedError(f"distance_metric '{distance_metric}' is not implemented (supported: 'euclidean')")


def _exclusive_onehot(t):
    """every voxel has exactly one channel at 1 and the others at 0"""
    return bool((((t == 0) | (t == 1)).all() & (t.sum(dim=1) == 1).all()).item())


def _kernels_take(t):
    """a tensor [B, C, D, H, W] that csrc/surface.hip takes: on the device, C <= 64, sides <= 4096"""
    return t.is_cuda and t.dim() == 5 and t.shape[1] <= 64 and max(t.shape[2:]) <= 4096


def _surface_numpy(want, p, g, symmetric, percentile, directed, class_thresholds):
    """the CPU restatements named in `want` of bool [B, C', *spatial] arrays, as float64 [B, C'] tensors"""
    out = {"asd": lambda: average_surface_distance_numpy(p, g, symmetric), "hd": lambda: hausdorff_distance_numpy(p, g, percentile, directed),
           "nsd": lambda: surface_dice_numpy(p, g, class_thresholds)}
    return tuple(torch.from_numpy(out[w]()) for w in want)


def _onehot_surface_metric(want, y_pred, y, include_background, symmetric=True, percentile=None, directed=False, class_thresholds=None):
    """one surface metric ("asd", "hd" or "nsd") of one-hot [B, C, *spatial] inputs -> float64 [B, C'] on the device of y_pred.  On a HIP
    device with exclusive one-hot 3-D inputs: class maps into csrc/surface.hip; otherwise the CPU restatement."""
    if y_pred.shape != y.shape:
        raise ValueError(f"y_pred and y should have same shapes, got {tuple(y_pred.shape)} and {tuple(y.shape)}.")
    if want == "nsd":
        class_thresholds = _check_thresholds(class_thresholds, y_pred.shape[1] - (0 if include_background else 1))
    if _kernels_take(y_pred) and _exclusive_onehot(y_pred) and _exclusive_onehot(y.to(y_pred.device)):
        from ..hip import ops
        return ops.surface_metrics(y.to(y_pred.device).argmax(dim=1).to(torch.uint8), pred=y_pred.argmax(dim=1), num_classes=y_pred.shape[1],
                                   include_background=include_background, symmetric=symmetric, percentile=percentile, directed=directed,
                                   want=(want,), class_thresholds=class_thresholds)[0]
    if not include_background:
        y_pred, y = y_pred[:, 1:], y[:, 1:]
    p, g = y_pred.detach().cpu().numpy().astype(bool), y.detach().cpu().numpy().astype(bool)
    return _surface_numpy((want,), p, g, symmetric, percentile, directed, class_thresholds)[0].to(y_pred.device)


def compute_average_surface_distance(y_pred, y, include_background=False, symmetric=False, distance_metric="euclidean"):
    """MONAI's compute_average_surface_distance on one-hot [B, C, *spatial] inputs -> float64 [B, C'] (C' = C - 1 without background), on the
    device of y_pred (_onehot_surface_metric)"""
    _check_metric(distance_metric)
    return _onehot_surface_metric("asd", y_pred, y, include_background, symmetric=symmetric)


def surface_distance_from_logits(logits, label, num_classes, include_background=True, symmetric=True):
    """AsDiscrete(argmax, to_onehot) on the logits + AsDiscrete(to_onehot) on the label + SurfaceDistanceMetric, fused: fp64 [B, C']"""
    return surface_metrics_from_logits(logits, label, num_classes, include_background=include_background, symmetric=symmetric, want=("asd",))[0]


# ------------------------------------------------------------------------------------------ Hausdorff distance
# MONAI 1.1.0 metrics/hausdorff_distance.py restated (parity unpinned): the edge sets and one-way distance lists of the surface distance above.

def _check_percentile(percentile):
    if percentile is not None and not 0 <= percentile <= 100:
        raise ValueError(f"percentile should be a value between 0 and 100, got {percentile}.")


def _list_percentile(d, percentile):
    """h of one distance list: NaN if it is empty, inf if it is all inf (one edge set is empty: numpy's percentile would interpolate
    inf - inf into NaN there), the maximum without a percentile (None or 0), else numpy's default ("linear") percentile written out"""
    n = d.shape[0]
    if n == 0:
        return math.nan
    if np.isinf(d).all():
        return math.inf
    if not percentile:
        return float(d.max())
    v = np.sort(d.astype(np.float64))
    pos = (percentile / 100) * (n - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, n - 1)
    return float(v[lo] + (v[hi] - v[lo]) * (pos - lo))


def hausdorff_distance_numpy(pred, gt, percentile=None, directed=False, use_scipy=True):
    """pred, gt: bool [B, C, *spatial] -> float64 [B, C] (compute_hausdorff_distance after ignore_background): per (b, c) the percentile
    (None or 0: the maximum) of d(pred -> gt), and the larger of that and d(gt -> pred)'s unless `directed`.  use_scipy as in
    average_surface_distance_numpy."""
    _check_percentile(percentile)
    nd = _ndimage() if use_scipy else None
    B, Cc = pred.shape[:2]
    hd = np.empty((B, Cc))
    for b, c in np.ndindex(B, Cc):
        ep, eg = _mask_edges(pred[b, c], gt[b, c], nd)
        h = _list_percentile(_surface_distance(ep, eg, nd), percentile)
        if not directed:
            h2 = _list_percentile(_surface_distance(eg, ep, nd), percentile)
            h = max(h, h2)              # NaN together (both lists empty) or inf together (one edge set empty)
        hd[b, c] = h
    return hd


def compute_hausdorff_distance(y_pred, y, include_background=False, distance_metric="euclidean", percentile=None, directed=False):
    """MONAI's compute_hausdorff_distance on one-hot [B, C, *spatial] inputs -> float64 [B, C'] on the device of y_pred (_onehot_surface_metric)"""
    _check_metric(distance_metric)
    _check_percentile(percentile)
    return _onehot_surface_metric("hd", y_pred, y, include_background, percentile=percentile, directed=directed)


def surface_metrics_from_logits(logits, label, num_classes, include_background=True, symmetric=True, percentile=None, directed=False,
                                want=("asd", "hd"), class_thresholds=None):
    """AsDiscrete(argmax, to_onehot) on the logits + AsDiscrete(to_onehot) on the label + the surface metrics named in `want` ("asd": average
    surface distance, "hd": Hausdorff distance, "nsd": normalized surface Dice at `class_thresholds`, one per class after include_background),
    fused: a tuple of fp64 [B, C'] in that order.  On a HIP device (fp32 [B, C, D, H, W] logits): ONE launch set over logits + labels, no
    one-hot volume (csrc/surface.hip); on CPU tensors (--infer_cpu) the restatements above.  Label values outside [0, C) belong to no class,
    as in dice_from_logits."""
    _check_percentile(percentile)
    want = (want,) if isinstance(want, str) else tuple(want)
    if "nsd" in want:
        class_thresholds = _check_thresholds(class_thresholds, num_classes - (0 if include_background else 1))
    if _kernels_take(logits) and logits.dtype == torch.float32 and logits.shape[1] == num_classes:
        from ..hip import ops
        return ops.surface_metrics(label.to(logits.device), logits=logits.contiguous(), include_background=include_background, symmetric=symmetric,
                                   percentile=percentile, directed=directed, want=want, class_thresholds=class_thresholds)
    classes = torch.arange(num_classes, device=logits.device).view(1, -1, *([1] * (logits.dim() - 2)))
    pred = logits.argmax(dim=1, keepdim=True) == classes
    lab = label.to(logits.device).reshape(logits.shape[0], 1, *logits.shape[2:]).long() == classes
    c0 = 0 if include_background else 1
    out = _surface_numpy(want, pred[:, c0:].cpu().numpy(), lab[:, c0:].cpu().numpy(), symmetric, percentile, directed, class_thresholds)
    return tuple(t.to(logits.device) for t in out)


def hausdorff_distance_from_logits(logits, label, num_classes, include_background=True, percentile=None, directed=False):
    """AsDiscrete(argmax, to_onehot) on the logits + AsDiscrete(to_onehot) on the label + HausdorffDistanceMetric, fused: fp64 [B, C']"""
    return surface_metrics_from_logits(logits, label, num_classes, include_background=include_background, percentile=percentile, directed=directed,
                                       want=("hd",))[0]


# ------------------------------------------------------------------------------------------ normalized surface Dice
# MONAI's SurfaceDiceMetric / compute_surface_dice (parity unpinned) stated on the edge sets and one-way distance lists of the surface distance
# above, crop and squeeze included: the share of both lists' distances that are <= the class's tolerance.

def _check_thresholds(class_thresholds, num_kept):
    """the tolerances as a list of floats: one per class after include_background, each finite and >= 0"""
    if class_thresholds is None:
        raise ValueError("class_thresholds is required: one tolerance per class.")
    taus = [float(t) for t in class_thresholds]
    if len(taus) != num_kept:
        raise ValueError(f"number of classes ({num_kept}) does not match number of class thresholds ({len(taus)}).")
    if any(not 0.0 <= t < math.inf for t in taus):
        raise ValueError(f"all class thresholds need to be finite and >= 0, got {taus}.")
    return taus


def _check_subvoxels(use_subvoxels):
    if use_subvoxels:
        raise NotImplementedError("use_subvoxels=True is not implemented")


def surface_dice_bound(tau):
    """the largest integer k with sqrt(float(k)) <= tau, at most 2^26 - 1 (above every squared distance in a volume of sides <= 4096): the
    integer bound the kernel compares squared distances with, d <= tau <=> d^2 <= k (csrc/surface.hip::sd_nsd_bound restated)"""
    lim = (1 << 26) - 1
    t2 = tau * tau
    k = int(math.floor(t2)) if t2 < lim else lim
    while k > 0 and math.sqrt(float(k)) > tau:
        k -= 1
    while k + 1 <= lim and math.sqrt(float(k + 1)) <= tau:
        k += 1
    return k


def surface_dice_numpy(pred, gt, class_thresholds, use_scipy=True):
    """pred, gt: bool [B, C, *spatial], one tolerance per channel -> float64 [B, C]: (#{d(pred -> gt) <= tau} + #{d(gt -> pred) <= tau}) over
    the two lists' lengths; NaN where both lists are empty, 0.0 where one edge set is empty (both lists all inf).  use_scipy as in
    average_surface_distance_numpy."""
    nd = _ndimage() if use_scipy else None
    B, Cc = pred.shape[:2]
    taus = _check_thresholds(class_thresholds, Cc)
    nsd = np.empty((B, Cc))
    for b, c in np.ndindex(B, Cc):
        ep, eg = _mask_edges(pred[b, c], gt[b, c], nd)
        d_pg, d_gp = _surface_distance(ep, eg, nd), _surface_distance(eg, ep, nd)
        total = d_pg.shape[0] + d_gp.shape[0]
        within = int((d_pg <= taus[c]).sum()) + int((d_gp <= taus[c]).sum())
        nsd[b, c] = np.nan if total == 0 else np.float64(within) / np.float64(total)
    return nsd


def compute_surface_dice(y_pred, y, class_thresholds, include_background=False, distance_metric="euclidean", use_subvoxels=False):
    """MONAI's compute_surface_dice on one-hot [B, C, *spatial] inputs -> float64 [B, C'] on the device of y_pred, with the rules of DESIGN.md
    section 7.9 (_onehot_surface_metric)"""
    _check_metric(distance_metric)
    _check_subvoxels(use_subvoxels)
    return _onehot_surface_metric("nsd", y_pred, y, include_background, class_thresholds=class_thresholds)


def surface_dice_from_logits(logits, label, num_classes, class_thresholds, include_background=True):
    """AsDiscrete(argmax, to_onehot) on the logits + AsDiscrete(to_onehot) on the label + SurfaceDiceMetric, fused: fp64 [B, C']"""
    return surface_metrics_from_logits(logits, label, num_classes, include_background=include_background, want=("nsd",),
                                       class_thresholds=class_thresholds)[0]


# ------------------------------------------------------------------------------------------ cumulative metrics (MONAI 1.1.0 metrics/metric.py)
_REDUCTIONS = ("none", "mean", "sum", "mean_batch", "sum_batch", "mean_channel", "sum_channel")


def do_metric_reduction(f, reduction="mean"):
    """monai.metrics.utils.do_metric_reduction on a [B, C] tensor -> (reduced, not_nans): NaNs are left out and counted, inf is not"""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"Unsupported reduction: {reduction}, available options are {list(_REDUCTIONS)}.")
    nans = torch.isnan(f)
    not_nans = (~nans).float()
    t_zero = torch.zeros(1, device=f.device, dtype=f.dtype)
    if reduction == "none":
        return f, not_nans
    f = f.clone()
    f[nans] = 0
    if reduction == "mean":
        not_nans = not_nans.sum(dim=1)
        f = torch.where(not_nans > 0, f.sum(dim=1) / not_nans, t_zero)
        not_nans = (not_nans > 0).float().sum(dim=0)
        f = torch.where(not_nans > 0, f.sum(dim=0) / not_nans, t_zero)
    elif reduction == "sum":
        not_nans = not_nans.sum(dim=[0, 1])
        f = torch.sum(f, dim=[0, 1])
    elif reduction == "mean_batch":
        not_nans = not_nans.sum(dim=0)
        f = torch.where(not_nans > 0, f.sum(dim=0) / not_nans, t_zero)
    elif reduction == "sum_batch":
        not_nans = not_nans.sum(dim=0)
        f = f.sum(dim=0)
    elif reduction == "mean_channel":
        not_nans = not_nans.sum(dim=1)
        f = torch.where(not_nans > 0, f.sum(dim=1) / not_nans, t_zero)
    else:
        not_nans = not_nans.sum(dim=1)
        f = f.sum(dim=1)
    return f, not_nans


class Cumulative:
    """monai.metrics.Cumulative: extend(*batch_first_tensors) appends to one buffer per argument; get_buffer() concatenates them along the
    batch (one tensor for one buffer, else a list)"""

    def __init__(self):
        self.reset()

    def reset(self):
        self._buffers = None

    def extend(self, *data):
        if self._buffers is None:
            self._buffers = [[] for _ in data]
        for buf, d in zip(self._buffers, data):
            d = torch.as_tensor(d)
            buf.append(d.reshape(1) if d.dim() == 0 else d.detach())

    def get_buffer(self):
        if self._buffers is None:
            return None
        out = [torch.cat(b, dim=0) if b else None for b in self._buffers]
        return out[0] if len(out) == 1 else out


class _CumulativeMetric(Cumulative):
    """CumulativeIterationMetric: __call__(y_pred=, y=) computes the per-batch [B, C'] values, appends them and returns them"""

    def __init__(self, include_background=True, reduction="mean", get_not_nans=False):
        super().__init__()
        self.include_background, self.reduction, self.get_not_nans = include_background, reduction, get_not_nans

    def __call__(self, y_pred, y):
        ret = self._compute(y_pred, y)
        self.extend(ret)
        return ret

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        f, not_nans = do_metric_reduction(data, reduction or self.reduction)
        return (f, not_nans) if self.get_not_nans else f


class DiceMetric(_CumulativeMetric):
    """monai.metrics.DiceMetric (ignore_empty=True) on one-hot [B, C, ...] inputs: dice_metric above, channel 0 dropped without background"""

    def _compute(self, y_pred, y):
        d = dice_metric(y_pred.float(), y.float().to(y_pred.device))
        return d if self.include_background else d[:, 1:]


class SurfaceDistanceMetric(_CumulativeMetric):
    """monai.metrics.SurfaceDistanceMetric on one-hot [B, C, ...] inputs (compute_average_surface_distance above), float64 [B, C']"""

    def __init__(self, include_background=False, symmetric=False, distance_metric="euclidean", reduction="mean", get_not_nans=False):
        _check_metric(distance_metric)
        super().__init__(include_background, reduction, get_not_nans)
        self.symmetric, self.distance_metric = symmetric, distance_metric

    def _compute(self, y_pred, y):
        return compute_average_surface_distance(y_pred, y, include_background=self.include_background, symmetric=self.symmetric,
                                                distance_metric=self.distance_metric)


class HausdorffDistanceMetric(_CumulativeMetric):
    """monai.metrics.HausdorffDistanceMetric on one-hot [B, C, ...] inputs (compute_hausdorff_distance above), float64 [B, C']"""

    def __init__(self, include_background=False, distance_metric="euclidean", percentile=None, directed=False, reduction="mean", get_not_nans=False):
        _check_metric(distance_metric)
        _check_percentile(percentile)
        super().__init__(include_background, reduction, get_not_nans)
        self.distance_metric, self.percentile, self.directed = distance_metric, percentile, directed

    def _compute(self, y_pred, y):
        return compute_hausdorff_distance(y_pred, y, include_background=self.include_background, distance_metric=self.distance_metric,
                                          percentile=self.percentile, directed=self.directed)


class SurfaceDiceMetric(_CumulativeMetric):
    """monai.metrics.SurfaceDiceMetric on one-hot [B, C, ...] inputs (compute_surface_dice above), float64 [B, C']"""

    def __init__(self, class_thresholds, include_background=False, distance_metric="euclidean", reduction="mean", get_not_nans=False,
                 use_subvoxels=False):
        _check_metric(distance_metric)
        _check_subvoxels(use_subvoxels)
        super().__init__(include_background, reduction, get_not_nans)
        self.class_thresholds = _check_thresholds(class_thresholds, len(list(class_thresholds)) if class_thresholds is not None else 0)
        self.distance_metric, self.use_subvoxels = distance_metric, use_subvoxels

    def _compute(self, y_pred, y):
        return compute_surface_dice(y_pred, y, self.class_thresholds, include_background=self.include_background,
                                    distance_metric=self.distance_metric, use_subvoxels=self.use_subvoxels)


class GeneralizedDiceScore(_CumulativeMetric):
    """monai.metrics.GeneralizedDiceScore (1.1.0) on one-hot [B, C, ...] inputs: compute_generalized_dice above, one value per sample.
    aggregate() returns the reduced value alone (`metric.aggregate().item()`, reference utils/trainer.py:249)."""
    _AGGREGATE = ("none", "mean", "sum", "mean_batch", "sum_batch")

    def __init__(self, include_background=True, reduction="mean_batch", weight_type="square"):
        if reduction not in self._AGGREGATE:
            raise ValueError(f"reduction must be one of {list(self._AGGREGATE)}.")
        _check_weight_type(weight_type)
        super().__init__(include_background, reduction, False)
        self.weight_type = weight_type

    def _compute(self, y_pred, y):
        return compute_generalized_dice(y_pred, y, include_background=self.include_background, weight_type=self.weight_type)

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("The data to aggregate must be a PyTorch Tensor.")
        reduction = reduction or self.reduction
        if reduction not in self._AGGREGATE:
            raise KeyError(f"reduction must be one of {list(self._AGGREGATE)}.")
        if reduction in ("mean", "sum"):         # the [B] buffer as one channel: do_metric_reduction reduces the channel axis first
            data = data.reshape(-1, 1)
        f, _ = do_metric_reduction(data, reduction)
        return f

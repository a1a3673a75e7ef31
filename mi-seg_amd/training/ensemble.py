"""Flip test-time augmentation and model ensembling: the mean of cross-validation fold models (MONAI 1.1.0
transforms/post/array.py::MeanEnsemble / VoteEnsemble) and nnU-Net's mirror TTA - predict on every flip of the volume, un-flip, average - as
one miseg_ensemble_accumulate call per member (hip/ops.py::ensemble_accumulate, csrc/ensemble.hip) on the stitched logits.

The arithmetic is the kernel's: members are folded in one after the other, acc = fl(acc + fl(w * t)), and the last fold multiplies by
fl(1 / sum of the weights).  MONAI's MeanEnsemble computes mean(x * w) / mean(w) over a stacked tensor instead; MeanEnsemble and VoteEnsemble
here are restated from MONAI (which is not installed beside this package): parity with it is unpinned."""
import torch

from ..hip import lib as L
from ..hip import ops
from .inferer import sliding_window_inference

IDENTITY = (False, False, False)


def tta_flip_sets(axes):
    """all 2^k flip triples (one flag per spatial axis D, H, W) over the k distinct spatial axes `axes`, e.g. (0, 1, 2): nnU-Net's mirror TTA.
    Order: the axes sorted ascending count up in binary, the lowest axis fastest - entry m flips sorted(axes)[i] iff bit i of m is set - so the
    identity comes first: (0, 2) gives (F, F, F), (T, F, F), (F, F, T), (T, F, T)."""
    ax = sorted({int(a) for a in axes})
    if any(a < 0 or a > 2 for a in ax) or len(ax) != len(tuple(axes)):
        raise ValueError(f"tta_flip_sets: axes {tuple(axes)} must be distinct spatial axes out of 0, 1, 2")
    return [tuple(any(a == ax[i] and (m >> i) & 1 for i in range(len(ax))) for a in range(3)) for m in range(1 << len(ax))]


def _members(img):
    """a list or a stacked tensor of predictions -> list of contiguous fp32 [B, C, D, H, W] tensors and whether a batch dim was added"""
    items = list(img) if not torch.is_tensor(img) else list(img.unbind(0))
    if not items:
        raise ValueError("ensemble: no predictions")
    if any(not torch.is_tensor(t) or t.shape != items[0].shape or t.dim() not in (4, 5) for t in items):
        raise ValueError("ensemble: predictions must be tensors of one shape, [C, D, H, W] or [B, C, D, H, W]")
    added = items[0].dim() == 4
    return [(t[None] if added else t).to(torch.float32).contiguous() for t in items], added


def _member_weights(weights, n, Cc, who):
    """None, [n] or [n, C] -> float64 [n, C]"""
    if weights is None:
        return torch.ones(n, Cc, dtype=torch.float64)
    w = torch.as_tensor(weights, dtype=torch.float64).cpu()
    if w.dim() == 1 and w.numel() == n:
        w = w[:, None].repeat(1, Cc)
    if tuple(w.shape) != (n, Cc):
        raise ValueError(f"{who}: weights of shape {tuple(w.shape)} for {n} members of {Cc} channels (one per member, or [members, channels])")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or bool((w.sum(0) <= 0).any()):
        raise ValueError(f"{who}: weights must be finite, non-negative and not all zero")
    return w


def _out_scale(w):
    """fl(1 / sum of the members' weights) per class: the weights as the kernel sees them (rounded to fp32), summed in float64"""
    return (1.0 / w.to(torch.float32).to(torch.float64).sum(0)).to(torch.float32)


class MeanEnsemble:
    """MONAI 1.1.0's MeanEnsemble(weights=None), restated (parity unpinned): called with a list or a stacked tensor [E, ...] of E predictions
    ([C, D, H, W] or [B, C, D, H, W]), returns their weighted mean as fp32.  weights: None, one value per member, or [E, C] (per member and
    channel).  MONAI's result is mean(x * w) / mean(w); this one is the sequential sum fl(acc + fl(w * x)) over the members in order, times
    fl(1 / sum of w), through ops.ensemble_accumulate (device tensors: miseg_ensemble_accumulate; CPU tensors: its torch restatement)."""

    def __init__(self, weights=None):
        self.weights = weights

    def __call__(self, img):
        items, added = _members(img)
        w = _member_weights(self.weights, len(items), items[0].shape[1], "MeanEnsemble")
        acc = torch.empty_like(items[0])
        for k, x in enumerate(items):
            ops.ensemble_accumulate(x, acc, weight=w[k], first=k == 0, out_scale=_out_scale(w) if k == len(items) - 1 else None)
        return acc[0] if added else acc


class VoteEnsemble:
    """MONAI 1.1.0's VoteEnsemble(num_classes=None), restated (parity unpinned): majority voting over a list or a stacked tensor of E
    predictions.  num_classes given: the members are class maps with one channel ([1, D, H, W] or [B, 1, D, H, W]), the result is the class
    with the most votes in the same layout and dtype, the lowest class on a tie (first-maximum argmax of the counts).  num_classes None: the
    members are one-hot / binary maps [(B,) C, D, H, W] and a channel is 1 where more than half of the members say so (round(count / E),
    half to even as torch.round: an even split gives 0).  The counts are summed by ops.ensemble_accumulate."""

    def __init__(self, num_classes=None):
        self.num_classes = num_classes

    def __call__(self, img):
        raw = list(img) if not torch.is_tensor(img) else list(img.unbind(0))
        dtype = raw[0].dtype if raw and torch.is_tensor(raw[0]) else torch.float32
        items, added = _members(img)
        if self.num_classes is not None:
            n = int(self.num_classes)
            if items[0].shape[1] != 1:
                raise ValueError(f"VoteEnsemble: with num_classes the members are class maps with one channel, got {items[0].shape[1]}")
            items = [torch.stack([(x[:, 0] == c) for c in range(n)], 1).to(torch.float32).contiguous() for x in items]
        acc = torch.empty_like(items[0])
        for k, x in enumerate(items):
            ops.ensemble_accumulate(x, acc, first=k == 0)
        if self.num_classes is not None:
            out = torch.stack([ops.first_max_argmax(a) for a in acc])[:, None].to(dtype)
        else:
            out = torch.round(acc / float(len(items))).to(dtype)
        return out[0] if added else out


class EnsembleInferer:
    """Sliding-window inference of an ensemble: `predictors` (one callable or a list: the fold models) times `flips` (a list of flip triples,
    one flag per spatial axis D, H, W - tta_flip_sets(axes); None: no flip), members ordered predictor-major, flip-minor.  Call it like
    partial(sliding_window_inference, predictor=model, ...): inferer(inputs, modalities=None) -> fp32 [B, C, D, H, W]; it can be handed to
    evaluate.test(model_inferer=...) and is what predict_volume builds.

    Per member: torch.flip of the (one-channel) input, the project's sliding_window_inference, one ops.ensemble_accumulate call that un-flips
    the stitched logits and folds them into the accumulator (first on the first member, the scale fl(1 / sum of weights) on the last).  Alive
    at any time: the accumulator and one member's logits.  mode "mean_logits" | "mean_prob" | "vote" is the term a member contributes (its
    logits, their softmax, the one-hot of their first-maximum argmax; "vote" ignores the weights and is not scaled: the result holds vote
    counts).  Whatever the mode, the first-maximum argmax of the result is the ensemble's class map, so every consumer of logits takes it.
    weights: None, one value per predictor, or [predictors, classes]; the flips of a predictor share its weight.
    One predictor, no flip, "mean_logits" and no weights returns the plain inferer's tensor (no kernel: weight 1, scale 1).
    The window blend is sliding_window_inference's: `infer_mode` is its `mode` ("constant" | "gaussian"; the keyword `mode` here is the
    ensemble's), every other keyword (sigma_scale, padding_mode, cval, roi_weight_map, device, ...) goes through under its own name.  CPU
    inputs, or device="cpu", run the same loop on the torch restatement of the fold."""

    def __init__(self, predictors, roi_size, sw_batch_size, overlap=0.5, *, flips=None, mode="mean_logits", weights=None, infer_mode="constant",
                 **sliding_window_kwargs):
        self.predictors = list(predictors) if isinstance(predictors, (list, tuple)) else [predictors]
        if not self.predictors:
            raise ValueError("EnsembleInferer: no predictor")
        if mode not in L.ENSEMBLE_KINDS:
            raise ValueError(f"EnsembleInferer: mode {mode!r} is not one of {tuple(L.ENSEMBLE_KINDS)}")
        self.flips = [IDENTITY] if flips is None else [tuple(bool(v) for v in f) for f in flips]
        if not self.flips or any(len(f) != 3 for f in self.flips):
            raise ValueError(f"EnsembleInferer: flips {flips} must be a non-empty list of (D, H, W) flag triples")
        self.roi_size, self.sw_batch_size, self.overlap, self.mode, self.weights = roi_size, sw_batch_size, overlap, mode, weights
        self.keywords = dict(sliding_window_kwargs, mode=infer_mode)

    @property
    def members(self):
        return len(self.predictors) * len(self.flips)

    def _window(self, inputs, predictor, modalities):
        return sliding_window_inference(inputs, self.roi_size, self.sw_batch_size, predictor, overlap=self.overlap, modalities=modalities, **self.keywords)

    @torch.no_grad()
    def __call__(self, inputs, modalities=None):
        if self.members == 1 and self.mode == "mean_logits" and self.weights is None and self.flips[0] == IDENTITY:
            return self._window(inputs, self.predictors[0], modalities)
        acc = w = None
        k = 0
        for i, predictor in enumerate(self.predictors):
            for flip in self.flips:
                dims = [2 + a for a in range(3) if flip[a]]
                logits = self._window(torch.flip(inputs, dims) if dims else inputs, predictor, modalities).contiguous()
                if acc is None:
                    acc = torch.empty_like(logits)
                    w = _member_weights(self.weights, len(self.predictors), logits.shape[1], "EnsembleInferer")
                    scale = _out_scale(w.repeat_interleave(len(self.flips), 0))
                k += 1
                last = k == self.members and self.mode != "vote"
                ops.ensemble_accumulate(logits, acc, flip=flip, kind=self.mode, weight=w[i], first=k == 1, out_scale=scale if last else None)
                del logits
        return acc

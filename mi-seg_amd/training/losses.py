"""Dice / Focal / CE losses with MONAI 1.1.0 semantics as used by the reference (networks/lightning_monai.py:46-67,
utils/training_utils.py:6-33).  Restated from MONAI's public API (MONAI is a pinned third-party dependency of the reference,
monai~=1.1.0, not present here): PARITY UNPINNED by any reference test -- SURVEY.md Appendix B.

On a HIP device ``DiceFocalLoss`` / ``DiceCELoss`` / ``GeneralizedDiceFocalLoss`` (and ``GeneralizedDiceLoss``) with ``to_onehot_y=True, softmax=True`` (the only way LitMonai builds them) are ONE
fused pass for the loss and one for d(loss)/d(logits) (csrc/training.hip) instead of ~6 torch passes over the
[B, C, 96^3] logits plus their autograd tape.  The torch arithmetic below is what runs for CPU tensors (the reference's ``--infer_cpu``
validation computes its loss on CPU logits, lightning_monai.py:187-189) and is the plain-PyTorch reference the GPU tests compare the
kernels with.

Channel handling, MONAI 1.1.0:
  * DiceFocalLoss one-hots the target, then -- when ``include_background`` is False -- strips channel 0 from BOTH logits and target
    before calling its sub-losses, which it builds WITHOUT include_background / to_onehot_y: the Dice softmax therefore runs over the
    C-1 foreground logits only, and the focal term sees the same C-1 channels.
  * DiceCELoss delegates include_background / to_onehot_y to its DiceLoss (softmax over all C channels, channel 0 dropped afterwards)
    and applies nn.CrossEntropyLoss over all channels.
  * GeneralizedDiceFocalLoss passes include_background / to_onehot_y to BOTH sub-losses: the generalized Dice softmax runs over all C
    channels and channel 0 is dropped afterwards (the DiceCELoss order), the focal term drops channel 0 of the raw logits."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from ..hip import lib as L
from ..hip import ops


def _one_hot(label, num_classes):
    # label [B,1,...] integer-valued -> [B,C,...]
    return F.one_hot(label[:, 0].long(), num_classes).movedim(-1, 1).to(torch.float32)


class DiceLoss(torch.nn.Module):
    def __init__(self, include_background=True, to_onehot_y=False, softmax=False, squared_pred=False, smooth_nr=1e-5, smooth_dr=1e-5):
        super().__init__()
        self.include_background, self.to_onehot_y, self.softmax = include_background, to_onehot_y, softmax
        self.squared_pred, self.smooth_nr, self.smooth_dr = squared_pred, float(smooth_nr), float(smooth_dr)

    def forward(self, logits, target):
        n_ch = logits.shape[1]
        p = torch.softmax(logits, 1) if self.softmax else logits
        t = _one_hot(target, n_ch) if self.to_onehot_y else target
        if not self.include_background and n_ch > 1:
            p, t = p[:, 1:], t[:, 1:]
        dims = tuple(range(2, logits.dim()))
        inter = (p * t).sum(dims)
        if self.squared_pred:
            den = (t * t).sum(dims) + (p * p).sum(dims)
        else:
            den = t.sum(dims) + p.sum(dims)
        return (1.0 - (2.0 * inter + self.smooth_nr) / (den + self.smooth_dr)).mean()


class FocalLoss(torch.nn.Module):
    """MONAI 1.1.0 FocalLoss: sigmoid/BCE form on RAW logits (not softmax), gamma 2, mean over space then (b, c)."""

    def __init__(self, include_background=True, to_onehot_y=False, gamma=2.0):
        super().__init__()
        self.include_background, self.to_onehot_y, self.gamma = include_background, to_onehot_y, gamma

    def forward(self, logits, target):
        n_ch = logits.shape[1]
        t = _one_hot(target, n_ch) if self.to_onehot_y else target
        x = logits
        if not self.include_background and n_ch > 1:
            x, t = x[:, 1:], t[:, 1:]
        b, c = x.shape[:2]
        x = x.reshape(b, c, -1).float()
        t = t.reshape(b, c, -1).float()
        max_val = (-x).clamp(min=0)
        ce = x - x * t + max_val + ((-max_val).exp() + (-x - max_val).exp()).log()
        loss = (F.logsigmoid(-x * (t * 2 - 1)) * self.gamma).exp() * ce
        return loss.mean(-1).mean()


class _FusedSegLoss(Function):
    """loss = fused kernel pass 1 (+ fixed-order finalize); d(loss)/d(logits) = pass 2 from the saved per-(b, c) sums."""

    @staticmethod
    def forward(ctx, logits, label, cfg):
        logits = logits.contiguous()
        loss, sums = ops.seg_loss_fwd(logits, label, cfg)
        ctx.save_for_backward(logits, label, sums)
        ctx.cfg = cfg
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, label, sums = ctx.saved_tensors
        return ops.seg_loss_bwd(logits, label, ctx.cfg, sums, g), None, None


def _fusable(logits, target, to_onehot_y, softmax):
    return (logits.is_cuda and logits.dtype == torch.float32 and to_onehot_y and softmax and target.shape[1] == 1 and 2 <= logits.shape[1] <= 16
            and logits.shape[0] <= 64)


class DiceFocalLoss(torch.nn.Module):
    def __init__(self, include_background=True, to_onehot_y=False, softmax=False, squared_pred=False, smooth_nr=1e-5, smooth_dr=1e-5, gamma=2.0,
                 lambda_dice=1.0, lambda_focal=1.0):
        super().__init__()
        # MONAI 1.1.0 builds the sub-losses without include_background / to_onehot_y; forward() strips channel 0 itself
        self.dice = DiceLoss(True, False, softmax, squared_pred, smooth_nr, smooth_dr)
        self.focal = FocalLoss(True, False, gamma)
        self.include_background, self.to_onehot_y, self.softmax = include_background, to_onehot_y, softmax
        self.lambda_dice, self.lambda_focal = lambda_dice, lambda_focal
        self.cfg = ops.SegLossCfg(L.LOSS_DICE_FOCAL, include_background, squared_pred, smooth_nr, smooth_dr, gamma, lambda_dice, lambda_focal)

    def forward(self, logits, target):
        if _fusable(logits, target, self.to_onehot_y, self.softmax):
            return _FusedSegLoss.apply(logits, target, self.cfg)
        return self.forward_torch(logits, target)

    def forward_torch(self, logits, target):
        n_ch = logits.shape[1]
        t = _one_hot(target, n_ch) if (self.to_onehot_y and n_ch > 1) else target
        x = logits
        if not self.include_background and n_ch > 1:
            x, t = x[:, 1:], t[:, 1:]
        return self.lambda_dice * self.dice(x, t) + self.lambda_focal * self.focal(x, t)


class DiceCELoss(torch.nn.Module):
    def __init__(self, include_background=True, to_onehot_y=False, softmax=False, squared_pred=False, smooth_nr=1e-5, smooth_dr=1e-5,
                 lambda_dice=1.0, lambda_ce=1.0):
        super().__init__()
        self.dice = DiceLoss(include_background, to_onehot_y, softmax, squared_pred, smooth_nr, smooth_dr)
        self.to_onehot_y, self.softmax = to_onehot_y, softmax
        self.lambda_dice, self.lambda_ce = lambda_dice, lambda_ce
        self.cfg = ops.SegLossCfg(L.LOSS_DICE_CE, include_background, squared_pred, smooth_nr, smooth_dr, 0.0, lambda_dice, lambda_ce)

    def forward(self, logits, target):
        if _fusable(logits, target, self.to_onehot_y, self.softmax):
            return _FusedSegLoss.apply(logits, target, self.cfg)
        return self.forward_torch(logits, target)

    def forward_torch(self, logits, target):
        ce = F.cross_entropy(logits.float(), target[:, 0].long())
        return self.lambda_dice * self.dice(logits, target) + self.lambda_ce * ce


_W_TYPES = ("square", "simple", "uniform")


class GeneralizedDiceLoss(torch.nn.Module):
    """MONAI 1.1.0 GeneralizedDiceLoss, reduction="mean", batch=False (parity unpinned): per sample
    1 - (2 sum_c w I + smooth_nr) / (sum_c w (G + P) + smooth_dr) over the kept classes, w = 1/G^2 ("square") | 1/G ("simple") | 1 ("uniform")
    from the label count G alone (no gradient), an infinite w replaced by the sample's largest finite one.

    ``forward_torch`` covers ``sigmoid`` and ``softmax`` (or neither) and both ``to_onehot_y`` values; ``other_act``, ``batch=True`` and a
    ``reduction`` other than "mean" are refused with NotImplementedError at construction.  The fused kernel path needs
    ``to_onehot_y=True, softmax=True`` (the way the reference builds it, utils/training_utils.py:26-33)."""

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, w_type="square", reduction="mean",
                 smooth_nr=1e-5, smooth_dr=1e-5, batch=False):
        super().__init__()
        if other_act is not None:
            raise NotImplementedError("GeneralizedDiceLoss: other_act is not implemented (supported: sigmoid, softmax or neither)")
        if batch:
            raise NotImplementedError("GeneralizedDiceLoss: batch=True is not implemented")
        if reduction != "mean":
            raise NotImplementedError(f"GeneralizedDiceLoss: reduction '{reduction}' is not implemented (supported: 'mean')")
        if int(sigmoid) + int(softmax) > 1:
            raise ValueError("Incompatible values: more than 1 of [sigmoid=True, softmax=True, other_act is not None].")
        if w_type not in _W_TYPES:
            raise ValueError(f"Unsupported w_type: {w_type}, available options are {list(_W_TYPES)}.")
        self.include_background, self.to_onehot_y, self.sigmoid, self.softmax = include_background, to_onehot_y, sigmoid, softmax
        self.w_type, self.smooth_nr, self.smooth_dr = w_type, float(smooth_nr), float(smooth_dr)
        self.cfg = ops.SegLossCfg(L.LOSS_GDICE_FOCAL, include_background, False, smooth_nr, smooth_dr, 2.0, 1.0, 0.0, ops.gdice_weight_type(w_type))

    def forward(self, logits, target):
        if _fusable(logits, target, self.to_onehot_y, self.softmax):
            return _FusedSegLoss.apply(logits, target, self.cfg)       # lambda_other = 0: the focal sum is computed and not used
        return self.forward_torch(logits, target)

    def forward_torch(self, logits, target):
        n_ch = logits.shape[1]
        p = logits
        if self.sigmoid:
            p = torch.sigmoid(p)
        if self.softmax and n_ch > 1:
            p = torch.softmax(p, 1)                                    # over ALL channels; channel 0 leaves afterwards
        t = _one_hot(target, n_ch).to(p.dtype) if (self.to_onehot_y and n_ch > 1) else target.to(p.dtype)
        if not self.include_background and n_ch > 1:
            p, t = p[:, 1:], t[:, 1:]
        dims = tuple(range(2, logits.dim()))
        inter = (p * t).sum(dims)
        g = t.sum(dims)
        den = g + p.sum(dims)
        w = generalized_dice_weights(g.detach(), self.w_type)
        num = 2.0 * (inter * w).sum(1) + self.smooth_nr
        return (1.0 - num / ((den * w).sum(1) + self.smooth_dr)).mean()


def generalized_dice_weights(g, w_type):
    """[B, C'] label counts -> class weights: 1/G^2 | 1/G | 1; per sample an infinite weight becomes the largest finite one (0 if none is)"""
    g = g if g.dtype == torch.float64 else g.float()
    w = torch.ones_like(g) if w_type == "uniform" else (1.0 / g if w_type == "simple" else 1.0 / (g * g))
    infs = torch.isinf(w)
    w = torch.where(infs, torch.zeros_like(w), w)
    return w + infs.to(w.dtype) * w.max(dim=1, keepdim=True)[0]


class GeneralizedDiceFocalLoss(torch.nn.Module):
    """MONAI 1.1.0 GeneralizedDiceFocalLoss: lambda_gdl * GeneralizedDiceLoss + lambda_focal * FocalLoss, both built WITH include_background
    and to_onehot_y (reference utils/training_utils.py:26-33 builds it with to_onehot_y=True, softmax=True and the background included).

    ``forward_torch`` covers ``sigmoid`` / ``softmax`` / neither; ``other_act`` and ``focal_weight`` are refused with NotImplementedError
    at construction.  On a HIP device with ``to_onehot_y=True, softmax=True`` the loss is the fused MISEG_LOSS_GDICE_FOCAL pass."""

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, w_type="square", reduction="mean",
                 smooth_nr=1e-5, smooth_dr=1e-5, batch=False, gamma=2.0, focal_weight=None, lambda_gdl=1.0, lambda_focal=1.0):
        super().__init__()
        if focal_weight is not None:
            raise NotImplementedError("GeneralizedDiceFocalLoss: focal_weight is not implemented")
        if lambda_gdl < 0.0:
            raise ValueError("lambda_gdl should be no less than 0.0.")
        if lambda_focal < 0.0:
            raise ValueError("lambda_focal should be no less than 0.0.")
        self.generalized_dice = GeneralizedDiceLoss(include_background, to_onehot_y, sigmoid, softmax, other_act, w_type, reduction, smooth_nr, smooth_dr, batch)
        self.focal = FocalLoss(include_background, to_onehot_y, gamma)
        self.to_onehot_y, self.softmax = to_onehot_y, softmax
        self.lambda_gdl, self.lambda_focal = lambda_gdl, lambda_focal
        self.cfg = ops.SegLossCfg(L.LOSS_GDICE_FOCAL, include_background, False, smooth_nr, smooth_dr, gamma, lambda_gdl, lambda_focal, ops.gdice_weight_type(w_type))

    def forward(self, logits, target):
        if _fusable(logits, target, self.to_onehot_y, self.softmax):
            return _FusedSegLoss.apply(logits, target, self.cfg)
        return self.forward_torch(logits, target)

    def forward_torch(self, logits, target):
        return self.lambda_gdl * self.generalized_dice.forward_torch(logits, target) + self.lambda_focal * self.focal(logits, target)


def loss_from_argparse_args(args):
    """the reference's utils/training_utils.py:6-36: it never passes include_background, so every loss includes the background.  Its dice_ce
    branch reads ``args.squared_pred``, which its own parser never sets (the switch is ``--squared_dice``): ``squared_pred`` is read when the
    namespace has it, ``squared_dice`` otherwise."""
    if args.criterion == "dice_focal":
        return DiceFocalLoss(to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=args.smooth_nr, smooth_dr=args.smooth_dr)
    if args.criterion == "dice_ce":
        return DiceCELoss(to_onehot_y=True, softmax=True, squared_pred=args.squared_pred if hasattr(args, "squared_pred") else args.squared_dice,
                          smooth_nr=args.smooth_nr, smooth_dr=args.smooth_dr)
    if args.criterion == "generalized_dice_focal":
        return GeneralizedDiceFocalLoss(to_onehot_y=True, softmax=True, smooth_nr=args.smooth_nr, smooth_dr=args.smooth_dr)
    raise ValueError("Criterion {} not implemented, please chose another optimizer.".format(args.criterion))

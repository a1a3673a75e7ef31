"""Plain restatement of what csrc/training.hip's loss and Dice metric kernels compute, for tests/test_seg_loss_ref_cpu.py and
tests/test_hip_seg_loss_forms.py: dice_focal, dice_ce and gdice_focal with MONAI 1.1.0 channel handling (header of training/losses.py),
the per-(b, c) sums the forward kernel leaves for the backward one, and the per-class Dice and generalized Dice score after argmax.

Everything is torch on the CPU in the dtype of the logits handed in: float64 logits give the judge (no cast to float32 anywhere, unlike
FocalLoss.forward / DiceCELoss.forward_torch), float32 logits give "the float32 torch composition" whose own error against the judge sizes a
bound where the project's bar is too tight for honest fp32 arithmetic (parity.py, local_tol).  The gradient is autograd's on these formulas.
softplus and log-sigmoid are written in their stable forms, so x = -80 or 1e4 costs nothing."""
import math
from dataclasses import dataclass

import torch

KINDS = ("dice_focal", "dice_ce", "gdice_focal")
W_TYPES = ("square", "simple", "uniform")


@dataclass(frozen=True)
class Cfg:
    kind: str = "dice_focal"
    include_background: bool = True
    squared_pred: bool = False      # ignored by gdice_focal: the generalized Dice never squares the prediction
    smooth_nr: float = 1e-5
    smooth_dr: float = 1e-5
    gamma: float = 2.0              # ignored by dice_ce
    lambda_dice: float = 1.0
    lambda_other: float = 1.0       # lambda_focal | lambda_ce
    w_type: str = "square"          # gdice_focal only


def one_hot(label, C, dtype=torch.float64):
    """class ids [B, 1, ...] (any dtype) -> [B, C, S]; an id outside [0, C) gives an all-zero row"""
    lab = label.reshape(label.shape[0], 1, -1).to(torch.int64)
    return (lab == torch.arange(C, dtype=torch.int64).reshape(1, C, 1)).to(dtype)


def softplus(z):
    return z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))


def log_sigmoid(z):
    return -softplus(-z)


def focal_elements(x, t, gamma):
    """MONAI 1.1.0 FocalLoss per element on raw logits: exp(gamma logsigmoid(-x (2 t - 1))) * BCE-with-logits(x, t)"""
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    return torch.exp(gamma * log_sigmoid(-x * (2 * t - 1))) * ce


def gdice_weights(G, w_type):
    """[B, C'] label counts -> weights 1/G^2 | 1/G | 1; an infinite one becomes the sample's largest finite one, 0 if there is none"""
    w = torch.ones_like(G) if w_type == "uniform" else (1.0 / G if w_type == "simple" else 1.0 / (G * G))
    inf = torch.isinf(w)
    w = torch.where(inf, torch.zeros_like(w), w)
    return w + inf.to(w.dtype) * w.max(dim=1, keepdim=True)[0]


def _parts(x, t, cfg):
    """x, t: [B, C, S] in one dtype -> (p, t, x of the kept channels, softmax over its support)"""
    c0 = 0 if cfg.include_background else 1
    if cfg.kind == "dice_focal":
        x, t = x[:, c0:], t[:, c0:]               # channel 0 leaves BEFORE the softmax
        p = torch.softmax(x, 1)
    else:
        p = torch.softmax(x, 1)[:, c0:]           # softmax over all channels, channel 0 dropped after
        if cfg.kind == "gdice_focal":
            x = x[:, c0:]                         # the focal term drops channel 0 of the raw logits
        t_all, t = t, t[:, c0:]
        if cfg.kind == "dice_ce":
            return p, t, x, t_all
    return p, t, x, None


def loss_from_onehot(logits, onehot, cfg):
    """logits [B, C, ...], onehot [B, C, ...] of the same dtype -> 0-dim loss in that dtype"""
    B, C = logits.shape[:2]
    x, t = logits.reshape(B, C, -1), onehot.reshape(B, C, -1).to(logits.dtype)
    p, tk, xk, t_all = _parts(x, t, cfg)
    inter, G = (p * tk).sum(2), tk.sum(2)
    if cfg.kind == "gdice_focal":
        w = gdice_weights(G.detach(), cfg.w_type)
        num = 2.0 * (inter * w).sum(1) + cfg.smooth_nr
        den = ((G + p.sum(2)) * w).sum(1) + cfg.smooth_dr
        dice = (1.0 - num / den).mean()
    else:
        P = (p * p).sum(2) if cfg.squared_pred else p.sum(2)
        dice = (1.0 - (2.0 * inter + cfg.smooth_nr) / (G + P + cfg.smooth_dr)).mean()      # t is 0 / 1: t^2 = t
    if cfg.kind == "dice_ce":
        other = -(t_all * torch.log_softmax(x, 1)).sum(1).mean()
    else:
        other = focal_elements(xk, tk, cfg.gamma).mean()
    return cfg.lambda_dice * dice + cfg.lambda_other * other


def loss(logits, label, cfg):
    return loss_from_onehot(logits, one_hot(label, logits.shape[1], logits.dtype), cfg)


def loss_and_grad(logits, label, cfg, upstream=1.0):
    """-> (loss, upstream * d loss / d logits) in the dtype of `logits`, by autograd on the formulas above"""
    x = logits.detach().clone().requires_grad_(True)
    val = loss(x, label, cfg)
    (grad,) = torch.autograd.grad(val * upstream, x)
    return val.detach(), grad


def kernel_sums(logits, label, cfg):
    """what seg_loss_finalize_kernel leaves in `sums`: ([B, C, 3] of sum p t, sum p (p^2 when squared), sum t - zero for a channel outside
    the Dice term - and the total of the focal / CE elements)"""
    B, C = logits.shape[:2]
    x = logits.reshape(B, C, -1)
    t = one_hot(label, C, logits.dtype)
    c0 = 0 if cfg.include_background else 1
    p, tk, xk, t_all = _parts(x, t, cfg)
    sq = cfg.squared_pred and cfg.kind != "gdice_focal"
    out = torch.zeros(B, C, 3, dtype=logits.dtype)
    out[:, c0:, 0], out[:, c0:, 1], out[:, c0:, 2] = (p * tk).sum(2), ((p * p) if sq else p).sum(2), tk.sum(2)
    other = -(t_all * torch.log_softmax(x, 1)).sum() if cfg.kind == "dice_ce" else focal_elements(xk, tk, cfg.gamma).sum()
    return out, other


# ------------------------------------------------------------------------------------------------ the metric
def argmax_first(logits):
    """[B, C, S] -> [B, S] class of the maximum, the FIRST one on a tie: a later channel takes over only when strictly larger"""
    best, arg = logits[:, 0].clone(), torch.zeros(logits.shape[0], logits.shape[2], dtype=torch.int64)
    for c in range(1, logits.shape[1]):
        m = logits[:, c] > best
        best, arg = torch.where(m, logits[:, c], best), torch.where(m, torch.full_like(arg, c), arg)
    return arg


def metric_counts(logits, label_onehot):
    """logits [B, C, ...], label one-hot [B, C, ...] (an all-zero row: a voxel that counts for the prediction only) ->
    int64 [B, C, 3]: intersection, predicted, labelled voxels"""
    B, C = logits.shape[:2]
    pred = one_hot(argmax_first(logits.reshape(B, C, -1)).reshape(B, 1, -1), C, torch.int64)
    lab = label_onehot.reshape(B, C, -1).to(torch.int64)
    return torch.stack([(pred * lab).sum(2), pred.sum(2), lab.sum(2)], 2)


def dice_of_counts(counts):
    """[B, C, 3] -> float64 [B, C]: 2 I / (P + G), NaN where the class has no labelled voxel"""
    c = counts.double()
    return torch.where(c[..., 2] > 0, 2.0 * c[..., 0] / (c[..., 1] + c[..., 2]).clamp(min=1.0), torch.full_like(c[..., 0], math.nan))


def generalized_score_of_counts(counts, include_background, w_type):
    """[B, C, 3] -> float64 [B]: 2 sum w I / sum w (G + P) over the kept classes (a single class is always kept); where the denominator is 0:
    1 if no kept class is predicted anywhere, else 0"""
    c = counts.double()
    if not include_background and c.shape[1] > 1:
        c = c[:, 1:]
    w = gdice_weights(c[..., 2], w_type)
    num, den = 2.0 * (w * c[..., 0]).sum(1), (w * (c[..., 2] + c[..., 1])).sum(1)
    empty = torch.where(c[..., 1].sum(1) == 0, torch.ones_like(num), torch.zeros_like(num))
    return torch.where(den == 0, empty, num / den.clamp(min=1e-300))

"""TEST INFRASTRUCTURE ONLY: an independent restatement of MONAI 1.1.0's weighted window blend (sliding_window_inference with
mode="gaussian" or a roi_weight_map), shared by tests/test_sliding_window_gaussian_cpu.py and tests/test_hip_stitch_gaussian.py.

MONAI is absent from the reference tree and the reference never asks for this mode: PARITY UNPINNED BY THE REFERENCE.  Restated from MONAI's
published behaviour (data/utils.py::compute_importance_map, networks/layers/simplelayers.py::GaussianFilter / gaussian_1d(approx="erf"),
inferers/utils.py::sliding_window_inference):

  * the importance map is a one-hot volume (1 at roi // 2) run through a separable, zero-padded filter whose 1-D kernels are
    0.5 * (erf(t (x + 0.5)) - erf(t (x - 0.5))), clamped at 0, NOT normalised, t = 0.70710678 / sigma, sigma = roi * sigma_scale,
    x = -tail .. tail, tail = int(max(4 sigma, 0.5) + 0.5); divided by its maximum; clamped from below to max(smallest non-zero value, 1e-3);
  * windows are visited with the last axis fastest: sum[window] += map * pred, weights[window] += map, out = sum / weights, all fp32.

`conv_map` filters the way MONAI does (three F.conv3d passes, first spatial axis first); `closed_map` is the per-axis product the filter
collapses to on a one-hot input.  The window scan is oracle/sliding_window.py's, which walks the positions one by one."""
import math

import torch
import torch.nn.functional as F

from oracle import sliding_window as OSW


def kernel_1d(sigma):
    tail = int(max(sigma * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=torch.float32)
    t = 0.70710678 / math.fabs(sigma)
    return (0.5 * (torch.erf(t * (x + 0.5)) - torch.erf(t * (x - 0.5)))).clamp(min=0), tail


def _scales(roi, sigma_scale):
    return tuple(sigma_scale) if isinstance(sigma_scale, (tuple, list)) else (sigma_scale,) * len(roi)


def clamp_like_the_inferer(m):
    return torch.clamp(m, min=max(m[m != 0].min().item(), 1e-3))


def conv_map(roi, sigma_scale=0.125):
    """the convolution form: one-hot volume, one zero-padded cross-correlation per axis (axis 0 first)"""
    vol = torch.zeros((1, 1) + tuple(roi), dtype=torch.float32)
    vol[(0, 0) + tuple(r // 2 for r in roi)] = 1.0
    for axis, (r, s) in enumerate(zip(roi, _scales(roi, sigma_scale))):
        k, tail = kernel_1d(r * s)
        shape, pad = [1, 1, 1, 1, 1], [0, 0, 0]
        shape[2 + axis], pad[axis] = k.numel(), tail
        vol = F.conv3d(vol, k.reshape(shape), padding=pad)
    m = vol[0, 0]
    return clamp_like_the_inferer(m / m.max())


def closed_map(roi, sigma_scale=0.125):
    """the closed form: fl(fl(p0[i] * p1[j]) * p2[k]), p_a[i] = k_a[c_a - i + tail_a] (0 outside the kernel), written as plain loops"""
    prof = []
    for r, s in zip(roi, _scales(roi, sigma_scale)):
        k, tail = kernel_1d(r * s)
        p = torch.zeros(r, dtype=torch.float32)
        for i in range(r):
            j = r // 2 - i + tail
            if 0 <= j < k.numel():
                p[i] = k[j]
        prof.append(p)
    m = torch.empty(tuple(roi), dtype=torch.float32)
    for i in range(roi[0]):
        m[i] = (prof[0][i] * prof[1])[:, None] * prof[2][None, :]
    return clamp_like_the_inferer(m / m.max())


def weighted_loop(win, wmap, starts, roi, size):
    """MONAI's accumulation over resident windows win [n, C, roi...] (window-index order) on win's device: (sum / weights, weights)"""
    out = torch.zeros((win.shape[1],) + tuple(size), dtype=torch.float32, device=win.device)
    ws = torch.zeros(tuple(size), dtype=torch.float32, device=win.device)
    wmap = wmap.to(win.device)
    i = 0
    for d in starts[0]:
        for h in starts[1]:
            for w in starts[2]:
                sl = (slice(d, d + roi[0]), slice(h, h + roi[1]), slice(w, w + roi[2]))
                out[(slice(None),) + sl] += wmap * win[i]
                ws[sl] += wmap
                i += 1
    return out / ws, ws


@torch.no_grad()
def weighted_sliding_window_reference(inputs, roi_size, predictor, wmap, overlap=0.5, padding_mode="constant", cval=0.0):
    """inputs [B, C, D, H, W] on the CPU; predictor(window [1, C, roi...]) -> [1, K, roi...]; one window at a time in visiting order"""
    roi = (roi_size,) * 3 if isinstance(roi_size, int) else tuple(roi_size)
    orig = tuple(inputs.shape[2:])
    pad = OSW.symmetric_pad(orig, roi)
    if any(lo or hi for lo, hi in pad):
        flat = [v for lo_hi in reversed(pad) for v in lo_hi]
        inputs = F.pad(inputs, flat, value=cval) if padding_mode == "constant" else F.pad(inputs, flat, mode=padding_mode)
    size = tuple(inputs.shape[2:])
    total = weights = None
    for b in range(inputs.shape[0]):
        for d, h, w in OSW.window_origins(size, roi, overlap):
            win = (slice(d, d + roi[0]), slice(h, h + roi[1]), slice(w, w + roi[2]))
            pred = predictor(inputs[(slice(b, b + 1), slice(None)) + win]).float()
            if total is None:
                total = torch.zeros((inputs.shape[0], pred.shape[1]) + size)
                weights = torch.zeros(size)
            total[(b, slice(None)) + win] += wmap * pred[0]
            if b == 0:
                weights[win] += wmap
    out = total / weights
    crop = tuple(slice(lo, lo + s) for (lo, _), s in zip(pad, orig))
    return out[(slice(None), slice(None)) + crop]

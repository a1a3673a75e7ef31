"""Sliding-window inference with MONAI 1.1.0's geometry (reference lightning_monai.py:86-93,187):
interval = int(roi * (1 - overlap)) per axis, num = ceil((size - roi) / interval) + 1, start_i = min(i * interval, size - roi),
constant importance map, out = sum(pred) / count, symmetric zero pad when the image is smaller than the roi.
The reference only ever blends with mode="constant"; MONAI's other blending arguments (mode="gaussian", sigma_scale, padding_mode, cval,
roi_weight_map) are accepted as well: out = sum(map * pred) / sum(map) with the dense importance map of `importance_map` (DESIGN.md 7.6;
restated from MONAI 1.1.0, parity UNPINNED - MONAI is not part of the reference tree).

Unlike the reference (sw_batch_size must stay 1 with instance_cond because the one-element `modalities` is passed unchanged to every
window batch), windows of one volume are batched with the volume's modality broadcast.

On a HIP device the stitching is sized for 288 GB of HBM: every window's logits stay resident (700 windows x 6 classes x 96^3 fp32 =
14.9 GB for the 512 x 512 x 363 volume of BASELINE configs[4]) and ONE gather kernel (csrc/training.hip::stitch_kernel) writes
out = sum / count with the windows summed in window-index order -- MONAI's accumulation order, so the result is bit-identical to the
sequential `out[window] += pred` loop, without its 700 read-modify-write passes over the 2.3 GB accumulator and without atomics.
A volume whose window logits exceed the resident budget (a share of the card's FREE memory, `resident_budget`) is stitched in slabs of
depth layers: whenever the buffer is full, the depths that no later layer can touch are written (slab form of the same kernel, same
accumulation order) and the layers that still overlap the next depths move to the front of the buffer - MONAI's loop has no size limit
and neither has this one.
A weighted blend is the same single gather: the map (3.5 MB at 96^3, cache resident) is handed to the kernel, which forms
sum(fl(map * pred)) and sum(map) in window-index order and divides.
With `device=cpu` (the reference's --infer_cpu: logits stitched in host memory) or CPU inputs the plain loop below runs."""
import math

import torch
import torch.nn.functional as F


def _starts(size, roi, overlap):
    if size <= roi:
        return [0]
    interval = int(roi * (1 - overlap))
    interval = interval if interval > 0 else 1
    num = int(math.ceil((size - roi) / interval)) + 1
    return [min(i * interval, size - roi) for i in range(num)]


def window_grid(image_size, roi_size, overlap):
    sd, sh, sw = (_starts(s, r, overlap) for s, r in zip(image_size, roi_size))
    return [(d, h, w) for d in sd for h in sh for w in sw]


BLEND_MODES = ("constant", "gaussian")
PADDING_MODES = ("constant", "reflect", "replicate", "circular")       # torch.nn.functional.pad's
_MAP_CACHE = {}        # (roi, mode, sigma_scale, device) -> importance map; built once on the CPU, uploaded once per device


def _clamp_map(m):
    """what MONAI's sliding_window_inference does to any importance map: no weight below max(smallest non-zero weight, 1e-3)"""
    return torch.clamp(m, min=max(float(m[m != 0].min()), 1e-3))


def _gaussian_profile(n, sigma):
    """p[i], i < n: MONAI's erf-integrated, un-normalised gaussian_1d kernel (truncated = 4.0) as seen from a 1 at n // 2 through a zero-padded
    correlation (GaussianFilter applies F.conv*d): p[i] = k[n // 2 - i + tail], 0 outside the kernel"""
    tail = int(max(sigma * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=torch.float32)
    t = 0.70710678 / abs(sigma)
    k = (0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())).clamp(min=0)
    idx = n // 2 - torch.arange(n) + tail
    ok = (idx >= 0) & (idx < k.numel())
    return torch.where(ok, k[idx.clamp(0, k.numel() - 1)], torch.zeros((), dtype=torch.float32))


def importance_map(roi, mode="constant", sigma_scale=0.125, device=None):
    """dense fp32 [rd, rh, rw] weight of a window's voxels in the blend, as sliding_window_inference applies it (clamped).

    Restated from MONAI 1.1.0 (data/utils.py::compute_importance_map, networks/layers/simplelayers.py::GaussianFilter / gaussian_1d,
    inferers/utils.py); MONAI is not in the reference tree, so this parity is UNPINNED.
      constant: ones.
      gaussian: a one-hot volume (1 at roi // 2) filtered separably, first spatial axis first, zero padding, with the un-normalised kernels
        k_a(x) = max(0.5 * (erf(t (x + 0.5)) - erf(t (x - 0.5))), 0), t = 0.70710678 / sigma_a, sigma_a = roi_a * sigma_scale_a,
        |x| <= int(max(4 sigma_a, 0.5) + 0.5) - in fp32 exactly fl(fl(p0[i] * p1[j]) * p2[k]) (the closed form computed here; a product
        with the zeros of the one-hot volume adds nothing) - then divided by its maximum.
      both: clamped from below to max(smallest non-zero value, 1e-3): at sigma_scale 0.125 more than half of a 96^3 map sits on that clamp,
        so the map is not separable and is kept dense.
    Built once on the CPU in fp32 and cached per (roi, mode, sigma_scale, device): the CPU loop and the HIP kernel blend with the same bits.
    The returned tensor is shared: do not write to it."""
    roi = tuple(int(r) for r in roi)
    if mode not in BLEND_MODES:
        raise ValueError(f"importance_map: mode {mode!r} is not one of {BLEND_MODES}")
    ss = tuple(float(v) for v in sigma_scale) if isinstance(sigma_scale, (tuple, list)) else (float(sigma_scale),) * len(roi)
    if len(ss) != len(roi):
        raise ValueError(f"importance_map: sigma_scale {sigma_scale!r} needs one value or one per axis of {roi}")
    device = torch.device("cpu" if device is None else device)
    key = (roi, mode, ss if mode == "gaussian" else None, device)
    if key not in _MAP_CACHE:
        if device.type != "cpu":
            _MAP_CACHE[key] = importance_map(roi, mode, ss, "cpu").to(device)
        elif mode == "constant":
            _MAP_CACHE[key] = torch.ones(roi, dtype=torch.float32)
        else:
            if any(v <= 0 for v in ss):
                raise ValueError(f"importance_map: sigma_scale {sigma_scale!r} must be positive")
            p = [_gaussian_profile(r, r * v) for r, v in zip(roi, ss)]
            m = (p[0][:, None, None] * p[1][None, :, None]) * p[2][None, None, :]
            _MAP_CACHE[key] = _clamp_map(m / m.max()).contiguous()
    return _MAP_CACHE[key]


def sigma_scale_arg(v):
    """--infer_sigma_scale as `importance_map` takes it: the scalar default, one value, or one value per axis"""
    if isinstance(v, (list, tuple)):
        return float(v[0]) if len(v) == 1 else tuple(float(x) for x in v)
    return float(v)


def _checked_weight_map(roi_weight_map, roi):
    """a caller's roi_weight_map as the blend uses it: fp32, clamped like a computed map"""
    m = torch.as_tensor(roi_weight_map)
    if tuple(m.shape) != tuple(roi):
        raise ValueError(f"sliding_window_inference: roi_weight_map {tuple(m.shape)} does not have the roi's shape {tuple(roi)}")
    m = m.detach().to(torch.float32)
    if not bool(torch.isfinite(m).all()) or bool((m < 0).any()) or not bool((m != 0).any()):
        raise ValueError("sliding_window_inference: roi_weight_map must be finite, non-negative and not all zero")
    return _clamp_map(m).contiguous()


RESIDENT_LIMIT_BYTES = None      # None: RESIDENT_FRACTION of the device's free memory at the first window; a number overrides it (tests)
RESIDENT_FRACTION = 0.7


def resident_budget(device):
    """bytes of window logits kept in HBM at a time for the gather"""
    if RESIDENT_LIMIT_BYTES is not None:
        return int(RESIDENT_LIMIT_BYTES)
    return int(_free_bytes(device) * RESIDENT_FRACTION)


def _free_bytes(device):
    """bytes this process can still allocate on `device`: what the driver reports free PLUS what torch's caching allocator holds reserved but
    unallocated (after a training run most of the card sits there: mem_get_info alone would size the buffer at its minimum or refuse it)"""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free) + int(torch.cuda.memory_reserved(device)) - int(torch.cuda.memory_allocated(device))


class _SlabStitcher:
    """resident window logits of the depth layers [lo, ...) of one volume + the slab-wise gather (see the module docstring)"""

    def __init__(self, starts, roi, channels, size, device, sw_batch_size, weight=None):
        self.starts, self.roi, self.size = starts, roi, size
        self.weight = weight                                               # importance map on `device`, or None: the constant blend
        self.layer = len(starts[1]) * len(starts[2])                       # windows per depth layer
        nd = len(starts[0])
        per_window = channels * roi[0] * roi[1] * roi[2] * 4
        # layers that can overlap one depth (+ the one being filled); the buffer never holds fewer
        span = 1 + max(sum(1 for j in range(i) if starts[0][j] + roi[0] > starts[0][i]) for i in range(nd))
        budget = resident_budget(device)
        self.cap = min(nd, max(budget // (per_window * self.layer), span + 1))       # whole layers kept resident
        need = (self.cap * self.layer + (sw_batch_size if self.cap < nd else 0)) * per_window
        if need > _free_bytes(device):
            raise MemoryError(f"sliding-window stitching needs {need / 1e9:.1f} GB for {self.cap} resident depth layers of {self.layer} windows")
        self.win = torch.empty((self.cap * self.layer + (sw_batch_size if self.cap < nd else 0), channels) + tuple(roi), dtype=torch.float32, device=device)
        self.lo = self.computed = self.done = 0                            # first resident layer, windows computed, depths written

    def reset(self):
        self.lo = self.computed = self.done = 0

    def add(self, pred, out):
        """append the next windows' logits (window-index order); stitches a slab first when they would not fit"""
        n = pred.shape[0]
        if self.computed - self.lo * self.layer + n > self.win.shape[0]:
            self._flush(out, self.computed // self.layer)
        at = self.computed - self.lo * self.layer
        self.win[at:at + n].copy_(pred)
        self.computed += n

    def finish(self, out):
        self._flush(out, len(self.starts[0]))

    def _flush(self, out, upto):
        """write the depths that only the complete layers [lo, upto) cover; keep the layers that reach beyond them"""
        from ..hip import ops
        sd, rd = self.starts[0], self.roi[0]
        nxt = sd[upto] if upto < len(sd) else self.size[0]
        if nxt <= self.done or upto <= self.lo:
            if self.computed - self.lo * self.layer >= self.win.shape[0]:
                raise RuntimeError("sliding-window stitching: the resident buffer holds no complete depth layer to write")
            return
        whole = self.lo == 0 and upto == len(sd)
        ops.stitch_windows(self.win[:(upto - self.lo) * self.layer], out, (sd[self.lo:upto], self.starts[1], self.starts[2]), self.roi,
                           slab=None if whole else (self.done, nxt - self.done), weight=self.weight)
        self.done = nxt
        keep = next((j for j in range(self.lo, upto) if sd[j] + rd > nxt), upto)
        a, b = (keep - self.lo) * self.layer, self.computed - self.lo * self.layer
        if a and b > a:
            # move the kept layers to the front in place, front to back in non-overlapping pieces of <= a windows (destination below source: a
            # piece never overwrites windows that are still to be moved) - a clone of the tail was a second buffer of nearly the budget's size
            for o in range(0, b - a, a):
                n = min(a, b - a - o)
                self.win[o:o + n].copy_(self.win[a + o:a + o + n])
        self.lo = keep


@torch.no_grad()
def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.5, modalities=None, device=None, *, mode="constant",
                             sigma_scale=0.125, padding_mode="constant", cval=0.0, roi_weight_map=None, **kwargs):
    """inputs [B, C, D, H, W]; returns [B, out, D, H, W] (MONAI 1.1.0's stitching arithmetic).

    mode "constant" (the reference's): out = sum(pred) / count.  mode "gaussian" or a `roi_weight_map` [rd, rh, rw] (finite, non-negative, not
    all zero; it replaces the computed map): out = sum(map * pred) / sum(map) over the covering windows in window-index order, every product
    rounded before it is added, all in fp32 - see `importance_map` (sigma_scale: a scalar or one value per axis).  padding_mode / cval: how an
    image smaller than the roi is padded (torch.nn.functional.pad: constant, reflect, replicate, circular).  Further keywords go to
    `predictor`."""
    roi = (roi_size,) * 3 if isinstance(roi_size, int) else tuple(roi_size)
    if mode not in BLEND_MODES:
        raise ValueError(f"sliding_window_inference: mode {mode!r} is not one of {BLEND_MODES}")
    if padding_mode not in PADDING_MODES:
        raise ValueError(f"sliding_window_inference: padding_mode {padding_mode!r} is not one of {PADDING_MODES}")
    wmap = None                   # CPU importance map; None: every window weighs 1 (the path and the bits of the constant blend)
    if roi_weight_map is not None:
        wmap = _checked_weight_map(roi_weight_map, roi).cpu()
    elif mode != "constant":
        wmap = importance_map(roi, mode, sigma_scale)
    B = inputs.shape[0]
    orig = tuple(inputs.shape[2:])
    pads = [max(r - s, 0) for r, s in zip(roi, orig)]
    if any(pads):
        pp = []
        for p in reversed(pads):
            pp += [p // 2, p - p // 2]
        inputs = F.pad(inputs, pp, value=cval) if padding_mode == "constant" else F.pad(inputs, pp, mode=padding_mode)
    size = tuple(inputs.shape[2:])
    starts = tuple(_starts(s, r, overlap) for s, r in zip(size, roi))
    grid = [(d, h, w) for d in starts[0] for h in starts[1] for w in starts[2]]
    mods = None
    if modalities is not None:
        mods = [int(m) for m in (modalities.reshape(-1).tolist() if isinstance(modalities, torch.Tensor) else modalities)]
    on_hip = inputs.is_cuda and (device is None or torch.device(device).type == "cuda")
    out = cnt = win = None
    stitcher = None
    for b in range(B):
        for i in range(0, len(grid), sw_batch_size):
            chunk = grid[i:i + sw_batch_size]
            x = torch.cat([inputs[b:b + 1, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]] for (d, h, w) in chunk], 0)
            pred = predictor(x, [mods[b]] * len(chunk), **kwargs) if mods is not None else predictor(x, **kwargs)
            if out is None:
                dev = pred.device if on_hip else (device or pred.device)
                out = torch.empty((B, pred.shape[1]) + size, dtype=torch.float32, device=dev) if on_hip else \
                    torch.zeros((B, pred.shape[1]) + size, dtype=torch.float32, device=dev)
                if wmap is not None:           # the computed maps are uploaded once per device (cache), a caller's map once per call
                    wmap = wmap.to(dev) if roi_weight_map is not None else importance_map(roi, mode, sigma_scale, dev)
                if on_hip:
                    stitcher = _SlabStitcher(starts, roi, pred.shape[1], size, dev, sw_batch_size, weight=wmap)
                else:
                    cnt = torch.zeros((1, 1) + size, dtype=torch.float32, device=dev)
            if on_hip:
                stitcher.add(pred, out[b])
                continue
            for j, (d, h, w) in enumerate(chunk):
                p = pred[j].to(out.device, torch.float32)
                out[b, :, d:d + roi[0], h:h + roi[1], w:w + roi[2]] += p if wmap is None else wmap * p
                if b == 0:
                    cnt[0, 0, d:d + roi[0], h:h + roi[1], w:w + roi[2]] += 1.0 if wmap is None else wmap
        if on_hip:
            stitcher.finish(out[b])
            stitcher.reset()
    if not on_hip:
        out = out / cnt
    if any(pads):
        sl = [slice(None), slice(None)] + [slice(p // 2, p // 2 + s) for p, s in zip(pads, orig)]
        out = out[tuple(sl)]
    return out

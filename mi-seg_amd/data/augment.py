"""GPU-resident training augmentation: the random tail of the reference's MONAI chain (data/multi_modal.py:50-65) on volumes that stay
in HBM (the deterministic head -- load, orient, resample, ScaleIntensity, SpatialPad -- is what the reference's CacheDataset caches).

    RandCropByPosNegLabeld(pos=1, neg=1, num_samples=patches_training_sample, image_threshold=0)
    RandFlipd x 3 (axes 0, 1, 2, prob randFlipd_prob each), RandRotate90d(prob, max_k=3, axes (0, 1))
    RandScaleIntensityd(factors=0.1, prob), RandShiftIntensityd(offsets=0.1, prob)

The host draws the per-patch parameters (a torch.Generator: reproducible, rank-seedable) and ONE gather kernel per batch
(csrc/training.hip::augment_kernel) writes image and label patches - no intermediate crops, no per-transform passes.  MONAI's own random
stream cannot be reproduced (its RNG consumption order is an implementation detail of a dependency that is not vendored): the
DISTRIBUTIONS are restated, parity unpinned.

Beyond the reference's chain, all off by default (csrc/augment.hip::miseg_augment_affine, DESIGN.md section 7.11 - still one gather per batch):

    RandAffined(prob, rotate_range, scale_range, translate_range, padding_mode)      small free rotations / zooms about the crop centre
    RandAdjustContrastd(prob, gamma)                                                   v' = ((v - min) / (max - min + 1e-7))^gamma (max - min) + min
    RandGaussianNoised(prob, mean, std)                                                std drawn U(0, noise_std) per sample"""
import ctypes as C
import math

import numpy as np
import torch

from ..hip import lib as L
from ..hip import ops


class ResidentVolume:
    """one cached sample: image fp32 [C, D, H, W] and label [D, H, W] on the device + its foreground / background voxel lists
    (MONAI map_binary_to_indices: fg = label > 0, bg = label == 0 & image > image_threshold)"""

    def __init__(self, image, label, modality=0, image_threshold=0.0):
        if image.dim() != 4 or label.shape != image.shape[1:]:
            raise ValueError("image [C, D, H, W] and label [D, H, W] expected")
        self.image = image.float().contiguous()
        self.label = label.contiguous()
        self.modality = int(modality)
        flat = self.label.reshape(-1)
        self.fg = torch.nonzero(flat > 0).reshape(-1)
        self.bg = torch.nonzero((flat == 0) & (self.image.amax(0).reshape(-1) > image_threshold)).reshape(-1)


def affine_matrix(rotate=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """float32 [3, 3] sampling matrix M = Rz . Ry . Rx . diag(scale): it maps an OUTPUT offset from the crop centre to the INPUT offset that
    is read there (a sampling grid, as MONAI's RandAffine builds one - so scale > 1 reads a wider region: the content shrinks).  Axes are the
    patch axes (0, 1, 2) = (D, H, W); rotate[a] is the angle about axis a, in radians, with

        Rx(r) = [[1, 0, 0], [0, c, -s], [0, s, c]]     Ry(r) = [[c, 0, s], [0, 1, 0], [-s, 0, c]]     Rz(r) = [[c, -s, 0], [s, c, 0], [0, 0, 1]]

    (c, s = cos r, sin r: MONAI's create_rotate forms).  Sign convention: rotate = (0, 0, -pi / 2) samples like torch.rot90(x, 1, (0, 1)) -
    RandRotate90d's rot_k = 1 - and (0, 0, +pi / 2) like rot_k = 3.  Composed in float64; entries of the rotation product within 1e-7 of 0 or
    +-1 are snapped to them before the scaling, so that quarter turns are exact gathers (the kernel's integer path needs the exact identity,
    tests/test_hip_augment_affine.py the exact quarter turn); a drawn angle is moved by less than 1e-7 of a voxel per voxel of offset."""
    rx, ry, rz = (float(r) for r in rotate)
    c, s = math.cos(rx), math.sin(rx)
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    c, s = math.cos(ry), math.sin(ry)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    c, s = math.cos(rz), math.sin(rz)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    R = Rz @ Ry @ Rx
    for v in (0.0, 1.0, -1.0):
        R[np.abs(R - v) < 1e-7] = v
    return (R @ np.diag(np.asarray(scale, dtype=np.float64))).astype(np.float32)


def _triple(v, name):
    t = (float(v),) * 3 if isinstance(v, (int, float)) else tuple(float(x) for x in v)
    if len(t) == 1:
        t = t * 3
    if len(t) != 3:
        raise ValueError(f"{name}: one value or one per axis expected, got {v!r}")
    return t


class GpuAugmenter:
    def __init__(self, roi, patches_training_sample=1, randFlipd_prob=0.2, randRotate90d_prob=0.2, randScaleIntensityd_prob=0.1,
                 randShiftIntensityd_prob=0.1, pos=1.0, neg=1.0, seed=0, randAffined_prob=0.0, rotate_range=(0, 0, 0), scale_range=(0, 0, 0),
                 translate_range=(0, 0, 0), affine_padding_mode="border", randAdjustContrastd_prob=0.0, gamma_range=(0.5, 4.5),
                 randGaussianNoised_prob=0.0, noise_mean=0.0, noise_std=0.1):
        """rotate_range: radians per axis, drawn U(-r, r); scale_range: factor 1 + U(-s, s) per axis; translate_range: voxels, U(-t, t);
        affine_padding_mode: "border" | "zeros" for positions outside the VOLUME (the resample reads the resident volume, not the crop);
        gamma_range: (low, high) of U(low, high); noise_std: the std of a sample is drawn U(0, noise_std) (MONAI's rule)"""
        self.roi = (roi,) * 3 if isinstance(roi, int) else tuple(roi)
        self.n = int(patches_training_sample)
        if not 1 <= self.n <= L.AUG_MAX_SAMPLES:
            raise ValueError(f"patches_training_sample must be in 1..{L.AUG_MAX_SAMPLES}")
        self.p_flip, self.p_rot, self.p_scale, self.p_shift = randFlipd_prob, randRotate90d_prob, randScaleIntensityd_prob, randShiftIntensityd_prob
        self.pos_ratio = pos / (pos + neg)
        self.seed = int(seed)
        self.gen = torch.Generator().manual_seed(seed)
        self.p_affine, self.p_gamma, self.p_noise = float(randAffined_prob), float(randAdjustContrastd_prob), float(randGaussianNoised_prob)
        self.rotate_range, self.scale_range = _triple(rotate_range, "rotate_range"), _triple(scale_range, "scale_range")
        self.translate_range = _triple(translate_range, "translate_range")
        if affine_padding_mode not in L.AUG_PAD_MODES:
            raise ValueError(f"affine_padding_mode {affine_padding_mode!r} is not one of {tuple(L.AUG_PAD_MODES)}")
        self.padding_mode = affine_padding_mode
        self.gamma_range = tuple(float(g) for g in gamma_range)
        if len(self.gamma_range) != 2 or not 0.0 < self.gamma_range[0] <= self.gamma_range[1]:
            raise ValueError(f"gamma_range: 0 < low <= high expected, got {gamma_range!r}")
        self.noise_mean, self.noise_std = float(noise_mean), float(noise_std)
        self.draws = 0                 # calls that went through miseg_augment_affine so far: the `draw` half of the noise key
        self._minmax = None            # the gamma scratch (zero before its first use; every call hands it back zeroed)

    @classmethod
    def from_argparse_args(cls, args, seed=0):
        """the augmenter of a parsed command line (utils/parser.py::DATA_ARGS + the roi of MODEL_ARGS)"""
        return cls((args.roi_x, args.roi_y, args.roi_z), patches_training_sample=args.patches_training_sample, randFlipd_prob=args.randFlipd_prob,
                   randRotate90d_prob=args.randRotate90d_prob, randScaleIntensityd_prob=args.randScaleIntensityd_prob,
                   randShiftIntensityd_prob=args.randShiftIntensityd_prob, seed=seed, randAffined_prob=args.randAffined_prob,
                   rotate_range=args.rotate_range, scale_range=args.scale_range, translate_range=args.translate_range,
                   affine_padding_mode=args.affine_padding_mode, randAdjustContrastd_prob=args.randAdjustContrastd_prob, gamma_range=args.gamma_range,
                   randGaussianNoised_prob=args.randGaussianNoised_prob, noise_std=args.noise_std)

    def _u(self):
        return float(torch.rand((), generator=self.gen))

    def _sym(self, r):
        return (self._u() * 2.0 - 1.0) * r

    def draw(self, vol: ResidentVolume):
        """per-patch parameters (host side): list of dicts origin / flip / rot_k / scale / shift (+ centre: the voxel the crop was drawn around,
        before the crop was moved inside the volume - what the pos / neg balance is about) + affine (float32 [3, 4] = [M | t], affine_matrix's
        convention, or None) / gamma (float or None) / noise ((mean, std) or None).  A transform whose probability is 0 consumes no random
        number, and the new ones draw after the sample's existing draws: with them off the parameter stream is the one it always was."""
        D, H, W = vol.label.shape
        out = []
        for _ in range(self.n):
            use_fg = (self._u() < self.pos_ratio and vol.fg.numel() > 0) or vol.bg.numel() == 0
            idx = vol.fg if (use_fg and vol.fg.numel() > 0) else vol.bg
            if idx.numel() == 0:
                centre = (D // 2, H // 2, W // 2)
            else:
                flat = int(idx[int(torch.randint(0, idx.numel(), (), generator=self.gen))])
                centre = (flat // (H * W), (flat // W) % H, flat % W)
            # MONAI correct_crop_centers: the crop stays inside the volume
            origin = [min(max(c - r // 2, 0), s - r) for c, r, s in zip(centre, self.roi, (D, H, W))]
            flip = [int(self._u() < self.p_flip) for _ in range(3)]
            rot_k = int(torch.randint(1, 4, (), generator=self.gen)) if self._u() < self.p_rot else 0
            scale = (self._u() * 0.2 - 0.1) if self._u() < self.p_scale else 0.0
            shift = (self._u() * 0.2 - 0.1) if self._u() < self.p_shift else 0.0
            affine = gamma = noise = None
            if self.p_affine > 0 and self._u() < self.p_affine:
                rot = [self._sym(r) for r in self.rotate_range]
                zoom = [1.0 + self._sym(s) for s in self.scale_range]
                t = [self._sym(t) for t in self.translate_range]
                affine = np.concatenate([affine_matrix(rot, zoom), np.asarray(t, dtype=np.float32)[:, None]], axis=1)
            if self.p_gamma > 0 and self._u() < self.p_gamma:
                gamma = self.gamma_range[0] + self._u() * (self.gamma_range[1] - self.gamma_range[0])
            if self.p_noise > 0 and self._u() < self.p_noise:
                noise = (self.noise_mean, self._u() * self.noise_std)
            out.append(dict(origin=origin, flip=flip, rot_k=rot_k, scale=scale, shift=shift, centre=centre, affine=affine, gamma=gamma, noise=noise))
        return out

    def __call__(self, vol: ResidentVolume, params=None):
        """-> batch dict like the reference's collated loader output: image [n, C, r, r, r] fp32, label [n, 1, r, r, r], modality [n].
        params: dicts as draw() returns them; the keys affine / gamma / noise may be absent.  A batch in which no sample has one of the three
        is miseg_augment_crop's, as it always was; any other goes through miseg_augment_affine (one launch, two when a sample has gamma)."""
        params = params if params is not None else self.draw(vol)
        if any(s < r for s, r in zip(vol.label.shape, self.roi)):
            raise ValueError("volume smaller than the roi: pad it first (SpatialPadd is part of the cached, deterministic head)")
        n, Cc = len(params), vol.image.shape[0]
        img = torch.empty((n, Cc) + self.roi, dtype=torch.float32, device=vol.image.device)
        lab = torch.empty((n, 1) + self.roi, dtype=vol.label.dtype, device=vol.image.device)
        D, H, W = vol.label.shape
        batch = {"image": img, "label": lab, "modality": torch.full((n,), vol.modality, dtype=torch.int64)}
        if not any(p.get("affine") is not None or p.get("gamma") is not None or p.get("noise") is not None for p in params):
            samples = (L.AugSample * n)()
            for i, p in enumerate(params):
                samples[i] = L.AugSample((C.c_int * 3)(*p["origin"]), (C.c_int * 3)(*p["flip"]), p["rot_k"], p["scale"], p["shift"])
            q = L.Augment(C.sizeof(L.Augment), vol.image.data_ptr(), vol.label.data_ptr(), vol.label.element_size(), Cc, D, H, W, self.roi[0], self.roi[1],
                          self.roi[2], n, img.data_ptr(), lab.data_ptr(), C.cast(samples, C.c_void_p))
            ops._call("miseg_augment_crop", q)
            return batch
        if self._minmax is None or self._minmax.device != vol.image.device:
            self._minmax = torch.zeros(L.AUG_AFFINE_SCRATCH_BYTES // 4, dtype=torch.int32, device=vol.image.device)
        augment_affine(vol.image, vol.label, self.roi, params, padding_mode=self.padding_mode, seed=self.seed, draw=self.draws, minmax=self._minmax,
                       out_image=img, out_label=lab)
        self.draws += 1
        return batch


def augment_affine(image, label, roi, samples, padding_mode="border", seed=0, draw=0, minmax=None, out_image=None, out_label=None):
    """One miseg_augment_affine call (csrc/augment.hip): image fp32 [C, D, H, W] and label [D, H, W] (1, 4 or 8 byte elements) on the device,
    samples: dicts (affine_sample) -> (image fp32 [n, C, roi], label [n, 1, roi]).  minmax: the int32 [64] gamma scratch, zero before its
    first use (the call hands it back zeroed); needed when a sample has gamma.  The noise of sample i is a function of (seed, draw, i)."""
    n, Cc = len(samples), image.shape[0]
    roi = tuple(roi)
    if not (image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and label.is_contiguous() and label.device == image.device):
        raise ValueError("augment_affine: contiguous device tensors expected, the image in float32")
    if out_image is None:
        out_image = torch.empty((n, Cc) + roi, dtype=torch.float32, device=image.device)
    if out_label is None:
        out_label = torch.empty((n, 1) + roi, dtype=label.dtype, device=image.device)
    arr = (L.AugAffineSample * max(n, 1))()
    for i, p in enumerate(samples):
        arr[i] = affine_sample(p)
    D, H, W = label.shape
    q = L.AugmentAffine(C.sizeof(L.AugmentAffine), image.data_ptr(), label.data_ptr(), label.element_size(), Cc, D, H, W, roi[0], roi[1], roi[2], n,
                        out_image.data_ptr(), out_label.data_ptr(), C.cast(arr, C.c_void_p), L.AUG_PAD_MODES[padding_mode], int(seed) & (2 ** 64 - 1),
                        int(draw) & (2 ** 64 - 1), None if minmax is None else minmax.data_ptr())
    ops._call("miseg_augment_affine", q)
    return out_image, out_label


def affine_sample(p):
    """a sample dict -> the miseg_aug_affine_sample of the C ABI.  The matrix is `affine` (float32 [3, 4] = [M | t], draw()'s key) or `m` [3, 3]
    and `t` [3]; absent / None: the exact identity.  `gamma`: a float, absent / None / <= 0 = off.  The noise is `noise` = (mean, std) or
    `noise_mean` / `noise_std`; absent / None / std <= 0 = off."""
    a = p.get("affine")
    if a is None and p.get("m") is not None:
        a = np.concatenate([np.asarray(p["m"], dtype=np.float32).reshape(3, 3), np.asarray(p.get("t", (0, 0, 0)), dtype=np.float32).reshape(3, 1)], axis=1)
    a = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), dtype=np.float32)], axis=1) if a is None else np.asarray(a, dtype=np.float32)
    if a.shape != (3, 4):
        raise ValueError("affine: a [3, 4] matrix [M | t] expected")
    gamma, noise = p.get("gamma"), p.get("noise")
    mean, std = noise if noise is not None else (p.get("noise_mean", 0.0), p.get("noise_std", 0.0))
    return L.AugAffineSample((C.c_int * 3)(*p["origin"]), (C.c_int * 3)(*p["flip"]), p["rot_k"], (C.c_float * 9)(*a[:, :3].reshape(-1).tolist()),
                             (C.c_float * 3)(*a[:, 3].tolist()), p["scale"], p["shift"], 0.0 if gamma is None else gamma, mean, std)
